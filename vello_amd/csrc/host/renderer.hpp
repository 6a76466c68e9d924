// Mirror of vello::Renderer / RenderParams / AaConfig (vello/src/lib.rs:175-193, :357-369, :432-515).
// render_to_texture = Resolver::resolve (host) + the C-ABI call that replaces
// WgpuEngine::run_recording.  In the real drop-in this class is the Rust `Renderer` with its
// `engine` field swapped for the FFI binding shown in INTEGRATION.md.
#pragma once
#include <array>
#include <optional>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/vello_hip.h"
#include "scene.hpp"

namespace vello {

enum class AaConfig : uint32_t { Area = 0, Msaa8 = 1, Msaa16 = 2 };

struct RenderParams {
    Color base_color{0.f, 0.f, 0.f, 1.f};
    uint32_t width = 0, height = 0;
    AaConfig antialiasing_method = AaConfig::Area;
    // A view transform for this frame (vello_hip_set_view_transform: a vello_encoding::Transform, [m0 m1 m2 m3 t0 t1], composed in
    // front of every transform of the scene on the GPU); none by default.  It holds for this frame only.
    std::optional<std::array<float, 6>> view;
};

// What Renderer::override_image binds to an image id in place of its pixels (upstream: a wgpu texture, its origin and mip
// level, vello/src/lib.rs:536-555): the device address of the texel at the image's origin, on the renderer's device, and the
// bytes between its rows (0 = width * 4).  RGBA8 words, copied verbatim into the atlas.
struct DeviceImageSource {
    uint64_t src = 0;
    uint64_t stride = 0;
};

struct RendererOptions {
    int device = 0;
    uint32_t antialiasing_support = VELLO_HIP_AA_MASK_ALL;  // AaSupport::all()
    vello_hip_capacities capacities{};                      // zero = reference pool sizes
};

class Renderer {
  public:
    // Renderer::new: returns nullptr and fills *err when no gfx950 device is usable.
    static Renderer *create(const RendererOptions &options, std::string *err);
    ~Renderer();
    // texture: linear RGBA8 (Rgba8Unorm) buffer of `stride` bytes per row, device memory when
    // is_device.  Returns a VELLO_HIP_* code; error() describes the last failure.
    // src_stream (nullable hipStream_t): the stream whose work writes the override sources; the atlas copy waits for it and
    // it waits for the copy (vello_hip_copy_images_device).
    int render_to_texture(const Scene &scene, void *texture, size_t stride, bool is_device, const RenderParams &params,
                          void *src_stream = nullptr);
    // Renderer::override_image (lib.rs:536-545): `source` replaces the image's pixels whenever the resolver schedules the
    // image for upload (nullopt removes the override); the image is marked dirty.  Returns the previous source.
    std::optional<DeviceImageSource> override_image(const vello_encoding::ImageData &image, std::optional<DeviceImageSource> source);
    // Renderer::mark_override_image_dirty (lib.rs:547-555): the source's contents changed; copy it again when next used
    void mark_override_image_dirty(const vello_encoding::ImageData &image) { resolver_.mark_image_dirty(image); }
    const std::string &error() const { return error_; }
    vello_hip_ctx *engine() { return ctx_; }
    const vello_hip_bump &last_bump() const { return bump_; }

  private:
    Renderer() = default;
    vello_hip_ctx *ctx_ = nullptr;
    vello_encoding::Resolver resolver_;
    std::unordered_map<uint64_t, DeviceImageSource> overrides_;  // image id -> source (WgpuEngine::image_overrides)
    std::vector<vello_hip_image_copy> copies_;                   // the override uploads of one render
    std::vector<uint8_t> packed_;
    vello_hip_bump bump_{};
    std::string error_;
};

}  // namespace vello
