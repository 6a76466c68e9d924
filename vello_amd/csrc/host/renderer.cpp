// See renderer.hpp.
#include "renderer.hpp"

#include <cstring>
#include <string>

namespace vello {

Renderer *Renderer::create(const RendererOptions &options, std::string *err) {
    vello_hip_ctx *ctx = nullptr;
    int r = vello_hip_create(options.device, options.antialiasing_support, &options.capacities, &ctx);
    if (r != VELLO_HIP_OK) {
        if (err) *err = vello_hip_last_error(nullptr);
        return nullptr;
    }
    Renderer *re = new Renderer();
    re->ctx_ = ctx;
    return re;
}

Renderer::~Renderer() { vello_hip_destroy(ctx_); }

std::optional<DeviceImageSource> Renderer::override_image(const vello_encoding::ImageData &image, std::optional<DeviceImageSource> source) {
    resolver_.mark_image_dirty(image);
    std::optional<DeviceImageSource> previous;
    auto it = overrides_.find(image.id);
    if (it != overrides_.end()) {
        previous = it->second;
        if (!source) overrides_.erase(it);
    }
    if (source) overrides_[image.id] = *source;
    return previous;
}

int Renderer::render_to_texture(const Scene &scene, void *texture, size_t stride, bool is_device, const RenderParams &params,
                                void *src_stream) {
    // render::render_full -> Resolver::resolve (vello/src/render.rs:84-112, :165)
    vello_encoding::Resolved res = resolver_.resolve(scene.encoding(), packed_);
    const vello_encoding::Layout &layout = res.layout;
    // the persistent image atlas (render.rs:160-203)
    if (res.atlas_size) {
        // an upload with neither an override nor pixels is refused before anything is enqueued (wgpu_engine.rs:505-514 panics);
        // the frame's uploads are marked dirty again, so the next render that uses them uploads them
        copies_.clear();
        const vello_encoding::ImageUpload *empty = nullptr;
        for (size_t i = 0; res.uploads && i < res.uploads->size(); i++) {
            const vello_encoding::ImageUpload &u = (*res.uploads)[i];
            if (overrides_.count(u.image.id)) continue;
            if (u.image.width && u.image.height && (!u.image.data || u.image.data->empty())) {
                empty = &u;
                break;
            }
        }
        int ar = VELLO_HIP_OK;
        if (res.atlas_resized) ar = vello_hip_resize_image_atlas(ctx_, res.atlas_size, res.atlas_size);
        if (empty) {
            for (size_t i = 0; i < res.uploads->size(); i++) resolver_.mark_image_dirty((*res.uploads)[i].image);
            if (ar != VELLO_HIP_OK) {
                error_ = vello_hip_last_error(ctx_);
                return ar;
            }
            error_ = "Tried to draw an invalid empty image (id " + std::to_string(empty->image.id) +
                     "). Maybe it was registered to a different renderer, or unregistered before this render was submitted.";
            return VELLO_HIP_E_INVALID;
        }
        for (size_t i = 0; ar == VELLO_HIP_OK && res.uploads && i < res.uploads->size(); i++) {
            const vello_encoding::ImageUpload &u = (*res.uploads)[i];
            auto it = overrides_.find(u.image.id);
            if (it != overrides_.end()) {  // WgpuEngine: copy_texture_to_texture from the override (wgpu_engine.rs:486-504), batched
                copies_.push_back(vello_hip_image_copy{it->second.src, it->second.stride, u.x, u.y, u.image.width, u.image.height});
                continue;
            }
            if (u.image.data && u.image.data->size() >= (size_t)u.image.width * u.image.height * 4u)
                ar = vello_hip_write_image(ctx_, u.x, u.y, u.image.width, u.image.height, u.image.data->data(), 0);
        }
        if (ar == VELLO_HIP_OK && !copies_.empty())
            ar = vello_hip_copy_images_device(ctx_, copies_.data(), (uint32_t)copies_.size(), src_stream);
        if (ar != VELLO_HIP_OK) {
            for (size_t i = 0; res.uploads && i < res.uploads->size(); i++) resolver_.mark_image_dirty((*res.uploads)[i].image);
            error_ = vello_hip_last_error(ctx_);
            return ar;
        }
    }
    vello_hip_layout l;
    static_assert(sizeof(l) == sizeof(layout), "Layout");
    std::memcpy(&l, &layout, sizeof l);
    vello_hip_render_params p{params.width, params.height, params.base_color.premul_rgba8(), (uint32_t)params.antialiasing_method};
    if (params.view) {
        int vr = vello_hip_set_view_transform(ctx_, params.view->data());
        if (vr != VELLO_HIP_OK) {
            error_ = vello_hip_last_error(ctx_);
            return vr;
        }
    }
    int r = vello_hip_render(ctx_, packed_.data(), packed_.size(), &l, &p, res.ramps, res.n_ramps, texture, stride, is_device ? 1 : 0, &bump_);
    if (r != VELLO_HIP_OK) error_ = vello_hip_last_error(ctx_);
    if (params.view) (void)vello_hip_set_view_transform(ctx_, nullptr);  // (the frame's view, not the renderer's)
    return r;
}

}  // namespace vello
