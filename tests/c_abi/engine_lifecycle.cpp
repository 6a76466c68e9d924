// Drives every allocator of the engine's host driver once and destroys the context: built with -fsanitize=address and linked
// against the SIMT-emulated library (tests/simt_emu/libvello_emu.so, whose hipMalloc is calloc), LeakSanitizer reports any device
// buffer or staging block that vello_hip_destroy forgets.  Exits 0 only if every call returned VELLO_HIP_OK.
// tests/test_abi.py::test_destroy_frees_every_device_buffer builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "vello_amd/csrc/host/renderer.hpp"

using namespace vello;

namespace {

constexpr uint32_t W = 64, H = 48;

#define OK(call)                                                                                         \
    do {                                                                                                 \
        const int r_ = (call);                                                                           \
        if (r_ != VELLO_HIP_OK) {                                                                        \
            std::fprintf(stderr, "%s:%d: %s = %d: %s\n", __FILE__, __LINE__, #call, r_, vello_hip_last_error(ctx)); \
            return 1;                                                                                    \
        }                                                                                                \
    } while (0)

kurbo::BezPath polygon(double cx, double cy, double r, int k) {
    kurbo::BezPath p;
    for (int i = 0; i < k; i++) {
        const double a = 6.283185307179586 * i / k;
        const kurbo::Point q{cx + r * std::cos(a), cy + r * std::sin(a)};
        if (i == 0) p.move_to(q);
        else p.line_to(q);
    }
    p.close_path();
    return p;
}

// `n` small fills and a stroke
void shapes(Scene &s, int n, double x0) {
    for (int i = 0; i < n; i++)
        s.fill(Fill::NonZero, Affine::translate(x0 + 3.0 * i, 4.0 + 2.0 * (i % 5)), Color{0.1f * (i % 10), 0.5f, 1.0f - 0.1f * (i % 10), 0.8f},
               polygon(6.0, 6.0, 5.0, 3 + i % 6));
    s.stroke(kurbo::Stroke::make(1.5), Affine::identity(), Color{1.f, 1.f, 1.f, 1.f}, kurbo::path_elements(kurbo::Circle{{x0 + 10.0, 24.0}, 9.0}, 0.1));
}

struct Packed {
    std::vector<uint8_t> bytes;
    vello_hip_layout layout;
    std::vector<uint32_t> ramps;
    uint32_t n_ramps = 0;
};

void pack(vello_encoding::Resolver &resolver, const Scene &s, Packed &out, vello_encoding::Resolved *res_out = nullptr) {
    const vello_encoding::Resolved res = resolver.resolve(s.encoding(), out.bytes);
    static_assert(sizeof(out.layout) == sizeof(res.layout), "Layout");
    std::memcpy(&out.layout, &res.layout, sizeof out.layout);
    out.n_ramps = res.n_ramps;
    out.ramps.assign(res.ramps, res.ramps + (size_t)res.n_ramps * 512u);
    if (res_out) *res_out = res;
}

void sizes(const Encoding &e, uint32_t out[6]) {
    const size_t v[6] = {e.path_tags.size(), e.path_data.size(), e.draw_tags.size(), e.draw_data.size(), e.transforms.size(), e.styles.size()};
    for (int k = 0; k < 6; k++) out[k] = (uint32_t)v[k];
}

}  // namespace

int main() {
    // three fragments: solid shapes; a gradient among shapes; an image among shapes
    Scene frag[3];
    shapes(frag[0], 12, 2.0);
    vello_encoding::Gradient lin;
    lin.p1[0] = 40.0;
    lin.stops = {{0.0f, Color{1.f, 0.f, 0.f, 1.f}}, {1.0f, Color{0.f, 0.f, 1.f, 1.f}}};
    frag[1].fill(Fill::NonZero, Affine::identity(), Brush(lin), std::nullopt, kurbo::path_elements(kurbo::Circle{{32.0, 24.0}, 14.0}, 0.1));
    shapes(frag[1], 9, 20.0);
    vello_encoding::ImageBrush img;
    img.image.id = 7;
    img.image.width = img.image.height = 4;
    std::vector<uint8_t> texels(4u * 4u * 4u);
    for (size_t i = 0; i < texels.size(); i++) texels[i] = (uint8_t)(i * 37u + 11u) | (i % 4u == 3u ? 0xffu : 0u);
    img.image.data = std::make_shared<const std::vector<uint8_t>>(texels);
    frag[2].draw_image(img, Affine::translate(50.0, 30.0));
    shapes(frag[2], 7, 30.0);

    // the library: the three in a row, each fragment the ranges its append added
    Scene library;
    vello_hip_fragment frs[3];
    for (int k = 0; k < 3; k++) {
        uint32_t a[6], b[6];
        sizes(library.encoding(), a);
        library.append(frag[k], std::nullopt);
        sizes(library.encoding(), b);
        uint32_t(*range[6])[2] = {&frs[k].path_tags, &frs[k].path_data, &frs[k].draws, &frs[k].draw_data, &frs[k].transforms, &frs[k].styles};
        for (int s = 0; s < 6; s++) (*range[s])[0] = a[s], (*range[s])[1] = b[s];
    }
    vello_encoding::Resolver resolver;
    Packed lib, small, mid;
    vello_encoding::Resolved lib_res;
    pack(resolver, frag[0], small);
    pack(resolver, frag[1], mid);
    pack(resolver, library, lib, &lib_res);
    if (!lib_res.atlas_size || !lib_res.uploads || lib_res.uploads->size() != 1u || lib.n_ramps != 1u || lib.layout.n_paths < 24u) {
        std::fprintf(stderr, "the scene is not the one this program means to build\n");
        return 1;
    }
    const vello_encoding::ImageUpload up = (*lib_res.uploads)[0];

    std::vector<uint32_t> target((size_t)W * H), source(16u, 0xff336699u);
    const vello_hip_render_params area{W, H, 0xff000000u, VELLO_HIP_AA_AREA}, msaa16{W, H, 0xff000000u, VELLO_HIP_AA_MSAA16};
    vello_hip_capacities caps{1u << 16, 1u << 16, 1u << 16, 1u << 16, 1u << 16, 1u << 14, 1u << 16};

    vello_hip_ctx *ctx = nullptr;
    OK(vello_hip_create(0, VELLO_HIP_AA_MASK_ALL, &caps, &ctx));
    OK(vello_hip_set_frames_in_flight(ctx, 4));
    OK(vello_hip_set_frames_in_flight(ctx, 2));
    OK(vello_hip_upload_scene(ctx, lib.bytes.data(), lib.bytes.size(), &lib.layout, lib.ramps.data(), lib.n_ramps));
    OK(vello_hip_render_resident(ctx, &area, nullptr, 0));  // (into the lane's own output buffer)
    OK(vello_hip_render_resident(ctx, &msaa16, target.data(), 0));
    const float view[6] = {0.5f, 0.0f, 0.0f, 0.5f, 8.0f, 6.0f};
    OK(vello_hip_set_view_transform(ctx, view));
    OK(vello_hip_render_resident(ctx, &area, target.data(), 0));
    OK(vello_hip_set_view_transform(ctx, nullptr));
    for (const Packed *p : {&small, &lib, &mid})
        OK(vello_hip_render_frame(ctx, p->bytes.data(), p->bytes.size(), &p->layout, &area, p->ramps.data(), p->n_ramps, target.data(), 0));
    OK(vello_hip_upload_fragments(ctx, lib.bytes.data(), lib.bytes.size(), &lib.layout, lib.ramps.data(), lib.n_ramps, frs, 3));
    vello_hip_instance inst[7];
    for (uint32_t i = 0; i < 7u; i++) inst[i] = vello_hip_instance{i % 3u, {1.0f, 0.0f, 0.0f, 1.0f, 2.0f * (float)i, (float)i}};
    OK(vello_hip_render_instances(ctx, inst, 7, &msaa16, target.data(), 0));
    OK(vello_hip_resize_image_atlas(ctx, lib_res.atlas_size, lib_res.atlas_size));
    OK(vello_hip_write_image(ctx, up.x, up.y, 4, 4, texels.data(), 0));
    const vello_hip_image_copy copy{(uint64_t)(uintptr_t)source.data(), 0, up.x, up.y, 4, 4};  // (emulated device memory is host memory)
    OK(vello_hip_copy_images_device(ctx, &copy, 1, nullptr));
    OK(vello_hip_set_profiling(ctx, (1u << VELLO_HIP_STAGE_COUNT) - 1u));
    OK(vello_hip_render_resident(ctx, &msaa16, target.data(), 0));  // (its events stay with the lane: the times are never read)
    vello_hip_bump demand{};
    demand.lines = caps.lines + 1u;
    OK(vello_hip_grow_pools(ctx, &demand, nullptr));
    OK(vello_hip_sync(ctx));
    vello_hip_destroy(ctx);
    return 0;
}
