// Drives the host paths of the per-frame stroke scale -- vello_hip_set_stroke_scale, its refusals, the frames of every entry point
// under it with frames in flight, vello_hip_estimate_capacities_styled -- from a program of its own.  Built with
// -fsanitize=address,undefined together with the engine's sources in their SIMT-emulated form (device buffers are heap blocks there,
// so the per-lane style copies behind a scene's bytes are bounds-checked like any other allocation).  Exits 0 only if every call
// returned what the contract says.  tests/test_stroke_scale_emu.py::test_stroke_scale_host_paths_under_sanitizers builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "vello_amd/csrc/host/renderer.hpp"

using namespace vello;

namespace {

constexpr uint32_t W = 96, H = 64;

#define EXPECT(call, want)                                                                                          \
    do {                                                                                                            \
        const int r_ = (call);                                                                                      \
        if (r_ != (want)) {                                                                                         \
            std::fprintf(stderr, "%s:%d: %s = %d, not %d: %s\n", __FILE__, __LINE__, #call, r_, (int)(want), ctx ? vello_hip_last_error(ctx) : ""); \
            return 1;                                                                                               \
        }                                                                                                           \
    } while (0)
#define OK(call) EXPECT(call, VELLO_HIP_OK)

struct Packed {
    std::vector<uint8_t> bytes;
    vello_hip_layout layout;
};

// `n` stroked lines, a style entry each, and a fill
void strokes(Scene &s, int n) {
    for (int i = 0; i < n; i++) {
        kurbo::BezPath p;
        p.move_to(kurbo::Point{4.0 + 7.0 * (i % 12), 4.0 + 9.0 * (i / 12)});
        p.line_to(kurbo::Point{9.0 + 7.0 * (i % 12), 7.0 + 9.0 * (i / 12)});
        s.stroke(kurbo::Stroke::make(0.3 + 0.37 * (i % 9)), Affine::identity(), Color{1.f, 0.1f * (i % 10), 0.5f, 1.f}, p);
    }
    s.fill(Fill::NonZero, Affine::identity(), Color{0.2f, 0.4f, 0.9f, 0.7f}, kurbo::path_elements(kurbo::Circle{{48.0, 32.0}, 11.0}, 0.1));
}

void pack(vello_encoding::Resolver &resolver, const Scene &s, Packed &out) {
    const vello_encoding::Resolved res = resolver.resolve(s.encoding(), out.bytes);
    static_assert(sizeof(out.layout) == sizeof(res.layout), "Layout");
    std::memcpy(&out.layout, &res.layout, sizeof out.layout);
}

void sizes(const Encoding &e, uint32_t out[6]) {
    const size_t v[6] = {e.path_tags.size(), e.path_data.size(), e.draw_tags.size(), e.draw_data.size(), e.transforms.size(), e.styles.size()};
    for (int k = 0; k < 6; k++) out[k] = (uint32_t)v[k];
}

}  // namespace

int main() {
    vello_encoding::Resolver resolver;
    Scene one, few, many, library;
    strokes(one, 1);
    strokes(few, 30);
    strokes(many, 300);
    // a library of two fragments: the ranges each append added
    vello_hip_fragment frs[2];
    const Scene *parts[2] = {&one, &few};
    for (int k = 0; k < 2; k++) {
        uint32_t a[6], b[6];
        sizes(library.encoding(), a);
        library.append(*parts[k], std::nullopt);
        sizes(library.encoding(), b);
        uint32_t(*range[6])[2] = {&frs[k].path_tags, &frs[k].path_data, &frs[k].draws, &frs[k].draw_data, &frs[k].transforms, &frs[k].styles};
        for (int s = 0; s < 6; s++) (*range[s])[0] = a[s], (*range[s])[1] = b[s];
    }
    Packed p_one, p_few, p_many, p_lib;
    pack(resolver, one, p_one);
    pack(resolver, few, p_few);
    pack(resolver, many, p_many);
    pack(resolver, library, p_lib);

    std::vector<uint32_t> target((size_t)W * H);
    const vello_hip_render_params msaa{W, H, 0xff000000u, VELLO_HIP_AA_MSAA16}, area{W, H, 0xff000000u, VELLO_HIP_AA_AREA};
    vello_hip_capacities caps{1u << 16, 1u << 16, 1u << 16, 1u << 16, 1u << 16, 1u << 14, 1u << 16};
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float bad[][2] = {{nan, 0.f}, {inf, 0.f}, {-inf, 0.f}, {0.f, 0.f}, {-0.f, 0.f}, {-2.f, 0.f}, {1.f, nan}, {1.f, inf}, {1.f, -inf}, {1.f, -0.25f}};
    const float third[2] = {1.0f / 3.0f, 0.45f}, wide[2] = {6.0f, 0.0f}, unit[2] = {1.0f, 0.0f};

    vello_hip_ctx *ctx = nullptr;
    EXPECT(vello_hip_set_stroke_scale(nullptr, third), VELLO_HIP_E_INVALID);
    EXPECT(vello_hip_set_stroke_scale(nullptr, nullptr), VELLO_HIP_E_INVALID);
    OK(vello_hip_create(0, VELLO_HIP_AA_MASK_ALL, &caps, &ctx));
    // the setting before any scene is resident; refusals change nothing
    OK(vello_hip_set_stroke_scale(ctx, third));
    for (const auto &b : bad) EXPECT(vello_hip_set_stroke_scale(ctx, b), VELLO_HIP_E_INVALID);
    EXPECT(vello_hip_render_resident(ctx, &msaa, target.data(), 0), VELLO_HIP_E_INVALID);  // (no scene uploaded)
    OK(vello_hip_set_frames_in_flight(ctx, 4));
    for (const Packed *p : {&p_one, &p_many, &p_few}) {
        OK(vello_hip_upload_scene(ctx, p->bytes.data(), p->bytes.size(), &p->layout, nullptr, 0));
        const float *settings[5] = {third, wide, nullptr, unit, third};
        for (const float *s : settings) {
            OK(vello_hip_set_stroke_scale(ctx, s));
            OK(vello_hip_render_resident(ctx, s == wide ? &area : &msaa, target.data(), 0));
        }
        OK(vello_hip_sync(ctx));
    }
    // private scenes whose style counts go up and down, under the setting
    OK(vello_hip_set_stroke_scale(ctx, wide));
    for (const Packed *p : {&p_few, &p_many, &p_one, &p_many})
        OK(vello_hip_render_frame(ctx, p->bytes.data(), p->bytes.size(), &p->layout, &msaa, nullptr, 0, target.data(), 0));
    OK(vello_hip_sync(ctx));
    // under a view and a morph (the path-data copies lie behind the style copies)
    const float view[6] = {2.0f, 0.0f, 0.0f, 2.0f, -20.0f, -10.0f};
    OK(vello_hip_set_view_transform(ctx, view));
    OK(vello_hip_set_stroke_scale(ctx, third));
    OK(vello_hip_upload_scene(ctx, p_few.bytes.data(), p_few.bytes.size(), &p_few.layout, nullptr, 0));
    OK(vello_hip_render_resident_morphed(ctx, VELLO_HIP_PATH_DATA_SCENE, VELLO_HIP_PATH_DATA_SCENE, 0.0f, nullptr, nullptr, &msaa, target.data(), 0));
    OK(vello_hip_render_resident(ctx, &msaa, target.data(), 0));
    OK(vello_hip_run_stages(ctx, &msaa, VELLO_HIP_STAGE_FLATTEN, VELLO_HIP_STAGE_FINE));
    OK(vello_hip_run_stages(ctx, &msaa, VELLO_HIP_STAGE_COARSE, VELLO_HIP_STAGE_FINE));
    OK(vello_hip_set_view_transform(ctx, nullptr));
    // composed and retained frames
    OK(vello_hip_upload_fragments(ctx, p_lib.bytes.data(), p_lib.bytes.size(), &p_lib.layout, nullptr, 0, frs, 2));
    vello_hip_instance inst[5];
    for (uint32_t i = 0; i < 5u; i++) inst[i] = vello_hip_instance{i % 2u, {1.0f, 0.0f, 0.0f, 1.0f, 3.0f * (float)i, (float)i}};
    OK(vello_hip_set_stroke_scale(ctx, wide));
    OK(vello_hip_render_instances(ctx, inst, 5, &msaa, target.data(), 0));
    OK(vello_hip_render_instances(ctx, inst, 0, &msaa, target.data(), 0));  // (an empty list: no style entry, no launch)
    OK(vello_hip_retain_instances(ctx, inst, nullptr, 5));
    for (const float *s : {(const float *)wide, (const float *)nullptr, (const float *)third}) {
        OK(vello_hip_set_stroke_scale(ctx, s));
        OK(vello_hip_render_retained(ctx, nullptr, 0, nullptr, &msaa, target.data(), 0));
    }
    OK(vello_hip_sync(ctx));
    // the blocking entry point with auto-grow: pools sized from the styled estimate
    OK(vello_hip_set_auto_grow(ctx, 1));
    OK(vello_hip_set_stroke_scale(ctx, wide));
    vello_hip_bump bump{};
    OK(vello_hip_render(ctx, p_many.bytes.data(), p_many.bytes.size(), &p_many.layout, &msaa, nullptr, 0, target.data(), 0, 0, &bump));
    OK(vello_hip_set_stroke_scale(ctx, nullptr));
    OK(vello_hip_sync(ctx));
    vello_hip_destroy(ctx);
    ctx = nullptr;

    // the estimate: NULL is _view; monotone in s on lines and segments; the same refusals
    vello_hip_capacities plain{}, viewed{}, styled{}, last{};
    OK(vello_hip_estimate_capacities_view(p_many.bytes.data(), p_many.bytes.size(), &p_many.layout, &msaa, view, &viewed));
    OK(vello_hip_estimate_capacities_styled(p_many.bytes.data(), p_many.bytes.size(), &p_many.layout, &msaa, view, nullptr, &styled));
    if (std::memcmp(&viewed, &styled, sizeof viewed) != 0) {
        std::fprintf(stderr, "estimate_capacities_styled(stroke = NULL) is not estimate_capacities_view\n");
        return 1;
    }
    OK(vello_hip_estimate_capacities(p_many.bytes.data(), p_many.bytes.size(), &p_many.layout, &msaa, &plain));
    for (float s : {0.25f, 1.0f, 4.0f, 32.0f}) {
        const float st[2] = {s, 0.0f};
        OK(vello_hip_estimate_capacities_styled(p_many.bytes.data(), p_many.bytes.size(), &p_many.layout, &msaa, nullptr, st, &styled));
        if (s == 1.0f && std::memcmp(&plain, &styled, sizeof plain) != 0) {
            std::fprintf(stderr, "estimate_capacities_styled((1, 0)) is not estimate_capacities on a scene of finite widths\n");
            return 1;
        }
        if (s > 0.25f && (styled.lines < last.lines || styled.seg_counts < last.seg_counts || styled.segments < last.segments)) {
            std::fprintf(stderr, "estimate_capacities_styled is not monotone in s at s = %g\n", (double)s);
            return 1;
        }
        last = styled;
    }
    for (const auto &b : bad)
        EXPECT(vello_hip_estimate_capacities_styled(p_many.bytes.data(), p_many.bytes.size(), &p_many.layout, &msaa, nullptr, b, &styled), VELLO_HIP_E_INVALID);
    EXPECT(vello_hip_estimate_capacities_styled(p_many.bytes.data(), p_many.bytes.size(), &p_many.layout, &msaa, nullptr, third, nullptr), VELLO_HIP_E_INVALID);
    return 0;
}
