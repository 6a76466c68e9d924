// pathtag scan + bbox_clear, one launch.
// Reference: pathtag_reduce / pathtag_reduce2 / pathtag_scan1 / pathtag_scan_{small,large} +
// bbox_clear (vello/src/render.rs:250-308, vello_shaders/shader/pathtag_scan.wgsl:28-76,
// shared/pathtag.wgsl:58-71, bbox_clear.wgsl:13-23).
// gfx950 design: 256 threads x 4 tag words per workgroup, tags read once (16 B per lane,
// coalesced), SWAR popcount reduction per word, wave64 shuffle scan + one LDS hop, then a
// single-pass decoupled look-back across workgroups (lookback.h).
#include "scan_body.h"

namespace vk {

__global__ void __launch_bounds__(256) k_pathtag_scan(Config cfg, uint32_t n_tag_words, uint32_t n_scene_words, const uint32_t *__restrict__ scene,
                                                      Control *control, unsigned long long *state,
                                                      TagMonoid *__restrict__ tag_monoids, PathBbox *__restrict__ path_bboxes) {
    pathtag_scan_workgroup(cfg, blockIdx.x, gridDim.x, n_tag_words, n_scene_words, scene, control, state, tag_monoids, path_bboxes);
}

void launch_pathtag_scan(const Frame &f, hipStream_t s) {
    uint32_t n_parts = (f.n_tag_words + PATHTAG_PART_WORDS - 1u) / PATHTAG_PART_WORDS;
    if (n_parts == 0) n_parts = 1;
    hipLaunchKernelGGL(k_pathtag_scan, dim3(n_parts), dim3(256), 0, s, f.cfg, f.n_tag_words, f.n_scene_words, f.scene, f.control,
                       f.pathtag_state, f.tag_monoids, f.path_bboxes);
}

// An indexed frame's first launch (SceneIndex, ctx.h): what the zero fill and k_pathtag_scan leave in the lane, without the scan.
// The zero region is cleared 16 bytes a thread; the control block -- its first 128 words -- is written by workgroup 0 a word a
// thread, so that the words the index knows (flatten's two list lengths that no frame can change, the scan's verdict) are stored
// once and by the thread that would have cleared them.  The path boxes are the template's, 8 bytes a thread (a PathBbox is three).
constexpr uint32_t FRAME_BEGIN_MAX_WG = 512u;
__global__ void __launch_bounds__(256) k_frame_begin(uint4 *zero, uint32_t zero_vec16, const unsigned long long *__restrict__ bbox_template, unsigned long long *__restrict__ path_bboxes,
                                                     uint32_t bbox_vec8, uint32_t n_strokes, uint32_t n_lines, uint32_t failed) {
    static_assert(sizeof(Control) == 512 && sizeof(PathBbox) == 24 && offsetof(Control, bump) == 0u && offsetof(Bump, failed) == 0u, "k_frame_begin");
    constexpr uint32_t CONTROL_VEC16 = sizeof(Control) / 16u;
    const uint32_t tid = threadIdx.x, stride = gridDim.x * 256u;
    if (blockIdx.x == 0u && tid < sizeof(Control) / 4u) {
        uint32_t v = 0u;
        if (tid == 0u) v = failed;  // bump.failed
        if (tid == offsetof(Control, heavy_count) / 4u + 1u) v = n_strokes;
        if (tid == offsetof(Control, heavy_count) / 4u + 2u) v = n_lines;
        reinterpret_cast<uint32_t *>(zero)[tid] = v;
    }
    for (uint32_t i = CONTROL_VEC16 + blockIdx.x * 256u + tid; i < zero_vec16; i += stride) zero[i] = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = blockIdx.x * 256u + tid; i < bbox_vec8; i += stride) path_bboxes[i] = bbox_template[i];
}

void launch_frame_begin(const Frame &f, hipStream_t s) {
    const uint32_t zero_vec16 = f.zero_bytes / 16u, bbox_vec8 = f.cfg.layout.n_paths * 3u;
    uint32_t grid = ((zero_vec16 > bbox_vec8 ? zero_vec16 : bbox_vec8) + 255u) / 256u;
    grid = grid < 1u ? 1u : grid > FRAME_BEGIN_MAX_WG ? FRAME_BEGIN_MAX_WG : grid;
    hipLaunchKernelGGL(k_frame_begin, dim3(grid), dim3(256), 0, s, reinterpret_cast<uint4 *>(f.control), zero_vec16,
                       reinterpret_cast<const unsigned long long *>(f.index_bboxes), reinterpret_cast<unsigned long long *>(f.path_bboxes), bbox_vec8, f.index_n_strokes,
                       f.index_n_lines, f.index_failed);
}

}  // namespace vk
