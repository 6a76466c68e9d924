/*
 * vello_hip.h -- C ABI of the MI355X (gfx950) engine that replaces vello's wgpu compute path.
 *
 * Drop-in boundary: everything above this file stays the reference's host code
 * (vello::Scene -> vello_encoding::Encoding -> Resolver::resolve -> packed scene bytes + Layout);
 * everything below it (vello/src/wgpu_engine.rs WgpuEngine::run_recording, the Recording built by
 * vello/src/render.rs:135-629, and the 22 WGSL entry points of vello_shaders/shader/) is replaced
 * by this library.  Plain pointers and sizes only; no C++/torch types.
 *
 * Reference interface replaced by each entry point:
 *   vello_hip_create           vello::Renderer::new                      vello/src/lib.rs:432-459
 *                              (+ shaders::full_shaders                  vello/src/shaders.rs:48-274)
 *   vello_hip_destroy          Drop for Renderer / WgpuEngine
 *   vello_hip_render           Renderer::render_to_texture               vello/src/lib.rs:474-515
 *                              = render_full + WgpuEngine::run_recording vello/src/render.rs:84-112,
 *                                                                        vello/src/wgpu_engine.rs:380-777
 *   vello_hip_render_frame     render_to_texture without the wait        vello/src/lib.rs:474-515, wgpu_engine.rs:757
 *   vello_hip_upload_scene     Command::Upload("vello.scene") +          vello/src/render.rs:229-232,
 *                              Command::UploadUniform("vello.config")    vello/src/recording.rs:124-140
 *   vello_hip_render_resident  the Dispatch/DispatchIndirect chain       vello/src/render.rs:250-502, :560-629
 *   vello_hip_resize_image_atlas  ImageProxy::new(atlas_width, atlas_height)  vello/src/render.rs:160-176
 *   vello_hip_write_image      Recording::write_image(image_atlas, x, y, ..) vello/src/render.rs:201-203
 *   vello_hip_copy_images_device  the image_overrides branch of         vello/src/wgpu_engine.rs:486-504,
 *                              Command::WriteImage (copy_texture_to_texture) vello/src/lib.rs:536-555
 *                              for Renderer::override_image / register_texture
 *   vello_hip_upload_fragments /  Scene::append(&other, Some(transform))  vello/src/scene.rs (append),
 *   vello_hip_render_instances    per instance + resolve + upload        vello_encoding/src/encoding.rs:95-152
 *   vello_hip_render_instances_painted  ... each appended scene encoded  vello_encoding/src/encoding.rs:280-290
 *                              with a solid brush of its own (encode_brush)
 *   vello_hip_retain_instances /  the same Scene::append per pair, hoisted  vello/src/scene.rs (append),
 *   vello_hip_render_retained /   out of the frame loop: the composed scene  vello_encoding/src/encoding.rs:95-152,
 *   vello_hip_release_retained    is kept, a frame brings only the          vello_encoding/src/math.rs:51-73
 *                              transforms of its appends (Transform::mul)
 *   vello_hip_render_retained_painted  ... and this frame's solid brushes  vello_encoding/src/encoding.rs:280-290
 *                              (encode_brush per appended scene)
 *   vello_hip_pick             (none upstream: the reference has no hit test; the contract is stated at the entry point)
 *   vello_hip_pick_rect        (none upstream either: marquee selection; the contract is stated at the entry point)
 *   vello_hip_sync             queue.submit + device.poll                vello/src/wgpu_engine.rs:757
 *   vello_hip_set_frames_in_flight  back-to-back queue.submit without waiting  vello/src/wgpu_engine.rs:757
 *   vello_hip_get_bump         the robust path's bump download           vello/src/lib.rs:730, :753-761
 *   vello_hip_grow_pools /     "TODO: apply logic to determine whether   vello/src/lib.rs:762-764,
 *   vello_hip_set_auto_grow    we need to rerun coarse" + pool sizes     vello_encoding/src/config.rs:398-408
 *   vello_hip_estimate_capacities  BumpEstimator::count_path / tally      vello_encoding/src/estimate.rs:54-190
 *   vello_hip_gather_frames /  (none upstream: one Renderer per wgpu Device;  SURVEY.md 8e
 *   vello_hip_gather_wait      the scenes-per-GPU exchange of BASELINE config C5)
 *   vello_hip_set_debug_flags  (test seam: reference-exact coarse output)  vello_shaders/shader/coarse.wgsl:156-471
 *   vello_hip_run_stages /     CpuShaderType::Present per-stage seam     vello/src/wgpu_engine.rs:57-61, :541-553,
 *   vello_hip_{read,write}_buffer  (CpuBinding byte buffers)             vello_shaders/src/cpu.rs:58-62
 *   vello_hip_set_profiling /  wgpu-profiler per-dispatch GPU timestamps vello/src/wgpu_engine.rs:570-588
 *   vello_hip_get_stage_ms
 */
#ifndef VELLO_HIP_H
#define VELLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vello_hip_ctx vello_hip_ctx;

/* vello_encoding::Layout, vello_encoding/src/resolve.rs:18-39 (10 x u32, offsets in u32 words) */
typedef struct vello_hip_layout {
    uint32_t n_draw_objects, n_paths, n_clips, bin_data_start;
    uint32_t path_tag_base, path_data_base, draw_tag_base, draw_data_base;
    uint32_t transform_base, style_base;
} vello_hip_layout;

/* vello::AaConfig, vello/src/lib.rs:175-193 */
enum { VELLO_HIP_AA_AREA = 0, VELLO_HIP_AA_MSAA8 = 1, VELLO_HIP_AA_MSAA16 = 2 };
/* vello::AaSupport bits for vello_hip_create(aa_mask) */
enum { VELLO_HIP_AA_MASK_AREA = 1, VELLO_HIP_AA_MASK_MSAA8 = 2, VELLO_HIP_AA_MASK_MSAA16 = 4, VELLO_HIP_AA_MASK_ALL = 7 };

/* vello::RenderParams, vello/src/lib.rs:357-369.  base_color is premultiplied RGBA8 packed with
 * R in the low byte (vello_encoding/src/config.rs:183). */
typedef struct vello_hip_render_params {
    uint32_t width, height;
    uint32_t base_color;
    uint32_t aa; /* VELLO_HIP_AA_* */
} vello_hip_render_params;

/* vello_encoding::BumpAllocators, vello_encoding/src/config.rs:24-37 */
typedef struct vello_hip_bump {
    uint32_t failed, binning, ptcl, tile, seg_counts, segments, blend, lines;
} vello_hip_bump;

/* Capacities of the bump-allocated pools in elements.  Zero fields take the reference's
 * hand-picked sizes (vello_encoding/src/config.rs:398-408). */
typedef struct vello_hip_capacities {
    uint32_t lines, bin_data, tiles, seg_counts, segments, blend_spill, ptcl;
} vello_hip_capacities;

/* Error codes (0 = ok).  Capacity overflow mirrors the reference protocol: the target is left
 * untouched (fine.wgsl:1070-1074) and additionally VELLO_HIP_E_CAPACITY is returned by
 * vello_hip_sync / vello_hip_render with the counters available through vello_hip_get_bump. */
enum {
    VELLO_HIP_OK = 0,
    VELLO_HIP_E_INVALID = -1,   /* bad argument / AA mode not enabled at create (render.rs:566-598 panics) / a packed scene
                                 * whose streams contradict each other: draw tags that need more draw data, info words,
                                 * clips or paths than the layout provides (refused at upload), or path tags that need more
                                 * path data, transforms or styles than the scene holds (found by the pathtag scan; the
                                 * target is left untouched and vello_hip_render / vello_hip_sync report it).  WebGPU's
                                 * robust buffer access absorbs such scenes upstream; HIP has none, so they are refused. */
    VELLO_HIP_E_HIP = -2,       /* HIP runtime error; see vello_hip_last_error */
    VELLO_HIP_E_NO_DEVICE = -3, /* no gfx950 device / kernels missing: never falls back to a CPU path */
    VELLO_HIP_E_CAPACITY = -4,  /* bump.failed != 0: a pool overflowed (the robust path grows the pools and renders again) */
    VELLO_HIP_E_INTERNAL = -5   /* a spin bound of the engine tripped (a look-back or k_front's grid barrier waited for a workgroup
                                 * that never arrived): the frame is discarded, the lane's counters are reset; NOT a pool overflow --
                                 * auto-grow does not treat it as one */
};

/* Stage ids (launch order; render.rs:250-502, :560-629).  Several reference dispatches are fused:
 * PATHTAG_SCAN = pathtag_reduce(+2)/scan(1)/scan + bbox_clear, DRAW_SCAN = draw_reduce + draw_leaf,
 * CLIP = clip_reduce + clip_leaf, PATH_COUNT/PATH_TILING include their *_setup dispatch.
 * A frame (and any vello_hip_run_stages range that holds both FLATTEN and DRAW_SCAN) runs DRAW_SCAN's workgroups in
 * FLATTEN's first launch -- the stage needs the scene and the pathtag scan only -- and then has no launch of its own: its
 * profiled time is an empty event pair; a range that starts at DRAW_SCAN launches it as a kernel. */
enum {
    VELLO_HIP_STAGE_PATHTAG_SCAN = 0,
    VELLO_HIP_STAGE_FLATTEN,
    VELLO_HIP_STAGE_DRAW_SCAN,
    VELLO_HIP_STAGE_CLIP,
    VELLO_HIP_STAGE_BINNING,
    VELLO_HIP_STAGE_TILE_ALLOC,
    VELLO_HIP_STAGE_PATH_COUNT,
    VELLO_HIP_STAGE_BACKDROP,
    VELLO_HIP_STAGE_COARSE,
    VELLO_HIP_STAGE_PATH_TILING,
    VELLO_HIP_STAGE_FINE,
    VELLO_HIP_STAGE_COUNT
};

/* Buffer ids for the differential-test seam (byte layouts = the reference's). */
enum {
    VELLO_HIP_BUF_SCENE = 0,
    VELLO_HIP_BUF_CONFIG,        /* ConfigUniform, 88 B */
    VELLO_HIP_BUF_TAG_MONOIDS,   /* PathMonoid[Tw], 20 B */
    VELLO_HIP_BUF_PATH_BBOXES,   /* PathBbox[P], 24 B */
    VELLO_HIP_BUF_BUMP,          /* BumpAllocators, 32 B */
    VELLO_HIP_BUF_LINES,         /* LineSoup[], 24 B */
    VELLO_HIP_BUF_DRAW_MONOIDS,  /* DrawMonoid[D], 16 B */
    VELLO_HIP_BUF_INFO_BIN_DATA, /* u32[] */
    VELLO_HIP_BUF_CLIP_INP,      /* Clip[K], 8 B */
    VELLO_HIP_BUF_CLIP_BBOXES,   /* f32x4[K] */
    VELLO_HIP_BUF_DRAW_BBOXES,   /* f32x4[D] */
    VELLO_HIP_BUF_BIN_HEADERS,   /* BinHeader[], 8 B */
    VELLO_HIP_BUF_PATHS,         /* Path[], 32 B */
    VELLO_HIP_BUF_TILES,         /* Tile[], 8 B */
    VELLO_HIP_BUF_SEG_COUNTS,    /* SegmentCount[], 8 B */
    VELLO_HIP_BUF_SEGMENTS,      /* PathSegment[], 24 B */
    VELLO_HIP_BUF_PTCL,          /* u32[] (after a frame with a damage rectangle: stale words in the blocks of tiles outside its window) */
    VELLO_HIP_BUF_BLEND_SPILL,   /* u32[] */
    VELLO_HIP_BUF_OUTPUT,        /* internal RGBA8 target, width*height*4 */
    VELLO_HIP_BUF_COUNT
};

/* Creates an engine bound to HIP device `device`.  Fails with VELLO_HIP_E_NO_DEVICE when no GPU is
 * present; there is no CPU fallback. */
int vello_hip_create(int device, uint32_t aa_mask, const vello_hip_capacities *caps /* nullable */, vello_hip_ctx **out);
void vello_hip_destroy(vello_hip_ctx *ctx);

/* One frame, host buffers in, blocking: upload + render + (optional) copy out.
 * `out_rgba8` receives un-premultiplied RGBA8 rows of `out_stride` bytes (fine.wgsl:1386-1397);
 * it is a device pointer when out_is_device != 0, else host memory (address, stride and what is written: THE TARGET at
 * vello_hip_render_resident).  `ramps` is the gradient
 * ramp texture (512 RGBA8 texels per ramp, vello_encoding/src/ramp_cache.rs:12) or NULL.
 * `bump_out` (nullable) receives the bump counters. */
int vello_hip_render(vello_hip_ctx *ctx, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                     const vello_hip_render_params *params, const uint32_t *ramps, uint32_t n_ramps, void *out_rgba8,
                     size_t out_stride, int out_is_device, vello_hip_bump *bump_out);

/* Split form used for steady-state measurement: the packed scene is made resident once ... */
int vello_hip_upload_scene(vello_hip_ctx *ctx, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                           const uint32_t *ramps, uint32_t n_ramps);
/* ... then each call enqueues one full frame (all stages) on the context's stream and returns
 * without waiting.  `out_device` may be NULL (render into the internal target only).  Resident frames ALWAYS show
 * the scene of the last vello_hip_upload_scene: scenes passed to vello_hip_render_frame are private to their frame
 * (VELLO_HIP_E_INVALID if no scene was ever uploaded).  The frame runs on the context's own (non-blocking) stream
 * (vello_hip_get_stream): work of the caller's streams on `out_device` -- clearing it, reading the previous frame -- has
 * to be finished or ordered against that stream by the caller, as with any wgpu texture shared between queues.
 *
 * THE TARGET (every entry point that takes one: vello_hip_render, _render_resident, _render_frame, _render_instances).
 * Device target: `out_device` and `out_stride` are multiples of 4; out_stride == 0 means width * 4, otherwise
 * width * 4 <= out_stride < 2^32 (a stride of 2^32 and more is refused, not supported).  Host target of vello_hip_render
 * (out_is_device == 0): any alignment; out_stride == 0 or out_stride >= width * 4.  The engine writes exactly the bytes
 * [y * out_stride, y * out_stride + width * 4) of each row y < height, and no other byte: padding between rows, the pixels
 * beside a sub-rectangle of a larger surface and everything behind the last row keep their contents.  A target that breaks
 * this is refused with VELLO_HIP_E_INVALID (vello_hip_last_error names the rule) before anything is uploaded or enqueued:
 * the target is untouched, the resident scene unchanged, and the in-flight rotation stays where it was. */
int vello_hip_render_resident(vello_hip_ctx *ctx, const vello_hip_render_params *params, void *out_device, size_t out_stride);
/* Animation form (every frame has its own scene): vello_hip_upload_scene + vello_hip_render_resident in one call
 * that does NOT wait for the frame.  The scene is copied into the private slot of the next in-flight buffer set
 * (only that set's previous frame is waited for), so with vello_hip_set_frames_in_flight(n > 1) the upload of frame
 * i+1 overlaps the rendering of frames i, i-1, ...  `scene` / `ramps` may be reused when the call returns; the target
 * is complete after vello_hip_sync_frame(0) / vello_hip_sync.  Replaces, per frame, the same reference calls as
 * vello_hip_render (vello/src/lib.rs:474-515) under wgpu's submit-without-wait (vello/src/wgpu_engine.rs:757). */
int vello_hip_render_frame(vello_hip_ctx *ctx, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                           const vello_hip_render_params *params, const uint32_t *ramps, uint32_t n_ramps, void *out_device,
                           size_t out_stride);

/* The image atlas: one RGBA8 texture that persists across frames (render.rs:160-176).  The Resolver owns
 * the packing: it patches every DrawImage's atlas xy (resolve.rs:300-316) and lists the images to (re)write.
 * resize discards the contents (zero-filled), as creating a new ImageProxy does.  Texel bytes are stored
 * verbatim; BGRA / straight-alpha images are normalised while sampling (fine.wgsl:829-858).
 * resize waits for the frames in flight.  write_image does not (wgpu's queue.write_texture is queued as well): it copies
 * the caller's pixels to pinned memory during the call and enqueues the transfer in submission order -- behind every
 * frame enqueued before it (they still sample the old texels), in front of every frame enqueued after it. */
int vello_hip_resize_image_atlas(vello_hip_ctx *ctx, uint32_t width, uint32_t height);
int vello_hip_write_image(vello_hip_ctx *ctx, uint32_t x, uint32_t y, uint32_t width, uint32_t height, const uint8_t *rgba8,
                          size_t stride /* bytes per source row; 0 = width*4 */);

/* One rectangle of a device-to-atlas copy: `src` is the device address (on the context's device) of the first of `height`
 * rows of `width` RGBA8 words, `src_stride` bytes apart (0 = width * 4).  Source address and stride are multiples of 4. */
typedef struct vello_hip_image_copy {
    uint64_t src;
    uint64_t src_stride;
    uint32_t x, y, width, height;
} vello_hip_image_copy;

/* Image overrides (Renderer::override_image / register_texture): copies `n` rectangles of device memory into the atlas in ONE
 * kernel launch (k_atlas_copy), texels verbatim (format and alpha type are applied while sampling, as for write_image).
 * Ordered like vello_hip_write_image -- behind every frame enqueued before it, in front of every frame enqueued after it --
 * and, when `src_stream` (a hipStream_t, nullable) is given, behind the work enqueued on it so far; `src_stream` then waits for
 * the copy, so work the caller enqueues there afterwards may overwrite the sources.  Nothing waits on the host.
 * VELLO_HIP_E_INVALID, with nothing enqueued, for a rectangle outside the atlas, a null or unaligned source of a rectangle
 * that is not empty, copies == NULL with n > 0, or (GPU builds) a source that is not device memory of the context's device.
 * n == 0 and empty rectangles do nothing.  The rectangles of one batch run concurrently: their destinations must not overlap
 * (no rectangle is "later" than another), and a source must not lie in the atlas itself. */
int vello_hip_copy_images_device(vello_hip_ctx *ctx, const vello_hip_image_copy *copies, uint32_t n, void *src_stream /* nullable hipStream_t */);

/* Robust dynamic memory.  vello_hip_grow_pools re-sizes every pool whose counter in `demand`
 * (from vello_hip_get_bump / bump_out after VELLO_HIP_E_CAPACITY) exceeds it, with 25 % headroom, on all in-flight
 * buffer sets; the caller then renders the frame again.  A stage that overflows stops the later stages
 * (shared/bump.wgsl:5-9), so one frame may need several rounds.  Returns VELLO_HIP_E_INVALID when nothing had to
 * grow.  With vello_hip_set_auto_grow(ctx, 1) the blocking vello_hip_render does these rounds itself and only
 * reports VELLO_HIP_E_CAPACITY if the demand cannot be met; every entry point that renders then also sizes the PTCL
 * pool for the target (64 words per tile are fixed, config.rs:408 allows ~2 Mpx of tiles) instead of failing with
 * VELLO_HIP_E_INVALID. */
int vello_hip_get_capacities(vello_hip_ctx *ctx, vello_hip_capacities *out);
int vello_hip_grow_pools(vello_hip_ctx *ctx, const vello_hip_bump *demand, vello_hip_capacities *new_caps /* nullable */);
int vello_hip_set_auto_grow(vello_hip_ctx *ctx, int enabled);
/* vello_encoding::BumpEstimator (vello_encoding/src/estimate.rs:54-190) applied to the packed scene: conservative
 * pool sizes for this scene at this target size, computed on the host without touching the GPU.  Lines and segments
 * follow the reference's counting rules (Wang's formula for curves, sqrt(2)-inflated tile crossings, arc counts of
 * round joins / caps); tiles, bin entries and PTCL words -- TODO upstream (estimate.rs:14-16) -- come from the paths'
 * control-point bounding boxes.  blend_spill is not estimated (0).  With vello_hip_set_auto_grow the blocking
 * vello_hip_render calls this itself when the scene is large against the current pools. */
/* How many rounds the last blocking vello_hip_render took (1 unless robust mode had to grow pools and re-run). */
uint32_t vello_hip_last_render_attempts(vello_hip_ctx *ctx);
/* Launches in which the stages of a small scene shared a kernel (VELLO_HIP_DEBUG_NO_FUSION), counted since the context was
 * created: lets a test see that the scene it renders took that path. */
uint64_t vello_hip_fused_launches(vello_hip_ctx *ctx);
/* Scene buffers allocated since the context was created (vello_hip_upload_scene's shared one and the private ones of
 * vello_hip_render_frame's lanes): lets a test see that frames whose scenes fit the buffers they have allocate nothing -- a
 * re-allocation frees device memory, which waits for every frame in flight. */
uint64_t vello_hip_scene_allocations(vello_hip_ctx *ctx);
/* Scene indexes built since the context was created.  vello_hip_upload_scene (and vello_hip_upload_fragments through it) builds one
 * for a scene too large for the small-scene launches (VELLO_HIP_SHAPE_FRONT_MAX_TAGS / _FRONT_MAX_DRAW_OBJECTS): the pathtag scan's
 * output and verdict, the path boxes as the scan leaves them, and the scene's segment tags sorted into fills, stroked curves and
 * stroked lines -- everything a frame of the resident scene would otherwise compute again from the same bytes, none of it a function
 * of a transform.  Frames of vello_hip_render_resident read it in place of the scan and of the sorting half of flatten's light
 * pass; every buffer a stage leaves is what it leaves without the index (tag monoids and path boxes bit for bit, the line soup as a
 * multiset), and VELLO_HIP_BUF_TAG_MONOIDS shows the index's array.  The next upload drops it; so does a vello_hip_write_buffer to
 * VELLO_HIP_BUF_SCENE of the resident scene, after which frames take the per-frame path until the next upload.  Private scenes
 * (vello_hip_render_frame), composed frames and the retained list are not indexed.  Lets a test see that frames build none. */
uint64_t vello_hip_scene_index_builds(vello_hip_ctx *ctx);
int vello_hip_estimate_capacities(const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                                  const vello_hip_render_params *params, vello_hip_capacities *out);

/* Viewport culling (default 0: every buffer and counter is the reference's).  With it on, flatten leaves out of the line soup
 * every line that lies wholly off the target on its top, bottom or right side.  With wt = ceil(width / 16), ht = ceil(height / 16)
 * and S = 0.0625f, a line (p0, p1) is left out iff, in f32,
 *     p0.y * S >= ht && p1.y * S >= ht,  or  p0.y * S <= 0 && p1.y * S <= 0,  or  p0.x * S >= wt && p1.x * S >= wt
 * (a NaN coordinate fails its comparisons: the line stays).  Lines wholly LEFT of the target stay: they bump the backdrops of
 * their rows.  path_count drops exactly these lines before it touches a backdrop or a count (path_count.wgsl:103-164: a path's
 * tile box is its draw box cut to the target), so
 *   1. path boxes -- hence draw boxes, clip boxes, bin lists, Path records, bump.binning, bump.tile -- do not change: a path's
 *      box is still the union of ALL its lines;
 *   2. the soup holds the lines the rule keeps and bump.lines counts them.  Exception: a curve piece too large for a workgroup's
 *      staging area has its slots reserved before its lines exist and keeps all of them (then: kept lines <= soup <= all lines,
 *      bump.lines = the soup's size);
 *   3. everything behind the soup is unchanged: backdrops, segment counts, bump.seg_counts, bump.segments, the PTCL, the
 *      segments, the image (seg_counts[].line_ix indexes the smaller soup);
 *   4. the line pool overflows (VELLO_HIP_E_CAPACITY, auto-grow's demand) on the smaller count: a view of a large scene fits a
 *      pool that the whole scene overflows.
 * vello_hip_estimate_capacities is unchanged (still an upper bound).  Applies to frames enqueued after the call, on every entry
 * point that renders (render, render_frame, render_resident, run_stages with FLATTEN in the range) and on all in-flight buffer
 * sets; frames already enqueued keep the setting they were enqueued with.  Worth switching on when a good part of the scene
 * lies off the target (a zoomed or panned view); on a scene that is all on the target flatten pays the test for nothing.
 * VELLO_HIP_E_INVALID for a null context. */
int vello_hip_set_viewport_cull(vello_hip_ctx *ctx, int enabled);

/* View transform for the frames that follow (default: none).  `view` is a vello_encoding::Transform, [m0 m1 m2 m3 t0 t1]: the
 * matrix [[m0 m2] [m1 m3]] and the translation (t0, t1).  A frame enqueued while a view V is set is rendered as if every entry T of
 * the scene's transform stream -- the words [transform_base, style_base) of the packed scene, n_xf = (style_base - transform_base) / 6
 * entries -- had been replaced by V.T, which is what Scene::append(scene, Some(V)) does to a scene on the host, without encoding,
 * packing or uploading anything.  V.T is computed as Transform::mul computes it (vello_encoding/src/math.rs:51-73): in f32, every
 * product and every sum rounded on its own, in this operand order and association:
 *     m0' = V.m0*T.m0 + V.m2*T.m1        m1' = V.m1*T.m0 + V.m3*T.m1
 *     m2' = V.m0*T.m2 + V.m2*T.m3        m3' = V.m1*T.m2 + V.m3*T.m3
 *     t0' = (V.m0*T.t0 + V.m2*T.t1) + V.t0
 *     t1' = (V.m1*T.t0 + V.m3*T.t1) + V.t1
 *   1. No other word of the scene changes.  A path encoded before any transform (trans_ix = 0 - 1: the zero-width stroke clip a
 *      scene may begin with, scene.rs:179-183) reads the six words BELOW the stream; it keeps reading exactly those words,
 *      uncomposed -- as it would after a host-side replacement of the stream.
 *   2. The resident scene is never modified: vello_hip_read_buffer(VELLO_HIP_BUF_SCENE) returns the uploaded bytes whatever views
 *      have been rendered, and VELLO_HIP_BUF_CONFIG holds the scene's own layout.  NULL restores frames without a view bit for
 *      bit, in every buffer and counter.
 *   3. A non-null view always composes, the identity included (on a scene of finite transforms the result equals the off state).
 *   4. VELLO_HIP_E_INVALID, and nothing changes, for a null context or a view with a NaN or infinite entry.  Singular and
 *      mirroring views are legal: what they show is what the composed scene shows.
 *   5. Applies to frames enqueued after the call on every entry point that renders (render, render_frame, render_resident, and
 *      run_stages when the range holds FLATTEN or DRAW_SCAN) and on all in-flight buffer sets; frames already enqueued keep the
 *      view they were enqueued with: four frames in flight may show four views of one resident scene.
 *   6. Composes with vello_hip_set_viewport_cull: the rule is applied to the lines of the viewed scene.
 *   7. With vello_hip_set_auto_grow the blocking vello_hip_render sizes the pools with vello_hip_estimate_capacities_view and the
 *      context's view.
 * The composed words are written by one small kernel (k_view_transforms, a lane per entry) at the head of every frame that has a
 * view, into a per-frame copy behind the scene's bytes; nothing crosses PCIe.  Scenes whose packed bytes and copies together
 * exceed 2^32 words are refused with VELLO_HIP_E_INVALID when a frame with a view is enqueued. */
int vello_hip_set_view_transform(vello_hip_ctx *ctx, const float view[6] /* nullable: off (default) */);
/* Damage rectangle for the frames that follow (default: none -- every frame draws its whole target).  `rect` is x0 y0 x1 y1 in
 * pixels, half open: a frame enqueued while one is set renders only the tiles the rectangle touches and writes only its pixels --
 * partial redraw for a caller that knows what changed (a highlight, a moved handle, a caret).  The engine does not compute damage.
 *   1. THE RECTANGLE.  R = rect cut to [0, width) x [0, height), computed per frame against that frame's target size.  x0 > x1 or
 *      y0 > y1 is VELLO_HIP_E_INVALID (vello_hip_last_error names the rule) and nothing changes: the setting, the rotation, every
 *      frame in flight.  An EMPTY R is legal (zero area, or wholly off the target): such a frame writes no byte of the target
 *      and launches neither k_coarse, k_path_tiling nor k_fine.  NULL restores whole frames bit for bit, in every buffer and
 *      counter; a rectangle that covers the whole target gives the off state's image, buffers and counters.
 *   2. THE TARGET.  The engine writes exactly the bytes [y * out_stride + x0 * 4, y * out_stride + x1 * 4) of the rows
 *      y0 <= y < y1 of R, and no other byte (this extends THE TARGET at vello_hip_render_resident: everything beside R keeps its
 *      contents like row padding does).  Every pixel of R holds the value the whole frame would have written there -- MSAA8 /
 *      MSAA16 bit for bit, area AA within the order of a tile's segment atomics, as for any two whole frames.  The blocking
 *      vello_hip_render with a host target copies R's rows and columns only.  With out_device == NULL the frame writes R into its
 *      lane's internal target; the internal targets of different lanes (vello_hip_set_frames_in_flight) are DIFFERENT surfaces,
 *      so partial frames want a caller's target or one frame in flight.
 *   3. EVERYTHING AHEAD OF COARSE IS THE WHOLE FRAME'S: tag monoids, path boxes, the line soup, draw monoids, info, clip boxes,
 *      bin lists, Path records, tile backdrops, SegmentCount records, and bump.lines / binning / tile / seg_counts.  (The soup
 *      and the backdrops of tiles left of R feed R's backdrops.)  vello_hip_pick and vello_hip_pick_rect after a damaged frame
 *      therefore answer as after the whole frame.  k_coarse_prep runs whole.
 *   4. BEHIND IT, with W = the tiles that intersect R: a tile outside W gets nothing -- no PTCL word, no segment slice, no
 *      blend-spill allocation, no bucket entry, no slice item; a tile inside W gets the command list, the segments and the blend
 *      offset the whole frame gives it.  bump.segments, bump.ptcl and bump.blend count W's tiles only, so the segment, PTCL and
 *      blend pools overflow (VELLO_HIP_E_CAPACITY, auto-grow's demand) on the smaller counts: a window of a frame fits pools the
 *      whole frame overflows.  vello_hip_estimate_capacities is unchanged (still an upper bound).  VELLO_HIP_BUF_PTCL: the blocks
 *      of tiles outside W hold stale words of earlier frames (word 0 of the buffer: tile 0's blend offset, or 0 when tile 0 is
 *      outside W).
 *   5. Composes with viewport culling, a view, instances, retained poses and paints, a morph, VELLO_HIP_DEBUG_NO_CULL, forced
 *      slices and frames in flight; none of them learns about it.
 *   6. Applies to frames enqueued after the call on every entry point that renders (render, render_frame, render_resident,
 *      render_resident_morphed, render_instances[_painted], render_retained[_painted], and run_stages when the range holds COARSE,
 *      PATH_TILING or FINE) and on all in-flight buffer sets; frames already enqueued keep the rectangle they were enqueued with:
 *      four frames in flight may carry four rectangles.
 * VELLO_HIP_E_INVALID for a null context. */
int vello_hip_set_damage_rect(vello_hip_ctx *ctx, const uint32_t rect[4] /* x0 y0 x1 y1, pixels, half-open; nullable: off (default) */);
/* vello_hip_estimate_capacities with V composed, by the same formula, into every transform the estimator reads; equal to it for
 * view == NULL.  VELLO_HIP_E_INVALID for a view with a NaN or infinite entry. */
int vello_hip_estimate_capacities_view(const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                                       const vello_hip_render_params *params, const float view[6] /* nullable */,
                                       vello_hip_capacities *out);
/* Stroke scale for the frames that follow (default: none): non-scaling strokes under a view.  `stroke` is (s, m): a frame enqueued
 * while it is set is rendered as if every stroke width of the scene's style stream had been multiplied by s and raised to at
 * least m -- what a host does by patching the widths and packing and uploading the scene again, without any of the three.  A
 * caller whose view zooms by z passes s = 1 / z for strokes that keep their width on screen (SVG's vector-effect:
 * non-scaling-stroke) and m = hairline / z for strokes that never fall below a hairline.
 *   1. THE FRAME'S STYLE WORDS.  The style stream is the entries e < n_styles = (scene_words - style_base) / 2; entry e is
 *      flags = scene[style_base + 2e] and w = scene[style_base + 2e + 1] as f32.  The flags word is copied verbatim.  The width word
 *      becomes w' = (x < m ? m : x) with x = fl(w * s) -- one f32 multiply, IEEE-rounded, and one compare -- iff
 *      (flags & STYLE_FLAGS_STYLE) != 0 and w > 0.0f.  Every other width word is a bit copy: fills, and strokes of width 0, of
 *      negative width or of NaN width (payloads and signed zeros arrive as they were).  The zero-width stroke that encodes an empty
 *      clip (scene.rs:179-183) therefore stays empty whatever m is.  s and m are in the path's own units, ahead of its transform,
 *      as the width is.
 *   2. WHAT SUCH A FRAME IS.  Bit for bit in every buffer and counter, the frame the same entry point would enqueue had the scene
 *      carried these words in its style stream (the line soup and the segment slices as multisets, as everywhere): under a view,
 *      viewport culling, a damage rectangle and a morph, with frames in flight, with and without the scene index, in the
 *      small-scene launches and without them, and with every kernel choice of the debug flags.
 *   3. STYLE INDEX -1.  A segment met before any STYLE marker keeps reading the two words BELOW the scene's own style stream,
 *      unscaled -- the rule the view has for transform -1.
 *   4. The scene is never modified: VELLO_HIP_BUF_SCENE shows the uploaded, composed or retained bytes, VELLO_HIP_BUF_CONFIG the
 *      scene's own layout.  The scene index stays valid: vello_hip_scene_index_builds does not move.
 *   5. Applies to frames enqueued after the call on every entry point that renders (render, render_frame, render_resident,
 *      render_resident_morphed, render_instances[_painted], render_retained[_painted], and run_stages when the range holds
 *      FLATTEN -- otherwise run_stages goes on from the lane's buffers as they are) and on all in-flight buffer sets; frames
 *      already enqueued keep the setting they were enqueued with: four frames in flight may carry four scales.  For composed and
 *      retained frames the composed or retained style stream is read on the device; the host never sees those bytes.
 *   6. A non-null setting always runs the kernel; (1, 0) gives the off state's buffers and counters on a scene of finite widths.
 *      NULL restores the off state bit for bit: frames without the setting run exactly the launches they run without this call.
 *   7. VELLO_HIP_E_INVALID, with vello_hip_last_error naming the rule and nothing changed (the setting, the rotation, the frames in
 *      flight), for a null context (no message: there is no context to hold one), for s that is NaN, infinite or <= 0, and for m
 *      that is NaN, infinite or < 0.  A scene whose packed bytes and copies together reach 2^32 words is refused with
 *      VELLO_HIP_E_INVALID when a frame with the setting is enqueued, the rotation left where it was.
 *   8. vello_hip_pick and vello_hip_pick_rect answer against the scaled strokes: they read the frame's soup and path boxes.
 *   9. With vello_hip_set_auto_grow the blocking vello_hip_render sizes the pools with vello_hip_estimate_capacities_styled and the
 *      context's setting.
 * The frame's style words are written by one small kernel (k_style_widths, a lane per entry) at the head of every frame that has
 * the setting, into a per-frame copy behind the scene's bytes; nothing crosses PCIe.
 * OUT OF SCOPE: per-style widths or factors from host or device memory (the same copy, another source); changing caps, joins,
 * miter limits or fill versus stroke (the scene index depends on the flags); a width in screen space for scenes whose transforms
 * differ in scale (s and m are applied ahead of each path's own transform). */
int vello_hip_set_stroke_scale(vello_hip_ctx *ctx, const float stroke[2] /* scale, min_width; nullable: off (default) */);
/* vello_hip_estimate_capacities_view with rule 1 of vello_hip_set_stroke_scale applied to every width the estimator reads; equal to
 * it for stroke == NULL.  VELLO_HIP_E_INVALID for a `stroke` that vello_hip_set_stroke_scale refuses. */
int vello_hip_estimate_capacities_styled(const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                                         const vello_hip_render_params *params, const float view[6] /* nullable */,
                                         const float stroke[2] /* nullable */, vello_hip_capacities *out);
/* Base image for the frames that follow (default: none -- every pixel of a frame starts from params.base_color).  A frame enqueued
 * while one is set is drawn OVER pixels that already lie in device memory: a cached raster under a selection overlay, a raster layer
 * under vector content, a decoded video frame under annotations -- without a second compositing pass and without an image draw in
 * the scene.  A setting like the view, the damage rectangle and the stroke scale: frames already enqueued keep what they were
 * enqueued with, so four frames in flight may lie over four images.
 *   1. THE WORDS.  One premultiplied RGBA8 word per pixel, R in the low byte: params.base_color's format, and any word is accepted
 *      as any base_color is (a channel above its alpha included).  Pixel (x, y) of a frame of width x height is the word at
 *      image_device + y * stride + 4 * x (stride 0: width * 4 of the frame).  The frame is, pixel for pixel, the frame the same entry
 *      point would enqueue with base_color equal to that pixel's word; params.base_color is ignored.  MSAA8 / MSAA16 bit for bit,
 *      area AA within the order of a tile's segment atomics, as for any two frames.  A uniform image equal to base_color gives
 *      the off state's target, buffers and counters.
 *   2. NOTHING AHEAD OF FINE LEARNS ABOUT IT.  Every buffer and counter of the frame is the off state's -- VELLO_HIP_BUF_PTCL,
 *      segments, bump counters, pool overflow, vello_hip_pick and vello_hip_pick_rect -- and vello_hip_estimate_capacities* is
 *      unchanged.  Coarse's occlusion culling never looked at the base.
 *   3. WHAT IS READ.  Exactly the words of the pixels the frame writes: the target's pixels, or R's under a damage rectangle
 *      (vello_hip_set_damage_rect); no byte outside [y * stride, y * stride + width * 4) of a row y < height, nothing for an empty
 *      R.  Four pixels at a time where they all lie inside and their address is 16-byte aligned, word by word otherwise, as the
 *      target is stored.  The image may be a sub-rectangle of a larger surface.
 *   4. IN PLACE.  The image may BE the target: the same address and the same effective stride as out_device.  The frame then draws
 *      over what the target holds -- a load in place of a clear; with a damage rectangle only R is read and written.  (Each pixel
 *      is read and then written by the same lane of the one wave that composites its tile.)  An image whose bytes
 *      [image, image + (height - 1) * stride + width * 4) overlap the target's in any other way is refused when the frame is
 *      enqueued.  The engine's output is UN-premultiplied and the base is premultiplied: the same word for opaque pixels only.
 *      Premultiplying a translucent previous output is the caller's business.
 *   5. REFUSALS, each VELLO_HIP_E_INVALID with vello_hip_last_error naming the rule and nothing changed -- the setting, the rotation,
 *      the frames in flight.  At the call: a null context; an address or a stride that is not a multiple of 4; a stride >= 2^32;
 *      src_stream with a NULL image.  When a frame is enqueued (nothing is enqueued, the rotation stays where it was): a non-zero
 *      stride below width * 4; (GPU builds) bytes [image, image + (height - 1) * stride + width * 4) that do not lie in one
 *      allocation of device memory of the context's device, tested as vello_hip_copy_images_device tests its sources (once per
 *      setting and extent, not per frame); the partial overlap of rule 4.
 *   6. ORDERING.  With src_stream (a hipStream_t) an event is recorded on it during the call; every frame enqueued under the
 *      setting waits for that event no later than its k_fine, and src_stream then waits for that frame's fine: work enqueued on
 *      it afterwards may overwrite the image.  Nothing waits on the host.  src_stream must stay valid while the setting stands.
 *      Without src_stream the caller keeps the image valid and unchanged until the frames have finished.  A new call, NULL
 *      included, replaces the event; vello_hip_destroy releases it.
 *   7. Applies to frames enqueued after the call on every entry point that renders (render, render_frame, render_resident,
 *      render_resident_morphed, render_instances[_painted], render_retained[_painted], and run_stages when the range holds FINE),
 *      with out_device == NULL (the image lies under the lane's internal target) and with the blocking vello_hip_render's host
 *      target (the copy-out is unchanged).  Composes with the view, viewport culling, damage rectangles, the stroke scale, morphs,
 *      forced slices and frames in flight.  An instance frame with n == 0 shows the image itself, as un-premultiplied words; a
 *      failed frame leaves the target untouched as before; NULL restores the off state bit for bit -- frames without the setting
 *      run exactly the launches they ran.
 *   8. OUT OF SCOPE: straight-alpha or BGRA sources; images in host memory; scaling or offsetting the image against the target; a
 *      base image per lane's internal target. */
int vello_hip_set_base_image(vello_hip_ctx *ctx, const void *image_device /* nullable: off (default) */,
                             size_t stride /* bytes per row; 0 = width * 4 of the frame */, void *src_stream /* nullable hipStream_t */);

/* Scene instances: the resident scene as a library of fragments, a frame as a list of (fragment, transform) pairs -- what a host
 * builds with Scene::append(&fragment, Some(transform)) per pair (vello_encoding/src/encoding.rs:95-152), composed on the GPU. */
/* (The two structs below are declared tag first, typedef after -- to C the same as `typedef struct X {...} X;` -- because the
 * struct parser of tests/test_shim.py, which reads every `typedef struct ... {` of this header, has no rule for array fields;
 * tests/test_scene_instances_emu.py holds these two to their ctypes and Rust mirrors.) */
/* Half-open ranges [begin, end) into the six streams of the resident scene. */
struct vello_hip_fragment {
    uint32_t path_tags[2];   /* tags (bytes) from the start of the tag stream          */
    uint32_t path_data[2];   /* words from path_data_base                               */
    uint32_t draws[2];       /* draw objects (= paths): index the draw tags             */
    uint32_t draw_data[2];   /* words from draw_data_base                               */
    uint32_t transforms[2];  /* entries of 6 words                                      */
    uint32_t styles[2];      /* entries of 2 words                                      */
};
typedef struct vello_hip_fragment vello_hip_fragment;
/* A fragment placed by `transform`, a vello_encoding::Transform [m0 m1 m2 m3 t0 t1] as vello_hip_set_view_transform takes it. */
struct vello_hip_instance {
    uint32_t fragment;
    float transform[6];
};
typedef struct vello_hip_instance vello_hip_instance;

/* vello_hip_upload_scene plus a table of `n_frags` fragments of that scene.  The scene is an ordinary resident scene
 * (vello_hip_render_resident shows it whole); a later vello_hip_upload_scene -- vello_hip_render's included -- drops the table.
 * Every fragment is checked against the host bytes; VELLO_HIP_E_INVALID (vello_hip_last_error names the fragment), with NOTHING
 * left resident, unless for each one
 *   - every range is ordered and lies inside its stream;
 *   - `draws` is as long as the tag range has PATH markers, `transforms` / `styles` as it has TRANSFORM / STYLE markers;
 *   - `draw_data` is as long as the fragment's draw tags ask for;
 *   - its clips are balanced, no prefix of its draw tags holding more END_CLIP than BEGIN_CLIP;
 *   - a TRANSFORM and a STYLE marker precede its first segment or PATH tag (a Scene that begins with a fill, a stroke or a
 *     filled layer satisfies this): no fragment reads transform -1 or a neighbour's style.
 * Whether the path data matches the tags is, as for any scene, the pathtag scan's to find (VELLO_HIP_E_INVALID at sync). */
int vello_hip_upload_fragments(vello_hip_ctx *ctx, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                               const uint32_t *ramps, uint32_t n_ramps, const vello_hip_fragment *frags, uint32_t n_frags);
/* The composed scene of instances i = 0 .. n-1, F(i) the fragment of instance i and V_i its transform:
 *   tags       the concatenation of the F(i)'s tag bytes, zero-padded to a multiple of 1024 bytes (none for no tags);
 *   then, in this order, the concatenations of the F(i)'s path-data words, draw tags, draw-data words, transform entries
 *   and style entries.
 *   1. Every transform entry T of instance i becomes V_i.T, by the formula and in the arithmetic of
 *      vello_hip_set_view_transform: f32, every product and every sum rounded on its own.  No other word changes.
 *   2. Layout: path_tag_base = 0, the five other bases are the running sums; n_paths = n_draw_objects = the sum of the `draws`
 *      lengths, n_clips = the fragments' clip tags, bin_data_start = their info words; scene_len = 4 * (style_base + 2 * styles).
 *   3. Gradient ramps and the image atlas are the library's (the draw data carries the library's ramp ids and atlas
 *      coordinates verbatim).
 * vello_hip_instances_layout returns exactly this layout and length on the host, without touching the GPU.
 * VELLO_HIP_E_INVALID for both entry points -- vello_hip_render_instances then enqueues nothing and leaves the rotation of the
 * in-flight buffer sets where it was -- when there is no fragment table, `inst` is NULL with n > 0, a fragment index is out of
 * range, a transform has a NaN or infinite entry, or the composed scene has 2^32 words or more or a count that leaves u32. */
int vello_hip_instances_layout(vello_hip_ctx *ctx, const vello_hip_instance *inst, uint32_t n, vello_hip_layout *layout_out,
                               size_t *scene_len_out);
/* vello_hip_render_frame with the frame's scene composed on the GPU: takes the next in-flight buffer set (waiting for that set's
 * previous frame only), copies a table of 52 bytes per instance through pinned memory, has ONE kernel (k_compose_scene) write the
 * composed scene into the set's private scene slot -- where vello_hip_render_frame copies host bytes -- enqueues every stage and
 * returns without waiting.  `inst` may be reused when the call returns.
 *   1. n == 0 renders the base colour.
 *   2. Composes with vello_hip_set_view_transform (applied on top: a transform entry ends up as View.(V_i.T)) and with
 *      vello_hip_set_viewport_cull, like a vello_hip_render_frame scene.
 *   3. Afterwards VELLO_HIP_BUF_SCENE / VELLO_HIP_BUF_CONFIG show the composed bytes and layout of the last frame and
 *      vello_hip_run_stages acts on them, as after vello_hip_render_frame.  The library's bytes are never modified.
 *   4. A pool overflow is reported as for vello_hip_render_frame: VELLO_HIP_E_CAPACITY at vello_hip_sync, the counters through
 *      vello_hip_get_bump; vello_hip_grow_pools and a second call render the frame again.
 * Out of scope: pool estimation for instance lists (vello_hip_estimate_capacities needs host bytes; with vello_hip_set_auto_grow
 * only the PTCL / info-word minimum of the target is sized), ramps or atlases per fragment, and unbalanced fragments. */
int vello_hip_render_instances(vello_hip_ctx *ctx, const vello_hip_instance *inst, uint32_t n, const vello_hip_render_params *params,
                               void *out_device, size_t out_stride);

/* Per-instance paint, parallel to the instance list: instance i of a fragment drawn in a solid colour of its own -- a glyph run's
 * brush (Encoding::encode_brush, vello_encoding/src/encoding.rs:280-290), a tinted or highlighted symbol, a selection colour, a
 * fade -- without a copy of the outline per colour in the library. */
enum { VELLO_HIP_PAINT_KEEP = 0, VELLO_HIP_PAINT_SOLID = 1 };
typedef struct vello_hip_paint {
    uint32_t flags, rgba;   /* rgba: premultiplied RGBA8, R in the low byte -- a DrawColor word, as base_color */
} vello_hip_paint;
/* vello_hip_render_instances with `paints[i]` applied to instance i.
 * The colour words of a fragment: walk its draw tags draws[0] .. draws[1] in order with a running offset d = 0 into its draw_data
 * range; a tag t advances d by (t >> 2) & 7; word d of a tag equal to DRAWTAG_FILL_COLOR (0x44) or DRAWTAG_BLURRED_ROUNDED_RECT
 * (0x2d4) is a colour word -- both hold a DrawColor first (vello_encoding/src/draw.rs:70-74, :175-186).  Nothing else is: not a
 * gradient's index and points, not an image's words, not the four floats of a blurred rect, not BEGIN_CLIP's blend and alpha words.
 * The rule is per fragment and relative to its own draw_data begin (fragments may overlap in the library).
 * The composed scene is the one vello_hip_render_instances documents, with one more rule:
 *   1b. Every colour word of instance i with paints[i].flags == VELLO_HIP_PAINT_SOLID becomes paints[i].rgba.  No other word
 *       changes; the layout and length are those of vello_hip_instances_layout, whatever the paints.
 *   - paints == NULL is vello_hip_render_instances (which is this call with NULL): the same frame, bit for bit in every buffer and
 *     counter, from the same kernel and the same table of 52 bytes per instance.  A paint list adds 8 bytes per instance to it.
 *   - A paint on an instance whose fragment has no colour word (gradient, image, clip-only, empty) and VELLO_HIP_PAINT_KEEP with
 *     any rgba are legal and change nothing.  Any rgba is accepted, as any base_color is.
 *   - VELLO_HIP_E_INVALID, with vello_hip_last_error naming the instance, for a flags value other than 0 or 1 -- like every refusal
 *     of vello_hip_render_instances, all of which apply: nothing is enqueued, the rotation and VELLO_HIP_BUF_SCENE stay as they
 *     were.  Also for a paint list on a library whose fragments' draw_data ranges add up to 2^32 words or more (no masks are kept
 *     for it; unpainted frames of such a library are served as before).
 *   - Paints belong to their frame: frames in flight may show one instance list under different paints, an unpainted frame that
 *     follows a painted one on the same buffer set shows the library's colours, the library's bytes are never modified.  `paints`
 *     may be reused when the call returns.
 *   - Afterwards VELLO_HIP_BUF_SCENE / VELLO_HIP_BUF_CONFIG show the painted composed bytes and layout and vello_hip_run_stages
 *     acts on them.  Composes with the view transform and viewport culling like any instance frame.  Coarse reads the composed
 *     colours: an instance painted opaque may occlude what lies under it, the same instance painted translucent may not.
 * Out of scope: alpha modulation of the library's colour (the host multiplies before it quantises, encoding.rs:280-290, so a
 * stored premultiplied word cannot reproduce it: the caller passes the finished word); gradient, image and layer-alpha overrides;
 * pool estimation for instance lists, which stays where vello_hip_render_instances left it. */
int vello_hip_render_instances_painted(vello_hip_ctx *ctx, const vello_hip_instance *inst, const vello_hip_paint *paints /* nullable */,
                                       uint32_t n, const vello_hip_render_params *params, void *out_device, size_t out_stride);

/* Retained instance lists: the list that the previous frame drew, re-posed.  The reference seam is still
 * Scene::append(&fragment, Some(transform)) per pair; this is the same composed scene with the appends hoisted out of the frame
 * loop.  vello_hip_retain_instances composes `inst` (with `paints`, nullable) ONCE into a retained scene owned by the context;
 * vello_hip_render_retained enqueues one frame of it under this frame's poses -- one 6-float transform per instance, which take
 * the place of inst[i].transform -- and returns without waiting.
 *   1. WHAT IS RETAINED.  The scene vello_hip_render_instances_painted(inst, paints, n) documents -- layout, length, padding, slack
 *      and rule 1b's colour words -- except that every transform entry is the library's T VERBATIM (copied, not multiplied by an
 *      identity: 1 * -0 + 0 * x is +0).  It lives in a slot of its own beside the resident library and the buffer sets' private
 *      slots; ramps and atlas are the library's.  Resident with it: for every transform entry the instance that owns it, and the
 *      rest poses inst[i].transform.  Every refusal of vello_hip_render_instances_painted applies, and a list of more than 2^32 / 6
 *      instances is refused as well: VELLO_HIP_E_INVALID with nothing retained and a previously retained list left as it was.  The
 *      call waits for the frames in flight, as an upload does; a second call replaces the list.  vello_hip_upload_scene,
 *      vello_hip_render's upload and vello_hip_upload_fragments drop the list with the fragment table;
 *      vello_hip_release_retained frees it (VELLO_HIP_OK when there is none).
 *   2. A RETAINED FRAME under poses X is, bit for bit in every buffer and counter, the frame
 *      vello_hip_render_instances_painted((fragment_i, X_i), paints, n) enqueues -- view transform and viewport culling included:
 *      a transform entry ends up as View.(X_i.T), each product rounded to six f32 words by vello_hip_set_view_transform's formula
 *      before the next is formed.  ONE kernel (k_instance_transforms, a lane per transform entry) writes the frame's transform
 *      words into a per-buffer-set copy behind the retained bytes; nothing is re-encoded and no other word is rewritten.  The one
 *      exception is VELLO_HIP_BUF_SCENE, which shows the retained bytes of rule 1 (the library's T's), as a viewed scene shows
 *      its own bytes; VELLO_HIP_BUF_CONFIG holds the composed layout.  vello_hip_run_stages after a retained frame acts on the
 *      retained scene and goes on from that frame's composed transform words as they are (the poses are not read again, and a
 *      view set since is not applied); on a buffer set that holds none of this list it uses the rest poses.
 *   3. WHERE THE POSES COME FROM.  transforms == NULL: the rest poses -- a static list re-rendered, or viewed under a moving
 *      vello_hip_set_view_transform, with no per-instance work on the host.  Host memory (transforms_is_device == 0): n x 6 floats,
 *      copied through pinned memory during the call (24 bytes per instance; `transforms` may be reused on return); a NaN or
 *      infinite entry is VELLO_HIP_E_INVALID with vello_hip_last_error naming the instance; src_stream must be NULL.  Device
 *      memory (transforms_is_device != 0): 4-byte aligned, n x 6 floats in one allocation on the context's device (anything else is
 *      refused in GPU builds, as vello_hip_copy_images_device refuses it).  The host does no per-instance work and does not
 *      read the poses.  With `src_stream` (a hipStream_t) the frame waits for what has been enqueued on it so far, and src_stream
 *      then waits for the kernel that reads the poses: work enqueued there afterwards may overwrite them.  Nothing waits on the
 *      host.  Without src_stream the caller keeps the poses valid and unchanged until the frame has finished.  A device pose with
 *      a NaN or infinite entry is found by the kernel: the frame is discarded like one whose tag stream contradicts its scene --
 *      the target untouched, VELLO_HIP_E_INVALID at vello_hip_sync -- and the next frame is unaffected.
 *   4. Poses belong to their frame: four frames in flight may show four pose sets of one retained list in four targets.
 *      Retained frames rotate over the in-flight buffer sets with every other kind of frame and may alternate with
 *      vello_hip_render_resident, _render_frame and _render_instances frames.  No frame modifies the library's bytes or the
 *      retained bytes.  THE TARGET (at vello_hip_render_resident) applies.  A pool overflow is reported as for
 *      vello_hip_render_instances: VELLO_HIP_E_CAPACITY at vello_hip_sync, then vello_hip_grow_pools and a second call.  A
 *      refused frame (VELLO_HIP_E_INVALID: no retained list, a pose or a pose source as rule 3 refuses it, a target or render
 *      parameters that are refused) enqueues nothing and leaves the rotation where it was.
 *   5. Out of scope: per-frame changes of membership or order (retain again); pool estimation for instance lists; more than one
 *      retained list per context.  Per-frame paints are vello_hip_render_retained_painted, below. */
int vello_hip_retain_instances(vello_hip_ctx *ctx, const vello_hip_instance *inst, const vello_hip_paint *paints /* nullable */, uint32_t n);
int vello_hip_render_retained(vello_hip_ctx *ctx, const float *transforms /* n x 6, nullable */, int transforms_is_device,
                              void *src_stream /* nullable hipStream_t */, const vello_hip_render_params *params, void *out_device,
                              size_t out_stride);
/* vello_hip_render_retained with this frame's paints: a highlight on what vello_hip_pick found, a selection colour, a fade, a heat
 * map whose colours a GPU op computes each frame -- without retaining the list again.  The reference seam is the one of
 * vello_hip_render_instances_painted (Encoding::encode_brush per appended scene).  vello_hip_render_retained is this call with
 * paints == NULL: the same frame, bit for bit, from the same kernels (no new kernel is launched), its draw data read from the
 * retained bytes.
 *   1. WHAT A PAINTED RETAINED FRAME IS.  Let R be the paints the list was retained with (KEEP everywhere if none), P this frame's
 *      paints, X this frame's poses as rule 3 of vello_hip_render_retained defines them, and Q_i = P_i where P_i.flags ==
 *      VELLO_HIP_PAINT_SOLID, else R_i.  The frame is vello_hip_render_instances_painted((fragment_i, X_i), Q, n), bit for bit in
 *      every buffer and counter, view transform and viewport culling included.  VELLO_HIP_PAINT_KEEP therefore keeps what the
 *      list was retained with, its retained paint included: a highlight is SOLID on one instance and KEEP on the rest.  A SOLID
 *      paint on an instance whose fragment has no colour word changes nothing.  Colour words are the ones the rule at
 *      vello_hip_render_instances_painted defines (DRAWTAG_FILL_COLOR, DRAWTAG_BLURRED_ROUNDED_RECT, per fragment), through the
 *      masks kept since vello_hip_upload_fragments; a library that keeps no masks refuses a paint list, as the other painted
 *      entry points do.
 *   2. HOW THE FRAME'S COLOURS ARE MADE.  ONE kernel (k_instance_paints, a lane per draw-data word) writes the frame's draw-data
 *      words into a per-buffer-set copy of the draw-data stream behind the retained bytes, at the head of the frame beside
 *      k_instance_transforms; nothing is re-encoded and no other word is rewritten.  The kernels that read draw data (the draw
 *      stage and coarse's preparation, in every launch form that holds them) are handed the copy in the stream's place, so
 *      coarse's occlusion culling judges the frame's colours: an instance painted opaque this frame may occlude, painted
 *      translucent it may not.  VELLO_HIP_BUF_SCENE shows the retained bytes as before -- the library's transforms and the
 *      retained colours R, not P -- and VELLO_HIP_BUF_CONFIG the composed layout with the scene's own draw_data_base.  The copy
 *      must be reachable with the scene pointer and a u32 word offset: a list whose retained bytes and copies together reach 2^32
 *      words is refused with VELLO_HIP_E_INVALID when a painted frame is enqueued; its unpainted frames are served as before.
 *   3. WHERE THE PAINTS COME FROM.  paints == NULL: an unpainted frame.  Host memory (paints_is_device == 0): n x 8 bytes, copied
 *      through pinned memory during the call (`paints` may be reused on return); a flags value other than 0 or 1 is
 *      VELLO_HIP_E_INVALID with vello_hip_last_error naming the instance, nothing is enqueued and the rotation stays where it
 *      was.  Device memory (paints_is_device != 0): 4-byte aligned, n x 8 bytes in one allocation on the context's device
 *      (anything else is refused in GPU builds, as for device poses); the host never reads it and does no per-instance work.  A
 *      device paint with flags other than 0 or 1 is found by the kernel and the frame is discarded exactly like one with a NaN
 *      device pose: the target untouched, VELLO_HIP_E_INVALID at vello_hip_sync, the next frame unaffected.  `src_stream` is legal
 *      when at least one of the two sources is device memory: the frame waits for what has been enqueued on it so far, and
 *      src_stream then waits for the last kernel of the frame that reads the caller's memory -- work enqueued there afterwards
 *      may overwrite poses and paints.  With two host sources, or two NULL sources, src_stream must be NULL.
 *   4. PAINTS BELONG TO THEIR FRAME.  Four frames in flight may show one list under four paint sets, and four pose sets, in four
 *      targets.  An unpainted retained frame that follows a painted one on the same buffer set shows the retained colours.  The
 *      retained bytes and the library's bytes are never modified.  vello_hip_run_stages after a painted retained frame goes on from
 *      that frame's colour words and transform words as they are: neither the paints nor the poses are read again.  Every
 *      refusal of vello_hip_render_retained applies.  A steady state of painted frames allocates no scene buffer
 *      (vello_hip_scene_allocations unchanged): the room for the copies is made with the list.
 *   5. Out of scope: alpha modulation; gradient, image and layer-alpha overrides; per-frame membership or order; pool estimation
 *      for instance lists. */
int vello_hip_render_retained_painted(vello_hip_ctx *ctx, const float *transforms /* n x 6, nullable */, int transforms_is_device,
                                      const vello_hip_paint *paints /* n entries, nullable */, int paints_is_device,
                                      void *src_stream /* nullable hipStream_t */, const vello_hip_render_params *params,
                                      void *out_device, size_t out_stride);
int vello_hip_release_retained(vello_hip_ctx *ctx);

/* Per-frame path data: a frame of the resident scene whose path-data words -- the points themselves -- are a blend of two sources,
 * without re-encoding and without a byte crossing PCIe per frame: a Lottie-style shape morph (keyframes share one tag stream by
 * construction), the edges of a graph whose node positions a GPU op computes, curves a simulation leaves in a device tensor.  The
 * reference has no such input (Scene::reset and encode again); like views, poses and paints this extends the boundary, and the
 * contract is stated here.  vello_hip_render_resident is unchanged: the same kernels, the same bytes.
 *   1. SOURCES.  src_a and src_b are each a keyframe index below the n_keys of vello_hip_upload_path_keyframes,
 *      VELLO_HIP_PATH_DATA_SCENE (the resident scene's own stream) or VELLO_HIP_PATH_DATA_DEVICE (`device_words`).  A source is
 *      N = vello_hip_path_data_words(ctx) words long (draw_tag_base - path_data_base of the resident scene; 0 when none is
 *      resident).  `device_words`: N words, 4-byte aligned -- a tensor slice that starts one float in is legal -- in one
 *      allocation on the context's device (anything else is refused in GPU builds, as device poses are refused).  The host never
 *      reads it.
 *   2. THE FRAME'S WORDS W, for every word i < N.  W[i] = A[i] verbatim (a bit copy: NaN payloads and signed zeros included) when
 *      src_a == src_b or t == 0.0f (either sign); W[i] = B[i] verbatim when t == 1.0f; otherwise
 *          W[i] = fl(A[i] + fl(t * fl(B[i] - A[i])))
 *      in f32, each of the three operations rounded on its own (no contraction into an FMA).  Any finite t is legal: t outside
 *      [0, 1] extrapolates.  A NaN result has an unspecified payload.  "Points from a device tensor" is
 *      src_a == src_b == VELLO_HIP_PATH_DATA_DEVICE.
 *   3. WHAT A MORPHED FRAME IS.  Bit for bit in every buffer and counter, the frame vello_hip_render_resident would enqueue had
 *      the scene been uploaded with W in the place of its path-data stream (the line soup and the segment slices as multisets, as
 *      everywhere) -- under a view transform and viewport culling, both applied to the morphed geometry; with frames in flight;
 *      with the scene index and without it; in the small-scene launches and without them; with every kernel choice of the
 *      debug flags.  ONE kernel (k_path_blend, a streaming pass: two reads and a write per word, one read in the verbatim cases)
 *      writes W into a per-buffer-set copy of the stream behind the scene's bytes at the head of the frame; the kernels that read
 *      path data are handed the copy in the stream's place.  Nothing in the scene index depends on a point, so it stays valid and
 *      no frame builds one.  VELLO_HIP_BUF_SCENE shows the uploaded bytes, VELLO_HIP_BUF_CONFIG the scene's own layout.
 *      vello_hip_run_stages after a morphed frame goes on from that frame's words as they are (the sources are not read again).
 *      vello_hip_pick and vello_hip_pick_rect answer against the morphed geometry: they read the frame's soup.
 *   4. BLENDS NEED FLOATS.  The third case of rule 2 is refused with VELLO_HIP_E_INVALID on a scene that holds an i16 segment
 *      tag (tag & 3 != 0 and tag & 8 == 0; found once, when the scene is uploaded): its words are pairs of 16-bit integers.
 *      Verbatim frames are legal on any scene.
 *   5. KEYFRAMES.  vello_hip_upload_path_keyframes copies n_keys alternative path-data streams (host memory, n_words words each,
 *      keyframe k at words + k * n_words) into a device buffer the context owns (vello_hip_destroy frees it).  It waits for the
 *      frames in flight, as an upload does; a second call replaces the set, n_keys == 0 drops it, and every upload of a scene
 *      (vello_hip_upload_scene, vello_hip_render's own, vello_hip_upload_fragments) drops it.  VELLO_HIP_E_INVALID with nothing
 *      changed: no resident scene, n_words != vello_hip_path_data_words(ctx), words == NULL with n_keys > 0.  Keyframe contents
 *      are not validated, as a scene's own points are not.
 *   6. ORDERING.  With `src_stream` (a hipStream_t; legal only when a source is VELLO_HIP_PATH_DATA_DEVICE) the frame waits for
 *      what has been enqueued on it so far, and src_stream then waits for k_path_blend: work enqueued there afterwards may
 *      overwrite device_words -- the kernel has copied what the frame needs.  Nothing waits on the host.  Without src_stream the
 *      caller keeps device_words unchanged until the frame has finished.
 *   7. REFUSALS.  VELLO_HIP_E_INVALID, vello_hip_last_error naming the rule, nothing enqueued and the rotation of the in-flight
 *      buffer sets where it was: a null context; no resident scene; a source index >= n_keys; VELLO_HIP_PATH_DATA_DEVICE with a
 *      null, misaligned or non-device device_words; device_words or src_stream given although no source names the device; a NaN
 *      or infinite t; rule 4; every refusal of vello_hip_render_resident (target, parameters); a scene whose bytes and copies
 *      together would reach 2^32 words (the copy must be reachable with the scene pointer and a u32 word offset).
 *   8. W BELONGS TO ITS FRAME.  Four frames in flight may show four values of t, or four device tensors, in four targets.  A
 *      vello_hip_render_resident frame that follows a morphed one on the same buffer set shows the scene's own points.  No frame
 *      modifies the resident bytes or the keyframes.  The room for the copies is made at most once per resident scene, by
 *      vello_hip_upload_path_keyframes or by the first morphed frame: that may re-allocate the scene buffer, which waits for the
 *      frames in flight and counts in vello_hip_scene_allocations.  A steady state of morphed frames allocates nothing.
 *   9. Out of scope: morphing private scenes (vello_hip_render_frame), composed instance frames and the retained list; keyframes
 *      whose tag streams differ; easing curves, or more than two sources per frame; host-memory sources per frame (a host uploads
 *      keyframes); pool estimation for morphed frames -- an overflow is reported at vello_hip_sync as always, and
 *      vello_hip_grow_pools plus a second call render the frame again. */
#define VELLO_HIP_PATH_DATA_SCENE 0xFFFFFFFFu  /* the resident scene's own path-data stream */
#define VELLO_HIP_PATH_DATA_DEVICE 0xFFFFFFFEu /* the caller's device memory (device_words) */
uint32_t vello_hip_path_data_words(vello_hip_ctx *ctx);
int vello_hip_upload_path_keyframes(vello_hip_ctx *ctx, const uint32_t *words, uint32_t n_keys, uint32_t n_words);
int vello_hip_render_resident_morphed(vello_hip_ctx *ctx, uint32_t src_a, uint32_t src_b, float t,
                                      const uint32_t *device_words /* nullable */, void *src_stream /* nullable hipStream_t */,
                                      const vello_hip_render_params *params, void *out_device, size_t out_stride);

/* Hit testing: the topmost draw object, and the instance that owns it, under each of n points of the frame submitted last on the
 * context -- the frame whose buffers vello_hip_read_buffer shows.  The reference has no hit test; like instances and views this
 * extends the boundary, and the contract is stated here.  Everything is read from what the frame left on the device (the line soup,
 * the draw monoids, the path boxes' draw flags, the composition's draw-tag prefix): no geometry is flattened on the host, a retained
 * list whose poses live only in device memory is answered like any other frame, and a view transform or poses need no handling of
 * their own -- the soup is in target space already.
 *   A point is (qx, qy) in target pixel coordinates: f32, y down, pixel (x, y) centred on (x + 0.5, y + 0.5).
 *   1. WINDING of a path at the point, over the frame's line soup (lines with path_ix >= n_paths are skipped).  For a line (p0, p1)
 *      all six f32 values are promoted to f64 and d = (p1x - p0x) * (qy - p0y) - (qx - p0x) * (p1y - p0y) is formed without
 *      contraction into FMA.  An upward line (p0y <= qy && qy < p1y) adds +1 when d < 0; a downward line (p1y <= qy && qy < p0y)
 *      adds -1 when d > 0.  Every comparison is written so that a NaN coordinate counts nothing; a point exactly on a line counts
 *      nothing for that line.  A path is HIT when its winding is != 0 (non-zero fill) or odd (even-odd fill: draw_flags &
 *      DRAW_INFO_FLAGS_FILL_RULE_BIT of its path box).  The sum does not depend on the order of the lines.  Strokes are in the soup
 *      as their outlines: a stroke is hit inside its width.
 *   2. VISIBILITY under clips.  Walking the draw objects in order with a stack: BeginClip pushes the hit bit of its path, a matched
 *      EndClip pops, a paint draw (fill colour, the three gradients, image, blurred rect) is a CANDIDATE when its own path is hit
 *      and every bit on the stack is set.  The result is the largest candidate draw index, or VELLO_HIP_PICK_NONE.  Blend modes and
 *      alpha play no part: a pick is geometric, a transparent fill is still hit.  Clip streams as Scene produces them (balanced) are
 *      in the contract; for others the result is unspecified, but the call completes.
 *   3. A point that is not finite, or outside [0, width) x [0, height) of that frame, is VELLO_HIP_PICK_NONE -- which also makes the
 *      answer independent of vello_hip_set_viewport_cull: the lines culling drops lie above, below or right of the target and
 *      cannot cross a leftward ray from a point inside it.  Such host points are not refused: a cursor off the window is ordinary
 *      input.
 *   4. INSTANCE.  Where the frame was composed from instances (vello_hip_render_instances, _painted, vello_hip_render_retained)
 *      instance_ix is the instance that owns the draw index: the last entry of the draw-tag stream's prefix that is <= it (empty
 *      fragments repeat an offset; the last one of a run holds the draw).  For any other frame, and where draw_ix is
 *      VELLO_HIP_PICK_NONE, it is VELLO_HIP_PICK_NONE.
 * THE CALL BLOCKS: it waits for the last submitted frame, runs the pick behind it on that frame's stream and returns once `out` is
 * written -- host memory (out_is_device == 0) or device memory, n entries either way.  `points` is n x 2 floats in host memory
 * (copied during the call) or in device memory (points_is_device != 0: 4-byte aligned, in one allocation of the context's device);
 * with `src_stream` (a hipStream_t; device points only) the read of the points waits for what has been enqueued on that stream so
 * far, as vello_hip_copy_images_device and vello_hip_render_retained order theirs.  n == 0 returns VELLO_HIP_OK and does nothing.
 * If the frame failed (bump.failed != 0: a pool overflowed and the soup is short, or the scene was bad) the call returns the code
 * vello_hip_sync reports for it -- VELLO_HIP_E_CAPACITY or VELLO_HIP_E_INVALID -- and writes nothing.  The call changes nothing that
 * a later vello_hip_sync, vello_hip_get_bump, vello_hip_read_buffer or the next frame sees: it does not move the rotation of the
 * in-flight buffer sets, allocates no scene buffer and writes none of the frame's buffers (its scratch -- a winding table of
 * queries x paths words per batch of queries, at most 16 MB unless one query's row is larger -- is the context's own).
 * VELLO_HIP_E_INVALID, with vello_hip_last_error naming the rule and nothing enqueued: a NULL context, `points` or `out`; n >
 * VELLO_HIP_PICK_MAX_POINTS; no frame was ever rendered (or its pools were grown or its scene replaced since); src_stream with host
 * points; a device pointer that is misaligned or (GPU builds) not device memory of the context's device. */
#define VELLO_HIP_PICK_NONE 0xFFFFFFFFu
#define VELLO_HIP_PICK_MAX_POINTS 4096u
typedef struct vello_hip_pick_hit { uint32_t draw_ix, instance_ix; } vello_hip_pick_hit;
int vello_hip_pick(vello_hip_ctx *ctx, const float *points /* n x 2 */, uint32_t n, int points_is_device,
                   void *src_stream /* nullable hipStream_t */, vello_hip_pick_hit *out /* n entries */, int out_is_device);
/* Measurement seam: milliseconds between two events around the launches of the last vello_hip_pick -- every batch's zero fill and two
 * kernels, not the wait for the frame nor the copies of host points and results -- or of the last vello_hip_pick_rect (its zero fill
 * and four kernels), whichever call came last; taken when vello_hip_set_profiling has any stage enabled; 0 otherwise
 * (scripts/pick_bench.py, scripts/pick_rect_bench.py). */
int vello_hip_pick_ms(vello_hip_ctx *ctx, float *ms_out);
/* Test seam: the shapes of the pick's kernels, so that tests place their cases on the boundaries -- lines per workgroup of the line
 * pass, draw objects per step of the resolve pass, queries per batch under VELLO_HIP_DEBUG_PICK_SMALL_BATCHES, bytes of the
 * winding-table budget; lines per workgroup of vello_hip_pick_rect's line pass and draw objects per workgroup of its draw pass.  0 for
 * any other `which`. */
enum { VELLO_HIP_PICK_LINES_PER_WORKGROUP = 0, VELLO_HIP_PICK_DRAWS_PER_STEP = 1, VELLO_HIP_PICK_SMALL_BATCH = 2, VELLO_HIP_PICK_SCRATCH_BYTES = 3,
       VELLO_HIP_PICK_RECT_LINES_PER_WORKGROUP = 4, VELLO_HIP_PICK_RECT_DRAWS_PER_WORKGROUP = 5 };
uint32_t vello_hip_pick_constant(int which);

/* Marquee selection: which draw objects, and which instances, a rectangle of the frame submitted last touches and which it encloses --
 * "the frame" exactly as vello_hip_pick defines it.  The reference has no such query; like vello_hip_pick this extends the boundary
 * and the contract is stated here.  It reads what the frame left on the device (the line soup in target space, the path boxes with
 * their fill rules, the draw monoids, the composition's draw-tag prefix); the words it writes are what a caller turns into the paints
 * of vello_hip_render_retained_painted, in device memory if it likes, so a selection can be shown in the next frame without the host
 * reading it.  draws_out[i] is the word of draw object i, instances_out[k] the word of instance k of a frame composed from instances
 * (vello_hip_render_instances, _painted, vello_hip_render_retained, _retained_painted); a word holds VELLO_HIP_REGION_TOUCHED,
 * VELLO_HIP_REGION_ENCLOSED, both or neither, and no other bit.
 *   0. THE REGION R'.  rect is (x0, y0, x1, y1) in target pixel coordinates, f32.  With W and H the frame's target size and all
 *      arithmetic in f32: x0' = max(min(x0, x1), 0), x1' = min(max(x0, x1), W), and y0', y1' likewise with H -- a rectangle dragged
 *      right to left is ordinary input, infinities clamp.  R' is EMPTY when a coordinate is NaN or !(x0' < x1' && y0' < y1'); an empty
 *      R' selects nothing: every output word is 0, the counts are 0, the call returns VELLO_HIP_OK.  The probe point C of a non-empty
 *      R': cx = x0' + (x1' - x0') * 0.5f, replaced by x0' when !(cx < x1'); cy likewise.  C lies in the target, and cy < H.
 *   1. PER PATH, over the counted lines of the soup (path_ix < n_paths).  Every comparison is written so that a NaN coordinate fails.
 *      MEETS: some line (p0, p1) of the path passes both (a) the f32 box test, all strict: min(p0x, p1x) < x1' && max(p0x, p1x) >
 *      x0' && min(p0y, p1y) < y1' && max(p0y, p1y) > y0', and (b) the four corners of R' are not all strictly on one side of it: with
 *      d(q) = (p1x - p0x) * (qy - p0y) - (qx - p0x) * (p1y - p0y), formed in f64 from the promoted f32 values without contraction (as
 *      in vello_hip_pick's rule 1), the four d are not all > 0 and not all < 0.  (Together: the separating-axis test of a segment
 *      against a box.  Strict, so a line that only runs along the boundary of R' does not meet it.)
 *      HIT: the path is hit at C by vello_hip_pick's rule 1 -- the same winding sum and fill rule, without rule 3's in-target test.
 *      TOUCH = MEETS or HIT: an outline crosses R', or R' lies inside the fill (a marquee within a large shape meets no line).
 *      BOXED: the path's PathBbox (the integer box flatten leaves) satisfies x0' <= bx0 && bx1 <= x1' && y0' <= by0 && by1 <= y1'.
 *   2. PER DRAW OBJECT, walking the draw objects with vello_hip_pick's clip stack: BeginClip pushes TOUCH of its path, a matched
 *      EndClip pops; a paint draw (the pick's six tags) is TOUCHED when TOUCH holds for its own path and every bit on the stack is
 *      set, and ENCLOSED when it is TOUCHED and its path is BOXED.  Every other draw object's word is 0.  THIS IS A PER-PATH RULE, NOT
 *      A PER-PIXEL ONE: a draw can be TOUCHED although the part of it inside R' is covered by later draws, or although its clip meets
 *      R' somewhere else than it does.  Blend modes and alpha play no part, as in a pick.
 *   3. PER INSTANCE k, which owns the draws [prefix[k], prefix[k + 1]): TOUCHED when one of its draws is TOUCHED; ENCLOSED when one of
 *      its draws is ENCLOSED and none of its paint draws whose path box is non-empty (bx0 < bx1 && by0 < by1) fails to be ENCLOSED.
 *      Empty fragments get 0.
 *   4. INDEPENDENT OF VIEWPORT CULLING (vello_hip_set_viewport_cull).  A culled line lies wholly at y <= 0, at y >= 16 * ceil(H / 16)
 *      or at x >= 16 * ceil(W / 16): it fails a strict box test against R', which lies in [0, W] x [0, H], and a leftward ray from C
 *      (0 <= cy < H, cx < W) cannot count it.  Path boxes do not change under culling (rule 1 of that contract).
 *   5. COUNTS.  counts_out receives the four totals, in host memory, whenever the call succeeds.
 *   6. SIZES AND REFUSALS.  vello_hip_pick_rect_sizes gives the frame's n_draw_objects and its instance count (0: the frame was not
 *      composed from instances); the outputs that are not NULL have exactly these sizes.  VELLO_HIP_E_INVALID, with
 *      vello_hip_last_error naming the rule, nothing enqueued and every output untouched: a NULL context or rect; draws_out,
 *      instances_out and counts_out all NULL; draws_out with n_draws different from the frame's count; instances_out with n_instances
 *      different from the frame's instance count, or on a frame that has no instances; a device output that is misaligned or (GPU
 *      builds) not device memory of the context's device; no frame to answer against by vello_hip_pick's rules (never rendered, pools
 *      grown since, scene replaced since).  A frame with bump.failed != 0 returns the code vello_hip_sync reports for it and writes
 *      nothing, as vello_hip_pick does.
 * One rectangle per call, in host memory.  THE CALL BLOCKS, on the frame's stream behind the frame, like vello_hip_pick; with
 * out_is_device != 0 draws_out and instances_out are device memory (4-byte aligned) that the kernels write directly.  It does not
 * move the rotation of the in-flight buffer sets, allocates no scene buffer and writes none of the frame's buffers: its scratch (two
 * words per path, one per instance, one per workgroup of the draw pass) is the context's own.  Out of scope: lassos, several
 * rectangles a call, rectangles in device memory, per-pixel visibility. */
enum { VELLO_HIP_REGION_TOUCHED = 1, VELLO_HIP_REGION_ENCLOSED = 2 };
typedef struct vello_hip_region_counts { uint32_t draws_touched, draws_enclosed, instances_touched, instances_enclosed; } vello_hip_region_counts;
int vello_hip_pick_rect_sizes(vello_hip_ctx *ctx, uint32_t *n_draws_out, uint32_t *n_instances_out);
int vello_hip_pick_rect(vello_hip_ctx *ctx, const float rect[4] /* x0 y0 x1 y1, host */,
                        uint32_t *draws_out /* nullable */, uint32_t n_draws,
                        uint32_t *instances_out /* nullable */, uint32_t n_instances,
                        int out_is_device, vello_hip_region_counts *counts_out /* nullable, host */);
/* Test seam: the sizes at which the pipeline's kernels and the host's launch switches cut their work, so that tests place tags, draw
 * objects, clips, lines and tile rows on those boundaries -- tags per partition of the pathtag scan's look-back and per block of
 * flatten's light pass; draw objects per partition of the draw scan; clips per partition of the clip kernels; draw objects (paths)
 * per workgroup of binning, tile_alloc and coarse's prepass; draw objects per batch of k_coarse and the number of bins its grid is
 * rounded up to; lines per chunk of path_count's three forms (soup size unknown with one frame in flight, soup known to be small,
 * frames in flight); SegmentCounts per workgroup of path_tiling; tiles per block of backdrop's row scan; the most tags and draw
 * objects (paths) of a scene whose front stages share launches, and the most segments of one whose front is ONE launch.  Then
 * fine's: the command words k_fine reads at a time; the fills, segments and crossing records a batch of fills holds at most; the
 * most records of a fill that takes the straight-line replay; how many words behind a prefetched window's base the list may resume
 * for the window to be used; the fills per slice of a long tile and the fills from which a tile is sliced (one frame in flight,
 * frames in flight; both under VELLO_HIP_DEBUG_FINE_SLICES); the command words from which a tile counts as heavy; the words per
 * bucket and the buckets of fine's tile order; the words of a tile's fixed command block; the words a workgroup of k_path_blend
 * takes per grid step in its 16-byte form.  0 for any other `which`. */
enum { VELLO_HIP_SHAPE_PATHTAG_PART_TAGS = 0, VELLO_HIP_SHAPE_FLATTEN_BLOCK_TAGS = 1, VELLO_HIP_SHAPE_DRAW_PART = 2, VELLO_HIP_SHAPE_CLIP_PART = 3,
       VELLO_HIP_SHAPE_DRAW_WORKGROUP = 4, VELLO_HIP_SHAPE_COARSE_BATCH = 5, VELLO_HIP_SHAPE_COARSE_GRID_BINS = 6,
       VELLO_HIP_SHAPE_PATH_COUNT_CHUNK = 7, VELLO_HIP_SHAPE_PATH_COUNT_CHUNK_SMALL = 8, VELLO_HIP_SHAPE_PATH_COUNT_CHUNK_IN_FLIGHT = 9,
       VELLO_HIP_SHAPE_PATH_TILING_WORKGROUP = 10, VELLO_HIP_SHAPE_BACKDROP_BLOCK_TILES = 11, VELLO_HIP_SHAPE_FRONT_MAX_TAGS = 12,
       VELLO_HIP_SHAPE_FRONT_MAX_DRAW_OBJECTS = 13, VELLO_HIP_SHAPE_FRONT_TINY_SEGMENTS = 14,
       VELLO_HIP_SHAPE_FINE_WINDOW_WORDS = 15, VELLO_HIP_SHAPE_FINE_BATCH_FILLS = 16, VELLO_HIP_SHAPE_FINE_BATCH_SEGMENTS = 17,
       VELLO_HIP_SHAPE_FINE_ITEM_CAP = 18, VELLO_HIP_SHAPE_FINE_SIMPLE_RECORDS = 19, VELLO_HIP_SHAPE_FINE_PREFETCH_REACH = 20,
       VELLO_HIP_SHAPE_FINE_SLICE_FILLS = 21, VELLO_HIP_SHAPE_FINE_SLICE_MIN_FILLS = 22, VELLO_HIP_SHAPE_FINE_SLICE_MIN_FILLS_IN_FLIGHT = 23,
       VELLO_HIP_SHAPE_FINE_SLICE_FILLS_FORCED = 24, VELLO_HIP_SHAPE_FINE_SLICE_MIN_FILLS_FORCED = 25, VELLO_HIP_SHAPE_FINE_HEAVY_WORDS = 26,
       VELLO_HIP_SHAPE_FINE_BUCKET_WORDS = 27, VELLO_HIP_SHAPE_FINE_BUCKETS = 28, VELLO_HIP_SHAPE_PTCL_INITIAL_ALLOC = 29,
       VELLO_HIP_SHAPE_PATH_BLEND_VEC_WORDS = 30, /* words a workgroup of k_path_blend takes per grid step in its 16-byte form */
       VELLO_HIP_SHAPE_COUNT = 31 };
uint32_t vello_hip_stage_constant(int which);

/* Test-seam switches (default 0).  VELLO_HIP_DEBUG_NO_CULL turns off coarse's occlusion culling (a draw hidden under a
 * later opaque full-tile cover is normally not emitted; the image is the same, but bump.segments / bump.ptcl and the
 * PTCL words are then <= the reference's): with it set, PTCL, segment slices and every bump counter equal the
 * reference's (coarse.wgsl:156-471) up to the order its atomics hand out slices and chunks.
 * VELLO_HIP_DEBUG_STROKE_KERNEL runs the stroked-line kernel of flatten for any number of stroked lines (it normally takes
 * over from 393 216 of them): same lines, a different kernel -- so that small test scenes exercise it.
 * VELLO_HIP_DEBUG_SEQ_CLIP matches clips with the one-wave stack machine that otherwise only takes scenes of more than
 * 524 288 clips (clip_reduce.wgsl / clip_leaf.wgsl run as partitioned kernels below that): same clip boxes.
 * VELLO_HIP_DEBUG_FINE_SLICES cuts EVERY tile's command list into slices of 4 fills for fine's MSAA modes (normally only
 * lists of >= 96 fills are cut, into slices of 32: the slices' coverage is computed by separate waves and the last one to
 * finish composites the tile): same image -- so that small test scenes exercise the sliced path.
 * VELLO_HIP_DEBUG_FLATTEN_COOP / _ALONE pick the kernels that flatten the scene's curves, stroked curves, joins and caps: the
 * wave-cooperative walk, or every lane on its own (normally the engine picks by what an earlier frame of the same scene put on
 * the list, and by the scene's size before there is one): same line soup as a multiset -- so that tests can hold both sets of
 * kernels to the oracle on the same scenes.
 * VELLO_HIP_DEBUG_NO_FUSION launches every stage of a small scene as a kernel of its own (normally the workgroups of consecutive
 * stages up to tile_alloc share launches when the scene is small enough for launch boundaries to matter): same buffers.
 * VELLO_HIP_DEBUG_PICK_SMALL_BATCHES answers the queries of a vello_hip_pick call three at a time (normally as many as fit the
 * winding-table budget): same answers -- so that a handful of queries on a small scene spans several batches.
 * VELLO_HIP_DEBUG_NO_SCENE_INDEX renders a resident scene that has an index (vello_hip_scene_index_builds) without it: the zero
 * fill, the pathtag scan and the whole-stream light pass of every frame, as for a scene that has none: same buffers -- for A/Bs and so
 * that tests can hold the two paths to each other.  It applies to whole frames: set it between frames, not between the stages of one. */
enum { VELLO_HIP_DEBUG_NO_CULL = 1, VELLO_HIP_DEBUG_STROKE_KERNEL = 2, VELLO_HIP_DEBUG_SEQ_CLIP = 4, VELLO_HIP_DEBUG_FINE_SLICES = 8,
       VELLO_HIP_DEBUG_FLATTEN_COOP = 16, VELLO_HIP_DEBUG_FLATTEN_ALONE = 32, VELLO_HIP_DEBUG_NO_FUSION = 64,
       VELLO_HIP_DEBUG_PICK_SMALL_BATCHES = 128, VELLO_HIP_DEBUG_NO_SCENE_INDEX = 256,
       /* measurement seam: bits 24-27 = 1 + the last stage vello_hip_render_resident launches (0: all of them) -- what the stages
        * up to k cost with frames in flight (scripts/experiments/r6_stage_marginal.py); the frames are incomplete */
       VELLO_HIP_DEBUG_LAST_STAGE_SHIFT = 24 };
int vello_hip_set_debug_flags(vello_hip_ctx *ctx, uint32_t flags);

/* Number of frames the context keeps in flight (default 1, max 8).  wgpu queues recordings without waiting
 * (wgpu_engine.rs:757); with n > 1 consecutive vello_hip_render_resident calls rotate over n private buffer
 * sets and streams and overlap on the GPU.  The caller must hand each in-flight frame its own target.
 *
 * Frames overlap only where their streams dispatch on different hardware queues.  The HIP runtime keeps a pool of hardware queues
 * per stream priority, each capped on its own (GPU_MAX_HW_QUEUES, 4 by default), and gives a new stream a new queue of its pool
 * until the cap, then the queue with the fewest streams.  When the device has a range of stream priorities the context therefore
 * creates its frames' streams with ONE priority that is not the default's (the greatest), so that up to as many frames in flight
 * as the cap allows have a hardware queue each whatever the process's other streams -- the null stream, the caller's, the
 * context's own upload and copy streams -- hold in the default pool; more frames in flight than the cap share queues by the
 * runtime's rule.  Without a range, or when such a stream cannot be created, the streams are of the default priority.  The
 * environment variable VELLO_HIP_DEBUG_LANE_QUEUES, read once by vello_hip_create, is the A/B seam: `default` creates the streams
 * with the default priority (hipStreamCreateWithFlags), `least` / `greatest` pick that end of the device's range; any other value
 * fails vello_hip_create with VELLO_HIP_E_INVALID. */
int vello_hip_set_frames_in_flight(vello_hip_ctx *ctx, uint32_t n);
/* The stream priority of frame lane `lane` (0 <= lane < the greatest number of frames in flight set so far), as
 * hipStreamGetPriority reports it, and the device's range as hipDeviceGetStreamPriorityRange does (a numerically LOWER value is a
 * greater priority; least == greatest: the device has none).  Read-only; any of the three pointers may be NULL.  Lets a test see
 * the placement rule above without a profiler.  VELLO_HIP_E_INVALID for a lane the context has not created. */
int vello_hip_lane_stream_priority(vello_hip_ctx *ctx, uint32_t lane, int *priority, int *device_least, int *device_greatest);
/* Waits for the frame enqueued `age` vello_hip_render_resident calls ago (0 = newest, age < frames in flight)
 * without draining the younger ones; does not inspect bump.failed (vello_hip_sync does). */
int vello_hip_sync_frame(vello_hip_ctx *ctx, uint32_t age);
/* Waits for everything enqueued; returns VELLO_HIP_E_CAPACITY if a frame overflowed. */
int vello_hip_sync(vello_hip_ctx *ctx);
int vello_hip_get_bump(vello_hip_ctx *ctx, vello_hip_bump *out);
/* The hipStream_t the context launches on (for callers that record their own events). */
void *vello_hip_get_stream(vello_hip_ctx *ctx);

/* Multi-GPU exchange for a host that owns one context per GPU in one process: the frame each context
 * enqueued last (src_frames[i], device memory of ctxs[i]'s GPU) is copied to dst_frames[i] on `dst_device` with
 * hipMemcpyPeerAsync on a per-context copy stream, ordered behind that frame by an event: SDMA over the peer's own xGMI
 * link, no CUs, all peers concurrently.  Returns without waiting; vello_hip_gather_wait blocks until the copies have
 * landed.  (One process per GPU gathers with RCCL instead: vello_amd/distributed.py, bench.py --gpus N.) */
int vello_hip_gather_frames(vello_hip_ctx *const *ctxs, uint32_t n, int dst_device, const void *const *src_frames, void *const *dst_frames,
                            size_t frame_bytes);
int vello_hip_gather_wait(vello_hip_ctx *const *ctxs, uint32_t n);

/* Differential-test seam: run stages [first, last] of the resident scene; read/write any buffer. */
int vello_hip_run_stages(vello_hip_ctx *ctx, const vello_hip_render_params *params, int first_stage, int last_stage);
int vello_hip_read_buffer(vello_hip_ctx *ctx, int buf_id, void *dst, size_t offset, size_t size);
int vello_hip_write_buffer(vello_hip_ctx *ctx, int buf_id, const void *src, size_t offset, size_t size);
size_t vello_hip_buffer_size(vello_hip_ctx *ctx, int buf_id);

/* Per-stage GPU timing with hipEvents on the launch stream.  stage_mask bit i enables events
 * around stage i; times accumulate until read.  vello_hip_get_stage_ms syncs, writes the summed
 * milliseconds and launch counts per stage, and resets the accumulators. */
int vello_hip_set_profiling(vello_hip_ctx *ctx, uint32_t stage_mask);
int vello_hip_get_stage_ms(vello_hip_ctx *ctx, float ms_out[VELLO_HIP_STAGE_COUNT], uint32_t count_out[VELLO_HIP_STAGE_COUNT]);
/* The stages that are several kernels, kernel by kernel (events between the launches while the stage is profiled):
 * VELLO_HIP_STAGE_FLATTEN -> k_flatten_light, k_flatten_main, k_flatten_tail with one frame in flight (k_flatten_light,
 * k_flatten_strokes, k_flatten_heavy with several: vello_hip_set_frames_in_flight); VELLO_HIP_STAGE_COARSE -> k_coarse_prep,
 * k_coarse (third entry 0).  Summed milliseconds since the last call and the number of profiled launches of the stage;
 * zeros for a stage of one kernel (its time is vello_hip_get_stage_ms's).  Reading resets the sums. */
int vello_hip_get_kernel_ms(vello_hip_ctx *ctx, int stage, float ms_out[3], uint32_t *count_out);

const char *vello_hip_stage_name(int stage);
const char *vello_hip_last_error(vello_hip_ctx *ctx /* nullable: last create() error */);

/* vello_encoding::make_mask_lut / make_mask_lut_16 (vello_encoding/src/mask.rs:36-98); exported so
 * the host can check the persistent LUT the engine keeps on the device. */
void vello_hip_make_mask_lut(uint8_t out[1024]);
void vello_hip_make_mask_lut_16(uint8_t out[8192]);

#ifdef __cplusplus
}
#endif
#endif
