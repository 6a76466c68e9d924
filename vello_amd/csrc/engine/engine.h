// Engine-internal interface between the host driver (ctx.h and the sources that include it) and the kernel translation units.
#pragma once
#include <cstddef>
#include "common.h"

namespace vk {

// Single-pass decoupled look-back state: per partition, NF granules for the workgroup aggregate
// followed by NF granules for the inclusive prefix.  A granule is one naturally aligned 8-byte
// {status:32, value:32} word written exactly once per frame by ONE relaxed agent-scope store
// (write-through), so it is never torn and needs no separate flag or fence
// (cdna_hip_programming.md guideline 16, form R2).
constexpr uint32_t SCAN_STATUS_AGG = 1, SCAN_STATUS_PREFIX = 2;
constexpr uint32_t PATHTAG_PART_WORDS = 1024;  // 256 threads x 4 tag words (= 4096 tags)
constexpr uint32_t DRAW_PART = 256;            // draw objects per partition
constexpr uint32_t DRAW_WG = 256;              // draw objects (k_binning, k_coarse_prep) or paths (k_tile_alloc) per workgroup: a thread each
#ifndef VK_FLATTEN_TPT
#define VK_FLATTEN_TPT 4
#endif
constexpr uint32_t FLATTEN_TAGS_PER_THREAD = VK_FLATTEN_TPT;
constexpr uint32_t FLATTEN_BLOCK_TAGS = 256 * FLATTEN_TAGS_PER_THREAD;
#ifndef VK_PC_LPT
#define VK_PC_LPT 4
#endif
constexpr uint32_t PATH_COUNT_LINES_PER_THREAD = VK_PC_LPT;
constexpr uint32_t PATH_COUNT_CHUNK = 256 * PATH_COUNT_LINES_PER_THREAD;
// A soup of fewer lines than this (known from a finished frame of the scene) is cut into chunks of 256 lines instead of 1 024:
// a chunk is 15-20 us of dependent phases whatever its size, and the tiger's 15 000 lines are 15 workgroups of the large kind
// on 256 CUs.  (768 workgroups of k_path_count are resident at once.)
constexpr int64_t PATH_COUNT_SMALL_MAX_LINES = 768 * 256;
// Spin bound for look-back waits: a predecessor always holds a smaller ticket, so it is resident
// or finished; the bound only turns a driver-level hang into a reported failure.
constexpr uint32_t SPIN_LIMIT = 1u << 24;
constexpr uint32_t FAILED_INTERNAL = 0x80000000u;  // set in bump.failed when a spin bound trips
// set in bump.failed by the pathtag scan when the tag stream asks for more path data, transforms, styles or paths
// than the scene buffer / layout hold (WebGPU's robust buffer access makes this harmless upstream; HIP has none):
// every later stage that would index with those counts bails out, the frame reports VELLO_HIP_E_INVALID
constexpr uint32_t FAILED_SCENE = 0x40000000u;
constexpr uint32_t FINE_WORK_BUCKETS = 32;  // buckets of FINE_BUCKET_WORDS command words (the last one: 992 and more)
constexpr uint32_t FINE_BUCKET_WORDS = 32;
// Stroked lines get workgroups of their own (beside the heavy list's in k_flatten_main with one frame in flight, as
// k_flatten_strokes ahead of k_flatten_heavy with several) once they alone fill the chip twice over at 12 waves per CU
// (256 CUs x 12 x 64 lanes); below that they are entries of the heavy list, whose duration the curves set anyway.
constexpr uint32_t FLATTEN_STROKE_KERNEL_MIN_LINES = 2u * 256u * 12u * 64u;
// command words from which a tile counts as long: its wave raises its issue priority (s_setprio) in k_fine
constexpr uint32_t FINE_HEAVY_WORDS = 384;
// fine, MSAA modes: a tile whose list holds >= FINE_SLICE_MIN_FILLS FILLs is cut into slices of FINE_SLICE_FILLS fills; every
// slice is a work item of its own (one wave computes the coverage of its fills into the coverage scratch), and the wave that
// finishes a tile's last slice composites the tile from the scratch (fine.hip).  k_fine's launch is as long as its longest
// tile's chain of fills otherwise (d2: 137 fills, 258 us against 117 us of balanced work).
#ifndef VK_SLICE_FILLS
#define VK_SLICE_FILLS 32
#endif
#ifndef VK_SLICE_MIN_FILLS
#define VK_SLICE_MIN_FILLS 96
#endif
constexpr uint32_t FINE_SLICE_FILLS = VK_SLICE_FILLS, FINE_SLICE_MIN_FILLS = VK_SLICE_MIN_FILLS;
// With frames in flight the tail of k_fine's launch is filled by the other frames' kernels, and what slicing costs -- the coverage
// through memory, a second pass over the list -- is no longer paid back: the threshold is higher there (round 6,
// profiles/r06_ab_slices_in_flight.txt).
#ifndef VK_SLICE_MIN_FILLS_IN_FLIGHT
#define VK_SLICE_MIN_FILLS_IN_FLIGHT 192
#endif
#ifndef VK_SLICE_FILLS_IN_FLIGHT
#define VK_SLICE_FILLS_IN_FLIGHT VK_SLICE_FILLS
#endif
constexpr uint32_t FINE_SLICE_FILLS_IN_FLIGHT = VK_SLICE_FILLS_IN_FLIGHT, FINE_SLICE_MIN_FILLS_IN_FLIGHT = VK_SLICE_MIN_FILLS_IN_FLIGHT;
constexpr uint32_t FINE_SLICE_FILLS_FORCED = 4, FINE_SLICE_MIN_FILLS_FORCED = 5;  // VELLO_HIP_DEBUG_FINE_SLICES
struct SliceItem {
    uint32_t tile_ix;     // ~0: a hole left by a tile whose slices did not fit the capacity
    uint32_t k_and_n;     // slice | slices of the tile << 16
    uint32_t cov_base;    // first word of the tile's coverage scratch: 64 words (one byte per pixel) per FILL
    uint32_t first_item;  // index of the tile's first item: its arrival counter is slice_counters[first_item]
};
// clip matching (clip.hip): clips per partition (a thread each) and the most partitions the one-workgroup stack pass holds
// in LDS; beyond CLIP_PART * CLIP_MAX_PARTS clips the one-wave stack machine (draw.hip) runs instead
constexpr uint32_t CLIP_PART = 256;
constexpr uint32_t CLIP_MAX_PARTS = 2048;
struct ClipEl { uint32_t clip_ix; float x0, y0, x1, y1; };  // an open BeginClip: its index in clip_inp, its box ∩ its local ancestors'
__host__ __device__ inline uint32_t clip_parts_pad(uint32_t parts) {  // leaves of the min-tree over the partitions
    uint32_t n = 2u;
    while (n < parts) n <<= 1;
    return n;
}
// words of Frame::clip_stack: the sequential machine's spill area (6 words per clip) or the partitions' scratch
// (open pushes, Bic, height, box below: 1287 words per partition; then the min-tree)
inline size_t clip_scratch_words(uint32_t n_clips) {
    size_t parts = (n_clips + CLIP_PART - 1u) / CLIP_PART;
    size_t par = parts * (CLIP_PART * 5u + 4u + 2u + 1u) + 2u * (size_t)clip_parts_pad((uint32_t)parts);
    size_t seq = ((size_t)n_clips + 1u) * 6u;
    return par > seq ? par : seq;
}

// Words of the per-frame control block (zeroed by ONE hipMemsetAsync per frame, together with
// the bump allocators and both look-back state arrays which follow it in the same allocation).
struct Control {
    Bump bump;              // must be first: VELLO_HIP_BUF_BUMP aliases it
    uint32_t ticket_pathtag;
    uint32_t ticket_draw;
    uint32_t heavy_count[4];  // flatten: tags queued by k_flatten_light: [0] fill curves, [1] strokes, [2] stroked lines; [3] stroked lines
                              // the stroke workgroups of k_flatten_main hand on to k_flatten_tail
    uint32_t pad[2];
    uint32_t work_count[FINE_WORK_BUCKETS];  // coarse -> fine: tiles per bucket of command-list length (k_fine runs the long ones first)
    uint32_t slice_items;   // coarse -> fine: SliceItems handed out (may run past the capacity: fine clamps); work_count[BUCKETS]
    uint32_t cov_words;     // coarse -> fine: words of the coverage scratch handed out
    // coarse prep -> coarse: any word nonzero = the scene holds an opaque solid-colour fill (k_coarse then walks its lists back to
    // front).  One flag in COARSE_OPAQUE_SHARDS words: every wave of k_coarse_prep that sees such a fill says so, and a scene of
    // 100 000 of them would otherwise send 1 800 atomics to one address (~12 ns each, see arc_count)
    uint32_t opaque_fills[8];
    uint32_t pad2[48 - FINE_WORK_BUCKETS - 2 - 8];
    // flatten: arcs the stroke workgroups set aside, counted in FLATTEN_ARC_SHARDS sub-lists (workgroup b appends to shard b mod
    // 64): ONE counter took 2 800 same-address atomics of ~12 ns each in a burst -- 30 us on the road-map scene
    uint32_t arc_count[64];
};
static_assert(sizeof(Control) == 512, "Control");
// (coarse and fine reach slice_items / cov_words through the work_count pointer)
static_assert(offsetof(Control, slice_items) == offsetof(Control, work_count) + 4u * FINE_WORK_BUCKETS, "Control::slice_items follows work_count");
static_assert(offsetof(Control, cov_words) == offsetof(Control, slice_items) + 4u, "Control::cov_words follows slice_items");
constexpr uint32_t FLATTEN_ARC_SHARDS = 64;
constexpr uint32_t COARSE_OPAQUE_SHARDS = 8;
static_assert(sizeof(Control::opaque_fills) == 4u * COARSE_OPAQUE_SHARDS, "Control::opaque_fills");
// Stroke workgroups of a scene of at most n_seg_max segments.  Side by side with the heavy list's workgroups (one frame in flight,
// k_flatten_main): one per round of 256 stroked lines, up to 4 096.  As a launch of their own (frames in flight,
// k_flatten_strokes): 512 -- the two a CU holds -- striding over the rounds: four frames in flight +1.9 % on the road map; the same
// grid for k_flatten_main is 2.8 % slower one frame at a time (profiles/r04_ab_s21_strokes_grid.txt).
#ifndef VK_STROKES_GRID_SIDE_BY_SIDE
#define VK_STROKES_GRID_SIDE_BY_SIDE 4096u
#endif
#ifndef VK_STROKES_GRID_OWN_LAUNCH
#define VK_STROKES_GRID_OWN_LAUNCH 384u  // (scripts/emu_variant_check.sh sets both to 2: several rounds per workgroup on the emulator's small scenes)
#endif
inline uint32_t flatten_strokes_grid(uint32_t n_seg_max, bool side_by_side) {
    const uint32_t cap = side_by_side ? VK_STROKES_GRID_SIDE_BY_SIDE : VK_STROKES_GRID_OWN_LAUNCH;
    const uint32_t g = (n_seg_max + 255u) / 256u;
    return g > cap ? cap : (g < 1u ? 1u : g);
}
// the arcs one shard of the arc list can be given (256 per round of each of its workgroups); the list holds FLATTEN_ARC_SHARDS x
// that many 64-byte items
inline uint32_t flatten_arc_shard_cap(uint32_t n_seg_max, bool side_by_side) {
    const uint32_t grid = flatten_strokes_grid(n_seg_max, side_by_side);
    const uint32_t rounds = ((n_seg_max + 255u) / 256u + grid - 1u) / grid;
    return ((grid + FLATTEN_ARC_SHARDS - 1u) / FLATTEN_ARC_SHARDS) * (rounds < 1u ? 1u : rounds) * 256u;
}

// A damage rectangle (vello_hip_set_damage_rect) in pixels and the window of tiles that meet it, both half open.  Kernel arguments
// of k_fine and k_coarse (wave-uniform); not part of Config, which is the reference's layout.
struct PixelRect { uint32_t x0, y0, x1, y1; };
struct TileRect { uint32_t x0, y0, x1, y1; };
inline bool empty(const PixelRect &r) { return r.x0 >= r.x1 || r.y0 >= r.y1; }
// W: the tiles that meet R (no tile for an empty R)
inline TileRect damage_window(const PixelRect &r) {
    if (empty(r)) return TileRect{0u, 0u, 0u, 0u};
    return TileRect{r.x0 / TILE_WIDTH, r.y0 / TILE_HEIGHT, (r.x1 + TILE_WIDTH - 1u) / TILE_WIDTH, (r.y1 + TILE_HEIGHT - 1u) / TILE_HEIGHT};
}

struct Frame {
    Config cfg;  // host copy; kernels receive it by value
    uint32_t n_tag_words;
    uint32_t n_scene_words;  // length of the packed scene
    uint32_t aa;
    // device pointers
    const uint32_t *scene;
    // The transform words flatten and draw_leaf read: entry ix lies at scene[(u32)(xf_base + ix * 6)] (read_transform, common.h).
    // Without a view that is the scene's own stream (xf_base == cfg.layout.transform_base); with one (vello_hip_set_view_transform)
    // it is the lane's composed copy, which k_view_transforms fills at the head of the frame -- slot -1 holds the six words below the
    // stream verbatim, slots 0 .. n_xf-1 hold V.T.  The copy lives behind the scene's bytes in the scene's own allocation, so that it
    // is reached with the same pointer and a u32 word offset: the kernels that read transforms are handed a Config whose
    // layout.transform_base is xf_base (xf_config) and are the same code whether a view is set or not.  The pathtag scan keeps the
    // scene's own Config: it judges indices against the scene's layout.
    uint32_t xf_base;
    bool has_view;
    Xform view;
    // A frame of the retained instance list (vello_hip_render_retained): xf_base is ALWAYS the lane's copy, which k_instance_transforms
    // fills at the head of the frame from the list's owner table and this frame's poses (pose_words; null: the copy already holds
    // the frame's words, nothing is launched -- vello_hip_run_stages after a retained frame).  pose_stream (nullable) is the
    // caller's stream that waits for that kernel; pose_mark the event it does so through.  pose_check: the poses are the caller's
    // device memory, which the host has not read -- the kernel tests them (host poses and the rest poses were tested on the host).
    bool retained;
    const uint32_t *xf_owner;
    const uint32_t *pose_words;
    uint32_t n_instances;
    hipStream_t pose_stream;
    hipEvent_t pose_mark;
    bool pose_check;
    // The draw-data words the draw stage and k_coarse_prep read: scene[(u32)(dd_base + offset)].  The scene's own stream
    // (dd_base == cfg.layout.draw_data_base) for every frame but a PAINTED frame of the retained list
    // (vello_hip_render_retained_painted): there it is the lane's copy of the stream behind the retained bytes and the transform
    // copies, which k_instance_paints fills at the head of the frame from the list's per-word table (dd_map) and this frame's
    // paints (paint_words: [n][2] (flags, rgba); null: the copy already holds the frame's words, nothing is launched --
    // vello_hip_run_stages after a painted frame).  paint_check: the paints are the caller's device memory, which the host has
    // not read -- the kernel tests their flags.  The readers are handed a Config whose layout.draw_data_base is dd_base
    // (xf_config, dd_config) and are the same code whether the frame is painted or not.
    uint32_t dd_base;
    const uint32_t *dd_map;
    const uint32_t *paint_words;
    bool paint_check;
    // The path-data words flatten reads: scene[(u32)(pd_base + offset)].  The scene's own stream (pd_base == cfg.layout.path_data_base)
    // for every frame but a MORPHED frame of the resident scene (vello_hip_render_resident_morphed): there it is the lane's copy of
    // the stream behind the scene's bytes and the transform copies, which k_path_blend fills at the head of the frame from two
    // sources (pd_a, pd_b: the scene's stream, a resident keyframe or the caller's device memory; pd_a null: the copy already holds
    // the frame's words, nothing is launched -- vello_hip_run_stages after a morphed frame).  pd_mode / pd_t: PathBlendArgs.
    // pd_stream (nullable) is the caller's stream that waits for that kernel, through pose_mark.  The readers are handed a Config
    // whose layout.path_data_base is pd_base (xf_config) and are the same code whether the frame is morphed or not.  The pathtag
    // scan keeps the scene's own Config: it judges lengths against the scene's layout.
    uint32_t pd_base;
    const uint32_t *pd_a, *pd_b;
    uint32_t pd_mode;
    float pd_t;
    hipStream_t pd_stream;
    // The style words flatten reads: entry e lies at scene[(u32)(st_base + e * 2)] (flags, then the stroke width).  The scene's own
    // stream (st_base == cfg.layout.style_base) for every frame but one with a stroke scale (vello_hip_set_stroke_scale): there it
    // is the lane's copy behind the scene's bytes and the transform copies, which k_style_widths fills at the head of the frame --
    // slot -1 holds the two words below the stream verbatim, slot e the flags verbatim and the width under the rule of
    // StyleWidthArgs.  The readers are handed a Config whose layout.style_base is st_base (xf_config) and are the same code
    // whether a scale is set or not.  The pathtag scan keeps the scene's own Config: it judges the stream's length against
    // n_scene_words, and reads flags only.
    uint32_t st_base;
    bool has_stroke;
    float stroke_scale, stroke_min;
    Control *control;
    uint32_t *heavy_list;   // flatten: tag indices that need the Euler-spiral / stroker path
    uint32_t *arc_items;    // flatten: 16 words per round join / cap arc that a stroke workgroup leaves to the heavy code
    unsigned long long *pathtag_state;  // [n_pathtag_parts][2][5]
    unsigned long long *draw_state;     // [n_draw_parts][2][4]
    TagMonoid *tag_monoids;
    PathBbox *path_bboxes;
    LineSoup *lines;
    DrawMonoid *draw_monoids;
    uint32_t *info_bin_data;
    Clip *clip_inp;
    Bbox4 *clip_bboxes;
    Bbox4 *draw_bboxes;
    BinHeader *bin_headers;
    Path *paths;
    Tile *tiles;
    SegmentCount *seg_counts;
    Segment *segments;
    uint32_t *ptcl;
    uint32_t *blend_spill;
    CoarseEl *coarse_el;     // coarse: one record per draw object (k_coarse_prep)
    uint32_t *tile_bits;     // coarse: three bits per tile of the pool (segments present / backdrop zero / backdrop even), a word per 8 tiles
    uint32_t *tile_order;    // coarse -> fine: [bucket][n_tiles] tile indices, filled up to control->work_count[bucket]
    SliceItem *slice_items;  // coarse -> fine: the slices of the long tiles (MSAA modes), slice_cap entries
    uint32_t *slice_counters;  // per first item: slices of the tile that have finished
    uint32_t *cov;           // fine: coverage scratch of the sliced tiles, cov_cap words
    uint32_t slice_cap, cov_cap;
    uint32_t slice_fills, slice_min_fills;  // 0 / 0: no slicing (area AA)
    uint32_t *clip_stack;  // clip_scratch_words(n_clips): scratch of the partitioned clip kernels / spill area of the sequential one
    uint8_t *output;
    size_t out_stride;
    const uint32_t *ramps;
    uint32_t n_ramps;
    const uint32_t *atlas;  // RGBA8 image atlas (render.rs:160-203), atlas_w x atlas_h texels
    uint32_t atlas_w, atlas_h;
    uint32_t stroke_kernel_min_lines;  // flatten: stroked lines from which stroke workgroups take them (FLATTEN_STROKE_KERNEL_MIN_LINES; 0 with VELLO_HIP_DEBUG_STROKE_KERNEL)
    bool path_count_small;  // path_count: chunks of 256 lines (PATH_COUNT_SMALL_MAX_LINES)
    bool flatten_side_by_side;  // flatten: stroke workgroups in the heavy list's launch (one frame in flight) instead of a kernel before it
    bool launch_stroke_kernel;  // false when an earlier frame of the same scene showed that stroke workgroups would exit at once
    bool flatten_coop;          // flatten's heavy list by the kernels of the wave-cooperative walk (flatten_walk.inc) instead of round 4's
    bool sequential_clip;  // VELLO_HIP_DEBUG_SEQ_CLIP: the one-wave stack machine whatever the clip count
    bool no_cull;  // VELLO_HIP_DEBUG_NO_CULL: coarse emits every draw, as the reference does (exact PTCL / segment diffs)
    bool viewport_cull;  // vello_hip_set_viewport_cull: flatten leaves lines off the target's top, bottom and right out of the soup (flatten.hip)
    // vello_hip_set_damage_rect: R, the caller's rectangle cut to this frame's target (pixels, half open); the whole target when the
    // option is off.  k_coarse builds lists for the tiles that meet R only (damage_window), k_fine stores R's pixels only; every
    // stage ahead of coarse is the whole frame's.  damaged: R is smaller than the target.
    PixelRect damage;
    bool damaged;
    // vello_hip_set_base_image: the frame's base image (null: none -- every pixel starts from cfg.base_color), one premultiplied
    // RGBA8 word per pixel, pixel (x, y) at base_image + y * base_stride + 4 * x; it may be the target.  k_fine_base reads R's words
    // of it; nothing ahead of fine learns about it.  base_event (nullable): what the frame's k_fine waits for -- the caller's
    // src_stream as it stood when the image was set; base_stream (nullable): that stream, which waits for the frame's fine through
    // base_mark.  All by value: frames in flight keep what they were enqueued with.
    const uint8_t *base_image;
    uint32_t base_stride;
    hipEvent_t base_event, base_mark;
    hipStream_t base_stream;
    bool brushes;  // the scene has gradient / image / blurred-rect draw objects (selects fine's specialisation)
    const uint32_t *mask_lut8;
    const uint32_t *mask_lut16;
    uint32_t zero_bytes;     // the lane's zero region: Control + both look-back states (k_front clears it itself)
    // A frame of an indexed scene (SceneIndex, ctx.h): tag_monoids is the index's array, the frame begins with k_frame_begin in the
    // place of the zero fill and the pathtag scan, the light pass walks the index's fill list and the stroke workgroups and the
    // heavy code read sections 1 and 2 from the index (index_lists laid out as heavy_list is: section s from word s * n_tags).
    bool indexed;
    const PathBbox *index_bboxes;  // [n_paths] the cleared boxes with the draw_flags / trans_ix the scan stores
    const uint32_t *index_lists;   // [3][n_tags]: fill segment tags | stroked tags that are not lines | stroked lines
    uint32_t index_n_fill, index_n_strokes, index_n_lines;
    uint32_t index_failed;         // the scan's verdict: 0 or FAILED_SCENE
    uint32_t *front_sync;    // k_front's grid-barrier counter (per lane; only ever grows)
    Bump *bump() const { return &control->bump; }
};

// the Config of the kernels that read transforms (flatten's, the draw stage's): the frame's, with the transform words' base -- and
// the draw-data words' base, which the draw stage reads through the same Config (an unpainted frame's: the scene's own), and the
// path-data words' base, which flatten reads through it (an unmorphed frame's: the scene's own), and the style words' base, which
// flatten reads through it (a frame's without a stroke scale: the scene's own)
inline Config xf_config(const Frame &f) {
    Config c = f.cfg;
    c.layout.transform_base = f.xf_base;
    c.layout.draw_data_base = f.dd_base;
    c.layout.path_data_base = f.pd_base;
    c.layout.style_base = f.st_base;
    return c;
}
// whether the frame's path-data words are the lane's copy (a morphed frame, or vello_hip_run_stages after one)
inline bool morphed(const Frame &f) { return f.pd_base != f.cfg.layout.path_data_base; }
// whether the frame's style words are the lane's copy (a frame with a stroke scale)
inline bool styled(const Frame &f) { return f.st_base != f.cfg.layout.style_base; }
// the Config of k_coarse_prep, which reads draw data and no transforms: the frame's, with the draw-data words' base
inline Config dd_config(const Frame &f) {
    Config c = f.cfg;
    c.layout.draw_data_base = f.dd_base;
    return c;
}
// k_view_transforms (scene_ops.hip): fills the frame's composed transform words; launched at the head of a frame that has a view
void launch_view_transforms(const Frame &f, hipStream_t s);
// k_instance_transforms (scene_ops.hip): what it is handed by value.  Slot 0 of `out` is the six words below the retained scene's
// transform stream, slots 1 .. n_xf are X_owner(e).T_e, with View in front when has_view is set: the frame's composed transform words.
struct InstanceXfArgs {
    const uint32_t *scene;   // the retained scene: its transform entries are the library's, verbatim
    const uint32_t *owner;   // [n_xf] the instance that owns each transform entry (non-decreasing)
    const uint32_t *poses;   // [n][6] this frame's poses, 4-byte aligned
    uint32_t *out;           // slot 0 of the lane's copy
    uint32_t *failed;        // nullable: &control->bump.failed, ORed with FAILED_SCENE when a pose holds a NaN or an infinity
    uint32_t transform_base, n_xf, n;
    uint32_t has_view;
    Xform view;
};
// fills the composed transform words of a retained frame; check_poses: the frame's control block has been cleared on `s` and the
// pathtag scan has not been enqueued yet
void launch_instance_transforms(const Frame &f, bool check_poses, hipStream_t s);
// k_instance_paints (scene_ops.hip): what it is handed by value.  Word w of `out` is the retained scene's draw-data word w, or the
// rgba of this frame's paint of the instance that owns it where the word is a colour word and that paint is SOLID: the frame's
// draw-data words.
//   map: [n_words] owner | is_colour_word << 31 per draw-data word of the retained scene (n <= 2^32 / 6 instances: bit 31 is free);
//        owners do not decrease along the stream.
constexpr uint32_t DD_MAP_COLOUR = 0x80000000u;
struct InstancePaintArgs {
    const uint32_t *scene;   // the retained scene: its colour words are the ones the list was retained with
    const uint32_t *map;     // [n_words]
    const uint32_t *paints;  // [n][2] this frame's (flags, rgba), 4-byte aligned
    uint32_t *out;           // word 0 of the lane's copy
    uint32_t *failed;        // nullable: &control->bump.failed, ORed with FAILED_SCENE when a paint's flags are neither KEEP nor SOLID
    uint32_t draw_data_base, n_words, n;
};
// fills the draw-data words of a painted retained frame (Frame::paint_words is set); check_paints: the frame's control block has
// been cleared on `s` and the pathtag scan has not been enqueued yet
void launch_instance_paints(const Frame &f, bool check_paints, hipStream_t s);
// k_path_blend (scene_ops.hip): what it is handed by value.  Word i of `out` is a[i] (PATH_BLEND_COPY_A), b[i] (PATH_BLEND_COPY_B) or
// fl(a[i] + fl(t * fl(b[i] - a[i]))) (PATH_BLEND_MIX): rule 2 of vello_hip_render_resident_morphed.  The host picks the mode -- the
// verbatim cases read ONE stream -- and the access width: 16-byte accesses when every address the mode touches is 16-byte aligned,
// dword accesses otherwise (launch_path_blend).
//   PATH_BLEND_VEC_WORDS  words a workgroup takes per grid step in the 16-byte form (256 lanes x 4 words)
constexpr uint32_t PATH_BLEND_COPY_A = 0u, PATH_BLEND_COPY_B = 1u, PATH_BLEND_MIX = 2u;
constexpr uint32_t PATH_BLEND_VEC_WORDS = 1024u, PATH_BLEND_MAX_WGS = 2048u;
struct PathBlendArgs {
    const uint32_t *a, *b;  // the two sources, n words each, 4-byte aligned (the one a copy mode does not name is not read)
    uint32_t *out;          // word 0 of the lane's copy
    uint32_t n;
    uint32_t mode;          // PATH_BLEND_*
    float t;
};
// fills the path-data words of a morphed frame (Frame::pd_a is set)
void launch_path_blend(const Frame &f, hipStream_t s);
// k_style_widths (scene_ops.hip): what it is handed by value.  Entry e of `out` is the scene's style entry e -- (flags, width) --
// with the flags verbatim and the width w replaced by max(fl(w * scale), min_width) iff the entry is a stroke
// (flags & STYLE_FLAGS_STYLE) and w > 0; every other width is a bit copy (rule 1 of vello_hip_set_stroke_scale).  The two words in
// front of `out` are slot -1: the two words below the scene's stream verbatim (zeros when the scene has no two words there).  The
// host picks the access width: 8-byte accesses when stream and copy are both 8-byte aligned, dword accesses otherwise
// (launch_style_widths).
struct StyleWidthArgs {
    const uint32_t *scene;  // the frame's scene: uploaded, composed or retained
    uint32_t *out;          // entry 0 of the lane's copy (slot -1 lies two words in front)
    uint32_t style_base, n_styles;
    float scale, min_width;
};
// fills the style words of a frame with a stroke scale (Frame::has_stroke)
void launch_style_widths(const Frame &f, hipStream_t s);

void launch_pathtag_scan(const Frame &f, hipStream_t s);
// k_frame_begin (scan.hip), an indexed frame's first launch: the zero fill of the lane's zero region, the path boxes from the
// index's template, control->heavy_count[1] / [2] and bump.failed from the index
void launch_frame_begin(const Frame &f, hipStream_t s);
// k_scene_index_lists (flatten.hip), once per upload: sorts the segment tags of a scanned scene (f.tag_monoids, f.control hold the
// scan's output and verdict) into `lists` ([3][n_tags], Frame::index_lists) and counts them in counts[0 .. 2] (zeroed by the caller)
void launch_scene_index_lists(const Frame &f, uint32_t *lists, uint32_t *counts, hipStream_t s);
// (mid: when not null, an event is recorded behind every kernel of the stage but the last: per-KERNEL times of a stage of
// several kernels, vello_hip_get_kernel_ms)
// with_draw_scan: the draw stage's workgroups ride in k_flatten_light's launch (the caller then leaves launch_draw_scan out)
// light_done: k_front has run the light pass (and the draw stage's workgroups) already
void launch_flatten(const Frame &f, hipStream_t s, hipEvent_t *mid = nullptr, bool with_draw_scan = false, bool light_done = false);
// Small scenes: the workgroups of consecutive stages as ONE launch (k_front, flatten.hip).  `stages`: FRONT_* bits, consecutive stages;
// returns what the launch adds to *f.front_sync (the caller keeps the counter's value: sync_base is the value before the launch).
constexpr uint32_t FRONT_ZERO = 1u, FRONT_PATHTAG = 2u, FRONT_LIGHT = 4u, FRONT_HEAVY = 8u, FRONT_BINNING = 16u, FRONT_TILE_ALLOC = 32u;
// (a turn per workgroup and stage at most -- FRONT_MAX_WG, flatten.hip: 16 light-pass blocks of 1 024 tags, 16 blocks of 256 draw objects; a
// scene of 2 000 paths with twice these is 1 % slower one frame at a time and 4 % with four in flight when its stages share launches,
// the scenes below gain 1-10 % and 3-50 %: profiles/r05_small_scene_latency.jsonl)
constexpr uint32_t FRONT_MAX_TAGS = 16384u, FRONT_MAX_DRAW_OBJECTS = 4096u;
constexpr uint32_t FRONT_TINY_SEGMENTS = 64u;  // up to here the heavy list joins the launch, which is then ONE workgroup
uint32_t launch_front(const Frame &f, hipStream_t s, uint32_t stages, bool with_draw_scan, uint32_t sync_base);
// The most segments a scene of this layout (Layout or vello_hip_layout) and tag-word count can hold
template <class L>
inline uint32_t flatten_n_seg_max(const L &layout, uint32_t n_tag_words) {
    // (a segment owns at least one word of path data, so the path-data stream bounds the segments even though the tag stream is padded)
    const uint64_t n_tags = (uint64_t)n_tag_words * 4u, n_data = layout.draw_tag_base - layout.path_data_base;
    return (uint32_t)(n_tags < n_data ? n_tags : n_data);
}
inline uint32_t flatten_n_seg_max(const Frame &f) { return flatten_n_seg_max(f.cfg.layout, f.n_tag_words); }
void launch_draw_scan(const Frame &f, hipStream_t s);
void launch_clip(const Frame &f, hipStream_t s);             // clip.hip
void launch_clip_sequential(const Frame &f, hipStream_t s);  // draw.hip
void launch_binning(const Frame &f, hipStream_t s);
void launch_tile_alloc(const Frame &f, hipStream_t s);
void launch_binning_tile_alloc(const Frame &f, hipStream_t s);
void launch_path_count(const Frame &f, hipStream_t s);
void launch_backdrop(const Frame &f, hipStream_t s);
void launch_coarse(const Frame &f, hipStream_t s, hipEvent_t *mid = nullptr);
// k_coarse_damage (coarse_damage.hip): k_coarse for a frame whose damage rectangle is smaller than its target, over the bins that meet
// its tile window; launch_coarse hands such frames on.  enable_coarse_damage_lds: its share of enable_coarse_lds.
void launch_coarse_damage(const Frame &f, hipStream_t s, uint32_t n_wg, TileRect win);
int enable_coarse_damage_lds();
int enable_coarse_lds();  // hipError_t of the per-device dynamic-LDS opt-in
void launch_path_tiling(const Frame &f, hipStream_t s);
void launch_fine(const Frame &f, hipStream_t s);
// k_fine_damage (fine_damage.hip): fine for a frame whose damage rectangle is smaller than its target; launch_fine hands such frames on
void launch_fine_damage(const Frame &f, hipStream_t s);
// k_fine_base (fine_base.hip): fine for a frame over a base image (Frame::base_image), damage rectangle or none; launch_fine hands such
// frames on
void launch_fine_base(const Frame &f, hipStream_t s);
// Test seam (vello_hip_stage_constant, seams.hip): the sizes that are named beside the kernels they belong to
uint32_t coarse_batch_draws();          // coarse.hip NB: draw objects per batch of a bin's list
uint32_t coarse_grid_bins();            // coarse.hip: k_coarse's grid holds a multiple of this many bins
uint32_t path_count_chunk(int form);    // path.hip: lines per chunk -- 0: soup size unknown, one frame in flight; 1: small soup; 2: frames in flight
uint32_t path_tiling_workgroup();       // path.hip: SegmentCounts per workgroup and turn
uint32_t backdrop_block_tiles();        // path.hip BACKDROP_BLOCK_TILES
uint32_t fine_window_words();           // fine.hip: command words k_fine reads at a time, a lane each
uint32_t fine_batch_fills();            // fine.hip MS_BATCH_FILLS: fills a batch holds at most
uint32_t fine_batch_segments();         // fine.hip: segments the fills of a batch hold at most (one 64-lane load)
uint32_t fine_item_cap();               // fine.hip MS_ITEM_CAP: crossing records a batch holds at most
uint32_t fine_simple_records();         // fine.hip: the most records of a fill that ms_fill_simple takes
uint32_t fine_prefetch_reach();         // fine.hip: words behind a prefetched window's base at which the list may resume for it to be used

// Device-to-atlas copies (vello_hip_copy_images_device, atlas.hip; k_atlas_copy, scene_ops.hip): one rectangle of raw RGBA8 words per entry.  `first` is
// the exclusive prefix of width * height over the batch, so the batch is one concatenated texel space that k_atlas_copy
// cuts into equal chunks whatever the rectangles' sizes.  Zero-sized rectangles are left out of the table by the host.
struct AtlasCopyDesc {
    uint64_t src;         // device address of the source's first texel
    uint64_t src_stride;  // bytes between source rows (a multiple of 4)
    uint64_t dst;         // atlas texel index of the destination's first texel: y * atlas_w + x
    uint64_t first;       // texels of the entries before this one
    uint32_t width, height;
};
static_assert(sizeof(AtlasCopyDesc) == 40, "AtlasCopyDesc");
// `descs`: n entries in device memory, `total` = the last entry's first + its texels (> 0)
void launch_atlas_copy(const AtlasCopyDesc *descs, uint32_t n, uint64_t total, uint32_t *atlas, uint32_t atlas_w, hipStream_t s);

// Scene instances (vello_hip_render_instances, scenes.hip; k_compose_scene, scene_ops.hip): what k_compose_scene is handed by value.  Streams are numbered in the order
// the packed scene holds them: 0 path tags, 1 path data, 2 draw tags, 3 draw data, 4 transforms, 5 styles.  Every offset is in u32 words
// but the tag stream's, which are in bytes.
//   table: [6][n + 1] exclusive prefixes of the instances' lengths per stream -- one stream's offsets are consecutive words, so a
//          search over them reads one run of memory -- then [n] fragment indices, then [n][6] transforms, then -- a painted frame's only -- [n][2] paints (compose_table_words);
//   frags: [n_frags][6] where each fragment's range begins in the library's stream.
// The grid is cut per stream (wg_first): a workgroup's chunk of steps x 256 words lies in ONE stream, so it needs one slice of one
// prefix; the last workgroup writes the 16 words of zero slack behind the scene.
constexpr uint32_t COMPOSE_MAX_STEPS = 8u, COMPOSE_TARGET_WGS = 2048u;
struct ComposeArgs {
    const uint32_t *lib;    // the library: the resident scene
    uint32_t *dst;          // the lane's private scene slot
    const uint32_t *table;
    const uint32_t *frags;
    uint32_t n, steps;
    uint32_t src_base[6];   // the library's layout bases
    uint32_t dst_base[6];   // the composed layout's
    uint32_t len[6];        // words of each composed stream (the tag stream's with its padding)
    uint32_t wg_first[7];   // first workgroup of each stream; [6]: the slack's
    uint32_t tag_bytes;     // tags of the composed scene, without the padding
};
// What the painted form of the kernel (k_compose_scene_painted) is handed besides: a frame with a paint list
// (vello_hip_render_instances_painted).  An unpainted frame's table, arguments and kernel are what they were before there were paints.
//   paints:    [n][2] (flags, rgba), the vello_hip_paint list verbatim: the lane's table, behind the transforms;
//   frag_bits: [n_frags] where each fragment's colour-word mask begins in `masks`, in bits;
//   masks:     a bit per draw-data word of every fragment, in the order of the table, set where the word is a colour word.
constexpr uint32_t PAINT_SOLID = 1u;  // VELLO_HIP_PAINT_SOLID of include/vello_hip.h (scenes.hip holds the two to each other)
struct ComposePaintArgs {
    const uint32_t *paints;
    const uint32_t *frag_bits;
    const uint32_t *masks;
};
inline size_t compose_table_words(uint32_t n, bool painted) { return 6u * ((size_t)n + 1u) + (painted ? 9u : 7u) * (size_t)n; }
// pa == nullptr: the unpainted form
void launch_compose_scene(const ComposeArgs &a, const ComposePaintArgs *pa, hipStream_t s);

// Hit testing (vello_hip_pick, pick.hip): what k_pick_lines and k_pick_resolve are handed by value.  Everything but `winding` and
// `out` is read only: the frame's line soup, draw monoids and path boxes in its lane, the draw tags of the scene it rendered, and --
// a frame composed from instances -- the draw-tag stream's exclusive prefix ([n_inst + 1], ComposeArgs::table's third row or the
// retained list's copy of it).
//   PICK_LINES_CHUNK  lines per workgroup of k_pick_lines, a lane each;
//   PICK_DRAW_CHUNK   draw objects per step of k_pick_resolve's walk, a lane each.
// THE BATCH RULE: the queries of one call are answered in batches of pick_batch(n_paths) queries.  A batch owns a winding table of
// batch x n_paths u32 words, zero-filled on the frame's stream ahead of its two launches; the table stays within
// PICK_SCRATCH_BYTES unless ONE query's row is larger (more than 4 Mi paths), which is then a batch of one.
// VELLO_HIP_DEBUG_PICK_SMALL_BATCHES makes every batch PICK_BATCH_FORCED queries, so that a small scene spans several.
constexpr uint32_t PICK_LINES_CHUNK = 256u, PICK_DRAW_CHUNK = 256u;
constexpr uint32_t PICK_NONE = 0xffffffffu, PICK_MAX_POINTS = 4096u;
constexpr size_t PICK_SCRATCH_BYTES = (size_t)16u << 20;
constexpr uint32_t PICK_BATCH_FORCED = 3u;
inline uint32_t pick_batch(uint32_t n_paths, bool forced) {
    if (forced) return PICK_BATCH_FORCED;
    if (n_paths == 0u) return PICK_MAX_POINTS;
    const size_t fit = PICK_SCRATCH_BYTES / ((size_t)n_paths * 4u);
    return fit < 1u ? 1u : fit > PICK_MAX_POINTS ? PICK_MAX_POINTS : (uint32_t)fit;
}
struct PickArgs {
    const LineSoup *lines;
    const float *points;            // [n][2] target pixel coordinates, device memory
    uint32_t *winding;              // [nq][n_paths]
    const uint32_t *draw_tags;      // [n_draw]
    const DrawMonoid *draw_monoids;
    const PathBbox *path_bboxes;
    const uint32_t *prefix;         // nullable: the frame was not composed from instances
    uint32_t *out;                  // [n][2] (draw_ix, instance_ix)
    uint32_t n_lines, n_paths, n_draw, n_inst;
    uint32_t width, height;         // the frame's target
    uint32_t q0, nq;                // the batch: queries q0 .. q0 + nq - 1
};
void launch_pick_lines(const PickArgs &a, hipStream_t s);    // (nothing to launch for an empty soup or a scene without paths)
void launch_pick_resolve(const PickArgs &a, hipStream_t s);  // a workgroup per query of the batch

// Marquee selection (vello_hip_pick_rect, pick_rect.hip): what its four kernels are handed by value.  The frame's buffers are read
// only, as in PickArgs.  R' and C of the contract are computed on the host (region_of) and travel as arguments, so they are
// wave-uniform.  `scratch` is the context's, zero-filled on the frame's stream ahead of the launches, region_scratch_words(...) words:
//   [n_paths]   MEETS: 1 once a line of the path meets R'          (k_region_lines ORs, the draw kernels read)
//   [n_paths]   the winding of the path at C, wrapping u32         (k_region_lines adds, the draw kernels read)
//   [n_inst]    per instance: REGION_TOUCHED | REGION_ENCLOSED of any of its draws, REGION_NOT_ALL once a paint draw with a non-empty
//               path box is not ENCLOSED                           (k_region_draws ORs, k_region_instances reads)
//   [4]         vello_hip_region_counts
//   [chunks]    the clip-stack sum of each REGION_DRAW_CHUNK draws  (k_region_draw_totals writes, k_region_draws reads)
//   REGION_LINES_CHUNK  lines per workgroup of k_region_lines, a lane each;
//   REGION_DRAW_CHUNK   draw objects per workgroup of k_region_draw_totals and k_region_draws, a lane each.
constexpr uint32_t REGION_LINES_CHUNK = 256u, REGION_DRAW_CHUNK = 256u;
constexpr uint32_t REGION_TOUCHED = 1u, REGION_ENCLOSED = 2u, REGION_NOT_ALL = 4u;
struct Region {
    float x0, y0, x1, y1;  // R'
    float cx, cy;          // C
};
// rule 0 of the contract; false: R' is empty
inline bool region_of(const float rect[4], uint32_t width, uint32_t height, Region &r) {
    const float w = (float)width, h = (float)height;
    for (int k = 0; k < 4; k++)
        if (rect[k] != rect[k]) return false;
    const float xa = rect[0] < rect[2] ? rect[0] : rect[2], xb = rect[0] < rect[2] ? rect[2] : rect[0];
    const float ya = rect[1] < rect[3] ? rect[1] : rect[3], yb = rect[1] < rect[3] ? rect[3] : rect[1];
    r.x0 = xa > 0.0f ? xa : 0.0f, r.x1 = xb < w ? xb : w;
    r.y0 = ya > 0.0f ? ya : 0.0f, r.y1 = yb < h ? yb : h;
    if (!(r.x0 < r.x1 && r.y0 < r.y1)) return false;
    r.cx = r.x0 + (r.x1 - r.x0) * 0.5f;
    if (!(r.cx < r.x1)) r.cx = r.x0;
    r.cy = r.y0 + (r.y1 - r.y0) * 0.5f;
    if (!(r.cy < r.y1)) r.cy = r.y0;
    return true;
}
inline uint32_t region_draw_chunks(uint32_t n_draw) { return (uint32_t)(((uint64_t)n_draw + REGION_DRAW_CHUNK - 1u) / REGION_DRAW_CHUNK); }
inline size_t region_scratch_words(uint32_t n_paths, uint32_t n_inst, uint32_t n_draw) {
    return 2u * (size_t)n_paths + n_inst + 4u + region_draw_chunks(n_draw);
}
struct RegionArgs {
    const LineSoup *lines;
    const uint32_t *draw_tags;      // [n_draw]
    const DrawMonoid *draw_monoids;
    const PathBbox *path_bboxes;
    const uint32_t *prefix;         // nullable: the frame was not composed from instances
    uint32_t *scratch;              // the layout above
    uint32_t *draws_out;            // nullable [n_draw]
    uint32_t *instances_out;        // nullable [n_inst]
    uint32_t n_lines, n_paths, n_draw, n_inst;
    Region r;
};
void launch_region_lines(const RegionArgs &a, hipStream_t s);      // (nothing to launch for an empty soup or a scene without paths)
void launch_region_draws(const RegionArgs &a, hipStream_t s);      // the two launches of the draw pass (none for a frame without draws)
void launch_region_instances(const RegionArgs &a, hipStream_t s);  // (none for a frame without instances)

}  // namespace vk
