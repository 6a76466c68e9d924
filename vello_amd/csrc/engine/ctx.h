// The host driver's data model -- the context, its lanes, its scene slots -- and the helpers its translation units share.
// (engine.h is the interface between the driver and the kernels; this header is the driver's own.)
#pragma once
#include "../../../include/vello_hip.h"

#include <string>
#include <vector>

#include "engine.h"

namespace vk {

// A device allocation, owned by the struct that holds it: freed with it.  (vello_hip_destroy sets the device and waits for every
// stream before the context and its lanes go away.)
struct DevBuf {
    void *ptr = nullptr;
    size_t size = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : ptr(o.ptr), size(o.size) { o.ptr = nullptr, o.size = 0; }
    ~DevBuf() {
        if (ptr) (void)hipFree(ptr);
    }
};

inline uint32_t align_up(uint32_t len, uint32_t alignment) { return len + ((0u - len) & (alignment - 1u)); }

// One frame in flight = one lane: its own stream and its own set of transient buffers.  The packed scene,
// ramps and mask LUTs are shared read-only.  wgpu queues recordings without waiting (wgpu_engine.rs:757); here
// consecutive frames additionally overlap on the GPU (coarse launches only one workgroup per bin, fine and
// flatten are latency-bound, so a second frame fills the idle CUs): vello_hip_set_frames_in_flight.
// What every frame of a resident scene would compute again from the same bytes: built once by
// vello_hip_upload_scene for the shared slot, for scenes too large for k_front.  Nothing in it depends on a transform.
struct SceneIndex {
    DevBuf monoids;  // [n_tag_words + 4] the pathtag scan's output: every lane's Frame::tag_monoids
    DevBuf bboxes;   // [n_paths + 1] the cleared boxes with the draw_flags / trans_ix the scan stores at the PATH markers
    DevBuf lists;    // [3][n_tags] fill segment tags | stroked tags that are not lines | stroked lines (Frame::index_lists)
    DevBuf counts;   // [4] the lists' lengths as the build kernel counted them
    uint32_t n_fill = 0, n_strokes = 0, n_lines = 0;
    uint32_t failed = 0;  // the scan's verdict: 0 or FAILED_SCENE
    bool valid = false;   // dropped by the next upload into the slot and by a vello_hip_write_buffer to its scene
};
// A packed scene made resident: the bytes, the ramp texture and everything the host derives from the Layout.
struct SceneSlot {
    DevBuf scene, ramps;
    vello_hip_layout layout{};
    size_t scene_len = 0;
    uint32_t n_tag_words = 0, n_pathtag_parts = 0, n_draw_parts = 0, n_ramps = 0;
    size_t zero_bytes = 0;
    bool brushes = false;   // gradient / image / blurred-rect draw objects present (selects fine's specialisation)
    bool resident = false;
    // stroked-line tags of the scene as k_flatten_light counted them in an earlier frame (-1: not known yet).  A property of
    // the scene alone; lets the host leave out stroke workgroups that would exit at once.
    int64_t stroke_lines = -1;
    // lines in the soup of a finished frame of this scene (-1 unknown): picks path_count's chunk size (path.hip, k_path_count<LPT>)
    int64_t soup_lines = -1;
    int64_t slice_demand = -1;  // slice items coarse asked for in a finished MSAA frame of this scene (max seen), -1 unknown
    // what k_flatten_light put on flatten's heavy list in a finished frame of this scene: fills' curves, stroked curves (+ the cap
    // markers of open subpaths), stroked lines (-1: not known yet): picks the kernels that take the list (Frame::flatten_coop)
    int64_t heavy_curves = -1, heavy_strokes = -1;
    uint64_t generation = 0;  // bumped by every upload into the slot: a lane's finished frame speaks for the scene it rendered only
    SceneIndex index;         // the shared slot only
    // The composed transform words of frames with a view (vello_hip_set_view_transform, Frame::xf_base): `view_sets` copies of
    // (n_xf + 1) * 6 words each, from word `view_at` of the scene's allocation -- behind the scene's bytes and their slack, never
    // part of what VELLO_HIP_BUF_SCENE shows.  The shared slot holds a copy per lane (frames in flight have views of their own), a
    // lane's private slot one.
    size_t view_at = 0;
    size_t view_cap_bytes = 0;  // bytes allocated from view_at on (ensure_scene)
    uint32_t view_sets = 0, view_set_words = 0;
    // the bytes were composed from the library's fragments (vello_hip_render_instances, vello_hip_retain_instances): ramps are the
    // shared slot's
    bool composed = false;
    // The retained slot only: the draw-data words of PAINTED retained frames (vello_hip_render_retained_painted, Frame::dd_base) --
    // `dd_sets` copies (a lane each) of `dd_set_words` words, the draw-data stream's length, from word `dd_at` of the scene's
    // allocation: behind the transform copies, in the same tail (view_cap_bytes covers both).  dd_sets == 0: the slot has none
    // (every other slot; a list so large that the copies would be out of a u32 word offset's reach -- it takes no paints).
    size_t dd_at = 0;
    uint32_t dd_sets = 0, dd_set_words = 0;
    // The shared slot only: the path-data words of MORPHED frames (vello_hip_render_resident_morphed, Frame::pd_base) -- `pd_sets`
    // copies (a lane each) of `pd_set_words` words from word `pd_at` of the scene's allocation: behind the transform copies, in the
    // same tail (view_cap_bytes covers both).  A copy is the stream's length plus PD_SLACK_WORDS, rounded up to whole quads, and
    // begins on a 16-byte boundary; its slack holds the words that follow the stream in the scene, so that a read behind the
    // stream's end (flatten's look at the tag after a stroked segment) finds what it finds in the scene itself.  pd_sets == 0: no
    // room yet -- it is made once per resident scene, by vello_hip_upload_path_keyframes or the first morphed frame
    // (ensure_morph_room), not by the upload: scenes that are never morphed pay nothing.
    size_t pd_at = 0;
    uint32_t pd_sets = 0, pd_set_words = 0;
    // The style words of frames with a stroke scale (vello_hip_set_stroke_scale, Frame::st_base): `st_sets` copies of
    // (n_styles + 1) * 2 words each -- slot -1 first -- from word `st_at` of the scene's allocation: behind the transform copies, in
    // the same tail (view_cap_bytes covers both), on an even word, so that a copy is 8-byte aligned where the scene's stream is.
    // A copy per lane in the shared and the retained slot, one in a lane's private slot, as the transform copies.
    size_t st_at = 0;
    uint32_t st_sets = 0, st_set_words = 0;
    bool i16_segments = false;  // a segment tag without PATH_TAG_F32 is present (found by load_slot from the host bytes): no blends
};
constexpr uint32_t PD_SLACK_WORDS = 8u;  // (a cubic's four points: what read_path_segment reads from a tag's offset on)
// A fragment of the library as the host keeps it: where its range begins in each stream and how long it is -- in the units of
// ComposeArgs (bytes for tags, words otherwise) -- what the composed layout and fine's specialisation need of its draw tags, and
// where the mask of its colour words lies (vello_hip_render_instances_painted).
struct FragmentInfo {
    uint32_t begin[6], len[6];
    uint32_t n_clips, info_words;
    bool brushes;
    uint32_t mask_bit;  // where its colour-word mask begins in ctx::frag_masks' bit array (valid while ctx::have_masks)
};
constexpr uint32_t MAX_LANES = 8;

// Which scene a lane's latest frame reads (slot_of): the context's shared scene (vello_hip_upload_scene), the lane's private slot
// (vello_hip_render_frame, vello_hip_render_instances) or the context's retained instance list (vello_hip_retain_instances).
enum class LaneScene : uint8_t { Shared, Own, Retained };

struct Lane {
    hipStream_t stream = nullptr;
    SceneSlot own;          // vello_hip_render_frame: the scene of the frame this lane is rendering
    LaneScene which = LaneScene::Shared;
    DevBuf buf[VELLO_HIP_BUF_COUNT];  // SCENE / CONFIG / BUMP entries unused (shared, see ctx; the head of zero_region: find_buf)
    DevBuf zero_region;               // Control + look-back states
    DevBuf clip_stack;
    DevBuf coarse_el;                 // coarse: CoarseEl per draw object
    DevBuf tile_bits;                 // coarse: 3 bits per tile of the pool, a word per 8 tiles
    DevBuf tile_order;                // coarse -> fine: tiles bucketed by command-list length
    DevBuf slice_items, slice_counters, cov;  // coarse -> fine: slices of long tiles, their arrival counters, coverage scratch
    DevBuf heavy_list;                // flatten: tag indices for the heavy code, 4 lists (one u32 per tag each, worst case)
    DevBuf arc_items;                 // flatten: arcs the stroke workgroups leave to the heavy code (64 B per segment, worst case)
    DevBuf compose_table;             // vello_hip_render_instances: the frame's ComposeArgs::table (+ ComposePaintArgs::paints)
    uint32_t compose_n = 0;           // ... and its instance count: vello_hip_pick finds the owner of a draw in the table's draw-tag prefix
    Config frame_cfg{};               // the Config of the lane's latest frame (prepare_frame): what vello_hip_pick answers against
    // vello_hip_render_retained: the frame's poses when they came from the host (n x 6 words, copied on the lane's stream) ...
    DevBuf poses;
    // ... and where the frame's k_instance_transforms reads them: `poses`, the caller's device memory, or null for the rest poses
    const uint32_t *pose_src = nullptr;
    hipStream_t pose_stream = nullptr;  // the caller's stream that waits for that kernel (null: none)
    bool pose_check = false;            // the caller's device memory: the host has not seen the poses, the kernel tests them
    // (all three belong to the frame being entered: vello_hip_render_retained clears them before it returns, so that no later
    // frame of the lane reads the caller's memory or stream again)
    // ctx::retained.generation of the list whose composed transform words the lane's copy holds (0: none): vello_hip_run_stages
    // after a retained frame goes on from them
    uint64_t posed_generation = 0;
    // vello_hip_render_retained_painted: the frame's paints when they came from the host (n x 2 words, copied on the lane's stream) ...
    DevBuf paints;
    // ... and where the frame's k_instance_paints reads them: `paints`, the caller's device memory, or null for an unpainted frame
    const uint32_t *paint_src = nullptr;
    bool paint_check = false;           // the caller's device memory: the host has not seen the paints, the kernel tests their flags
    // (both belong to the frame being entered and are cleared with the pose source)
    // ctx::retained.generation of the list whose painted draw-data words the lane's copy holds BECAUSE the lane's latest retained
    // frame was a painted one (0: it was not): vello_hip_run_stages after a painted frame goes on from them
    uint64_t painted_generation = 0;
    // vello_hip_render_resident_morphed: where the frame's k_path_blend reads its two sources (the shared scene's stream, the
    // context's keyframes or the caller's device memory; pd_a null: not a morphed frame), its mode and t, and the caller's stream
    // that waits for it (null: none).  They belong to the frame being entered and are cleared before the entry point returns.
    const uint32_t *pd_a = nullptr, *pd_b = nullptr;
    uint32_t pd_mode = 0;
    float pd_t = 0.0f;
    hipStream_t pd_stream = nullptr;
    // ctx::shared.generation of the scene whose morphed path-data words the lane's copy holds BECAUSE the lane's latest frame of the
    // shared scene was a morphed one (0: it was not): vello_hip_run_stages after a morphed frame goes on from them
    uint64_t morphed_generation = 0;
    DevBuf front_sync;               // k_front's grid-barrier counter (zeroed once, when allocated)
    uint32_t front_sync_value = 0;    // ... and its value once every launch enqueued so far has run
    struct EvPair {
        int stage;
        hipEvent_t a, b;
        hipEvent_t mid[2];  // behind the stage's first / second kernel when it has more than one (flatten: 3, coarse: 2)
    };
    std::vector<EvPair> events;
    // hands the lane's events back to the context's pool (which vello_hip_destroy destroys)
    void return_events(std::vector<hipEvent_t> &pool) {
        for (auto &ev : events)
            for (hipEvent_t e : {ev.a, ev.b, ev.mid[0], ev.mid[1]})
                if (e) pool.push_back(e);
        events.clear();
    }
    bool used = false;
    bool slices_on = false;   // the lane's latest frame ran with fine's slices enabled (an MSAA frame)
    bool frame_damaged = false;  // the lane's latest frame drew less than its target (Frame::damaged): its slice count is not the scene's
    uint32_t slice_cap_coarse = 0;  // slice blocks the lane's latest COARSE launch was told of (a later FINE must launch as many)
    uint32_t slice_fills_coarse = 0;  // ... and the slice size it cut with (0: no slices -- an area-AA frame)
    bool frame_indexed = false;  // the lane's latest frame read the shared slot's index (VELLO_HIP_BUF_TAG_MONOIDS shows its array)
    bool flatten_ran = false;  // the control block holds flatten's counts (a partial vello_hip_run_stages range may stop before it)
    uint64_t frame_generation = 0;  // slot_of(...).generation when the lane's latest frame was set up
    uint64_t atlas_epoch_seen = 0;  // ctx::atlas_epoch the lane's stream has been ordered behind
};

// Pinned staging block of one vello_hip_write_image: the caller's pixels are copied here during the call, the DMA into the
// atlas runs from it on the upload stream; free again once `done` has passed.
struct Staging {
    void *host = nullptr;
    size_t size = 0;
    hipEvent_t done = nullptr;
    bool busy = false;
    Staging() = default;
    Staging(Staging &&o) noexcept : host(o.host), size(o.size), done(o.done), busy(o.busy) { o.host = nullptr, o.done = nullptr; }
    ~Staging() {
        if (host) (void)hipHostFree(host);
        if (done) (void)hipEventDestroy(done);
    }
};

}  // namespace vk

struct vello_hip_ctx {
    int device = 0;
    uint32_t aa_mask = 0;
    vello_hip_capacities caps{};
    vk::DevBuf config;
    vk::DevBuf mask8, mask16;
    vk::SceneSlot shared;  // vello_hip_upload_scene: one scene for every lane
    // vello_hip_upload_path_keyframes: n_keys alternative path-data streams of the shared scene, keyframe k at word
    // k * key_stride -- the stream's length rounded up to whole quads: every keyframe is 16-byte aligned (dropped by every upload
    // into the shared slot; the buffer stays for the next set)
    vk::DevBuf keyframes;
    uint32_t n_keys = 0, key_stride = 0;
    // vello_hip_upload_fragments: the shared scene as a library of fragments (dropped by the next vello_hip_upload_scene)
    std::vector<vk::FragmentInfo> fragments;
    bool have_fragments = false;
    vk::DevBuf frag_table;  // ComposeArgs::frags
    // the fragments' colour-word masks: [n_frags] bit offsets (ComposePaintArgs::frag_bits), then the bit array (::masks), a bit
    // per draw-data word of every fragment in the table's order.  Not kept (have_masks false) for a table whose draw-data ranges
    // add up to 2^32 words or more: such a library takes no paints.
    vk::DevBuf frag_masks;
    bool have_masks = false;
    // ... and the host's copy of the bit array (FragmentInfo::mask_bit indexes it): vello_hip_retain_instances builds the list's
    // per-word table from it
    std::vector<uint32_t> frag_masks_host;
    // vello_hip_retain_instances: the composed scene of ONE instance list, kept across frames (transform entries: the library's,
    // verbatim; a transform copy per lane behind its bytes, as the shared slot has), the instance that owns each transform entry
    // ([n_xf] u32) and the rest poses ([n][6] f32).  Dropped with the fragment table.
    vk::SceneSlot retained;
    vk::DevBuf retained_owner, retained_rest;
    vk::DevBuf retained_prefix;  // [n + 1] the list's draw-tag prefix (ComposeArgs::table's third row): vello_hip_pick's owner search
    // [draw-data words] owner | colour word << 31 (InstancePaintArgs::map): what k_instance_paints reads.  Built with the list when
    // the library keeps masks (have_masks); a list of a library without them takes no paints.
    vk::DevBuf retained_ddmap;
    uint32_t retained_n = 0;
    bool have_retained = false;
    hipEvent_t pose_mark = nullptr;  // orders a retained frame's pose kernel, and vello_hip_pick's read of device points, against the caller's src_stream
    vk::DevBuf atlas;  // persistent image atlas (render.rs:160-176), shared by all lanes
    uint32_t atlas_w = 0, atlas_h = 0;
    std::vector<vk::Lane> lanes;
    // The lanes' streams have ONE stream priority that is not the default's when the device has a range: the runtime keeps a pool of
    // hardware queues per priority, so the lanes do not share queues with the null stream or the caller's streams.
    // Chosen once by vello_hip_create; false: hipStreamCreateWithFlags (no range, a failed creation, VELLO_HIP_DEBUG_LANE_QUEUES=default)
    bool lane_own_pool = false;
    int lane_priority = 0;
    uint32_t n_active = 1;  // lanes in the rotation (<= lanes.size(): shrinking keeps the buffers)
    uint32_t next_lane = 0, last_lane = 0;
    bool auto_grow = false;
    bool viewport_cull = false;  // vello_hip_set_viewport_cull: copied into every Frame when it is prepared
    bool has_view = false;       // vello_hip_set_view_transform: likewise
    vk::Xform view{1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};
    bool has_stroke = false;     // vello_hip_set_stroke_scale: likewise
    float stroke_scale = 1.0f, stroke_min = 0.0f;
    bool has_damage = false;     // vello_hip_set_damage_rect: likewise; cut to the frame's target by prepare_frame (Frame::damage)
    uint32_t damage[4] = {0u, 0u, 0u, 0u};  // x0 y0 x1 y1 as the caller gave them (x0 <= x1, y0 <= y1)
    // vello_hip_set_base_image: likewise (Frame::base_image ...).  base_stride 0: width * 4 of the frame.  base_stream: the caller's
    // src_stream (null: none); base_ready was recorded on it during the call and is what the frames' k_fine wait for (recorded again
    // by the next call: a wait already enqueued keeps the record it was enqueued against); base_mark carries a frame's fine back
    // to base_stream.  base_checked: bytes from base_image on that are known to lie in one allocation of the context's device
    // (0: not asked yet) -- one runtime query per setting and size, not per frame.
    const uint8_t *base_image = nullptr;
    size_t base_stride = 0;
    hipStream_t base_stream = nullptr;
    hipEvent_t base_ready = nullptr, base_mark = nullptr;
    uint64_t base_checked = 0;
    hipStream_t copy_stream = nullptr;  // vello_hip_gather_frames: this context's peer copy
    hipEvent_t frame_done = nullptr;
    // vello_hip_write_image: atlas uploads are stream-ordered, not host-synchronous (wgpu's queue.write_texture is queued
    // too, render.rs:160-203).  An upload waits for the frames enqueued before it (they may sample the texels it replaces)
    // and every frame enqueued after it waits for `atlas_ready`.
    hipStream_t upload_stream = nullptr;
    hipEvent_t atlas_ready = nullptr, lane_mark = nullptr;
    uint64_t atlas_epoch = 0;  // uploads enqueued so far
    std::vector<vk::Staging> staging;
    vk::DevBuf copy_descs;  // vello_hip_copy_images_device: the batch's AtlasCopyDesc table (written and read on the upload stream only)
    // vello_hip_pick (blocking: idle between calls): a batch's winding table, host points on their way in, a host result on its way out
    vk::DevBuf pick_winding, pick_points, pick_out;
    float pick_ms = 0.f;  // device time of the last pick's (or pick_rect's) launches, taken while profiling is on (vello_hip_pick_ms)
    // vello_hip_pick_rect (blocking too): RegionArgs::scratch, and host outputs on their way out ([n_draw] + [n_inst] words)
    vk::DevBuf region_scratch, region_out;
    uint32_t debug_flags = 0;  // VELLO_HIP_DEBUG_*
    bool force_brushes = false;  // pre-warm: run fine's brush specialisation on a scene without brushes
    uint32_t last_render_attempts = 0;  // rounds the last vello_hip_render needed (robust mode)
    uint64_t fused_launches = 0;  // k_front launches so far (vello_hip_fused_launches)
    uint64_t scene_allocations = 0;  // scene buffers allocated so far (vello_hip_scene_allocations)
    uint64_t scene_index_builds = 0;  // scene indexes built so far (vello_hip_scene_index_builds)
    // last frame
    vk::Config cfg{};
    bool have_cfg = false;
    bool cfg_unsent = false;  // `cfg` is newer than the device copy (vello_hip_render_instances): sent when VELLO_HIP_BUF_CONFIG is next touched
    // profiling
    uint32_t prof_mask = 0;
    std::vector<hipEvent_t> event_pool;
    float stage_ms[VELLO_HIP_STAGE_COUNT] = {};
    uint32_t stage_count[VELLO_HIP_STAGE_COUNT] = {};
    float kernel_ms[VELLO_HIP_STAGE_COUNT][3] = {};  // per kernel of the stages that are several (flatten, coarse)
    uint32_t kernel_count[VELLO_HIP_STAGE_COUNT] = {};
    std::string last_error;
};

namespace vk {

#define HIP_TRY(ctx, expr)                                                                             \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
            return VELLO_HIP_E_HIP;                                                                    \
        }                                                                                              \
    } while (0)

inline SceneSlot &slot_of(vello_hip_ctx *c, Lane &l) {
    return l.which == LaneScene::Own ? l.own : l.which == LaneScene::Retained ? c->retained : c->shared;
}
// bytes between the rows of a target
inline size_t row_stride(const vello_hip_render_params *p, size_t out_stride) { return out_stride ? out_stride : (size_t)p->width * 4u; }

// context.hip
int ensure(vello_hip_ctx *c, DevBuf &b, size_t bytes);
int sync_all(vello_hip_ctx *c);
uint32_t cov_cap_words(const vello_hip_capacities &d, uint32_t aa_mask);
int commit_caps(vello_hip_ctx *c, const vello_hip_capacities &d);
int presize_pools(vello_hip_ctx *c, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout, const vello_hip_render_params *params);
int alloc_lane_scene(vello_hip_ctx *c, Lane &l, const SceneSlot &sc);
// frames.hip
int check_target(vello_hip_ctx *c, const vello_hip_render_params *p, const void *out, size_t out_stride, bool device);
int check_base_image(vello_hip_ctx *c, const vello_hip_render_params *p, const void *out, size_t out_stride);
int view_base(vello_hip_ctx *c, const SceneSlot &sc, const Lane &l, uint32_t &base);
int paint_base(vello_hip_ctx *c, const SceneSlot &sc, const Lane &l, uint32_t &base);
int morph_base(vello_hip_ctx *c, const SceneSlot &sc, const Lane &l, uint32_t &base);
int style_base(vello_hip_ctx *c, const SceneSlot &sc, const Lane &l, uint32_t &base);
int prepare_frame(vello_hip_ctx *c, Lane &l, const vello_hip_render_params *p, void *out_device, size_t out_stride, Frame &f, bool upload_cfg);
int run_stage_range(vello_hip_ctx *c, Lane &l, const Frame &f_in, int first, int last);
// scenes.hip
int load_slot(vello_hip_ctx *c, SceneSlot &sc, hipStream_t st, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
              const uint32_t *ramps, uint32_t n_ramps);
void drop_retained(vello_hip_ctx *c);
int ensure_morph_room(vello_hip_ctx *c);
// atlas.hip
int acquire_staging(vello_hip_ctx *c, size_t bytes, Staging *&out);
// seams.hip
hipEvent_t get_event(vello_hip_ctx *c);
// pick.hip: what the queries on the frame submitted last share (vello_hip_pick, vello_hip_pick_rect)
struct QueryFrame {
    Lane *lane;
    const SceneSlot *scene;
    const uint32_t *prefix;  // null: the frame was not composed from instances
    uint32_t n_inst;
};
const char *not_device_memory(vello_hip_ctx *c, const void *p, size_t bytes);
const char *query_frame(vello_hip_ctx *c, QueryFrame &q);
int judge_frame(vello_hip_ctx *c, const char *who, Lane &l, Bump &bump);

// One step of enter_frame that an entry point has nothing to add to.
constexpr auto no_step = [](Lane &) { return 0; };

// How vello_hip_render_frame, vello_hip_render_instances, vello_hip_render_retained and vello_hip_render_resident enqueue a frame on the next lane of the
// rotation; each hands in what it does differently:
//   set_up(l, new_scene)   waits for the lane where it must and gives it its scene slot (l.which); new_scene = false where the
//                          lane's scene-dependent buffers already fit the slot
//   rotate_first           the rotation moves before prepare_frame (a frame that prepare_frame refuses has then moved it) or only
//                          once prepare_frame has accepted the frame
//   staged(l)              what else may refuse the frame, asked after the view's pre-check and before prepare_frame
//   enqueue(l)             what the lane's stream gets ahead of the stages
// The view's pre-check (view_base) comes before the rotation moves, for the slot the frame will read -- not for a shared slot that
// holds no scene: prepare_frame refuses that frame itself.  The stroke scale's (style_base) likewise.  A composed slot whose frame
// prepare_frame refuses holds no scene: its bytes were never written.
template <class SetUp, class Staged, class Enqueue>
int enter_frame(vello_hip_ctx *c, const vello_hip_render_params *params, void *out_device, size_t out_stride, bool rotate_first, int last,
                SetUp set_up, Staged staged, Enqueue enqueue) {
    HIP_TRY(c, hipSetDevice(c->device));
    // (a base image's enqueue-time rules: asked first -- a refusal leaves the lane, its slot and the rotation as they were)
    if (int br = check_base_image(c, params, out_device, out_stride)) return br;
    const uint32_t li = c->next_lane % c->n_active;
    Lane &l = c->lanes[li];
    int r;
    bool new_scene = true;
    const LaneScene was = l.which;
    if ((r = set_up(l, new_scene))) return r;
    if (new_scene && (r = alloc_lane_scene(c, l, slot_of(c, l)))) {
        // the lane is not sized for its new slot (buffers only ever grow: it still fits the one it had): the next frame of this
        // slot must see new_scene again
        l.which = was;
        return r;
    }
    uint32_t xf_base;
    // (a retained frame always reads its lane's copy, view or no view)
    if ((c->has_view || l.which == LaneScene::Retained) && (l.which != LaneScene::Shared || c->shared.resident) &&
        (r = view_base(c, slot_of(c, l), l, xf_base)))
        return r;
    // (the stroke scale's pre-check: asked for its refusal only -- prepare_frame picks the base)
    if (uint32_t probe; c->has_stroke && (l.which != LaneScene::Shared || c->shared.resident) && (r = style_base(c, slot_of(c, l), l, probe))) return r;
    if ((r = staged(l))) return r;
    const auto rotate = [&] {
        c->next_lane = (li + 1u) % c->n_active;
        c->last_lane = li;
    };
    if (rotate_first) rotate();
    Frame f;
    if ((r = prepare_frame(c, l, params, out_device, out_stride, f, false))) {
        if (l.which == LaneScene::Own && l.own.composed) l.own.resident = false;
        return r;
    }
    if (!rotate_first) rotate();
    if ((r = enqueue(l))) return r;
    return run_stage_range(c, l, f, 0, last);
}

}  // namespace vk
