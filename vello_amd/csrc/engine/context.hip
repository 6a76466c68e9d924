// The context's life and its memory: create and destroy, frames in flight, the pools' capacities and their growth, a lane's buffers.
#include <array>
#include <cstdlib>
#include <cstring>

#include "ctx.h"

using namespace vk;

namespace {

std::string g_create_error;

// words of coarse's tile bits: one per 8 tiles (three planes' bytes side by side, coarse.hip plane_window) + 2 of slack for
// the two-word windows read at the last tiles
uint32_t tile_bits_words(uint32_t tiles) { return (tiles + 63u) / 64u * 8u + 2u; }

// The pool-capacity buffers of one lane (reference sizes: config.rs:398-408): which buffer, how many elements the capacities ask
// for, and an element's bytes.  alloc_lane_pools allocates by this table and pool_bytes adds it up.
struct Pool {
    DevBuf &buf;
    size_t count, elem;
};
std::array<Pool, 9> lane_pools(Lane &l, const vello_hip_capacities &d, uint32_t aa_mask) {
    return {{{l.buf[VELLO_HIP_BUF_LINES], d.lines, sizeof(LineSoup)},
             {l.buf[VELLO_HIP_BUF_INFO_BIN_DATA], d.bin_data, 4u},
             {l.buf[VELLO_HIP_BUF_TILES], d.tiles, sizeof(Tile)},
             {l.buf[VELLO_HIP_BUF_SEG_COUNTS], d.seg_counts, sizeof(SegmentCount)},
             {l.buf[VELLO_HIP_BUF_SEGMENTS], d.segments, sizeof(Segment)},
             {l.buf[VELLO_HIP_BUF_BLEND_SPILL], d.blend_spill, 4u},
             {l.buf[VELLO_HIP_BUF_PTCL], d.ptcl, 4u},
             {l.tile_bits, tile_bits_words(d.tiles), 4u},
             {l.cov, cov_cap_words(d, aa_mask), 4u}}};
}

// What VELLO_HIP_DEBUG_LANE_QUEUES asks for (vello_hip.h, vello_hip_set_frames_in_flight)
enum class LaneQueues { Greatest, Least, Default, Unknown };
LaneQueues lane_queues_from_env() {
    const char *v = std::getenv("VELLO_HIP_DEBUG_LANE_QUEUES");
    if (!v || !*v || !std::strcmp(v, "greatest")) return LaneQueues::Greatest;
    if (!std::strcmp(v, "least")) return LaneQueues::Least;
    if (!std::strcmp(v, "default")) return LaneQueues::Default;
    return LaneQueues::Unknown;
}

// The priority of the lanes' streams (ctx::lane_own_pool, ::lane_priority).  A device without a range, or a runtime that fails the
// query, leaves the default.
void choose_lane_priority(vello_hip_ctx *c, LaneQueues want) {
    c->lane_own_pool = false;
    c->lane_priority = 0;
#ifndef VELLO_SIMT_EMU  // (the emulator has no queues)
    if (want == LaneQueues::Default) return;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    if (least == greatest) return;
    c->lane_own_pool = true;
    c->lane_priority = want == LaneQueues::Least ? least : greatest;
#endif
}

int create_lane_stream(vello_hip_ctx *c, Lane &l) {
#ifndef VELLO_SIMT_EMU
    if (c->lane_own_pool) {
        if (hipStreamCreateWithPriority(&l.stream, hipStreamNonBlocking, c->lane_priority) == hipSuccess) return 0;
        (void)hipGetLastError();  // (sticky otherwise: the next HIP_TRY would report it)
        l.stream = nullptr;
        c->lane_own_pool = false;  // the lanes still to come are created as this one is
    }
#endif
    HIP_TRY(c, hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
    return 0;
}

int alloc_lane_pools(vello_hip_ctx *c, Lane &l) {
    if (!l.stream)
        if (int r = create_lane_stream(c, l)) return r;
    for (const Pool &p : lane_pools(l, c->caps, c->aa_mask))
        if (int r = ensure(c, p.buf, p.count * p.elem)) return r;
    return 0;
}

// bytes alloc_lane_pools asks for, per lane, at capacities `d`
size_t pool_bytes(vello_hip_ctx *c, const vello_hip_capacities &d) {
    size_t bytes = 0;
    for (const Pool &p : lane_pools(c->lanes[0], d, c->aa_mask)) bytes += p.count * p.elem;
    return bytes;
}

}  // namespace

namespace vk {

int ensure(vello_hip_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 256;
    if (b.size >= bytes) return 0;
    if (b.ptr) HIP_TRY(c, hipFree(b.ptr));
    b.ptr = nullptr;
    b.size = 0;
    HIP_TRY(c, hipMalloc(&b.ptr, bytes + 256));
    b.size = bytes;
    return 0;
}

int sync_all(vello_hip_ctx *c) {
    for (auto &l : c->lanes)
        if (l.stream) HIP_TRY(c, hipStreamSynchronize(l.stream));
    return 0;
}

// fine's coverage scratch (sliced tiles): 64 words per FILL of a sliced tile.  A FILL is >= 5 command words, so 2 x the
// PTCL pool holds the fills of lists that add up to a sixth of the pool; tiles that do not fit are rendered unsliced
// (coarse only cuts what fits), so the scratch is an optimisation with a ceiling of its own -- 2^26 words, 256 MB per
// lane: it does not follow a PTCL pool grown into the gigabytes -- and a context without an MSAA mode, which never
// slices, holds none (it used to triple the PTCL footprint unconditionally).
constexpr uint32_t COV_CAP_MAX_WORDS = 1u << 26;
uint32_t cov_cap_words(const vello_hip_capacities &d, uint32_t aa_mask) {
    if ((aa_mask & (VELLO_HIP_AA_MASK_MSAA8 | VELLO_HIP_AA_MASK_MSAA16)) == 0u) return 0u;
    return d.ptcl >= COV_CAP_MAX_WORDS / 2u ? COV_CAP_MAX_WORDS : d.ptcl * 2u;
}

// Makes `d` the context's capacities, or leaves the context as it was: ensure() frees a buffer before it allocates the
// larger one, so after a failed hipMalloc the lane holds a null pool -- the old sizes are put back (they fitted before)
// and c->caps keeps describing what the lanes really hold.  Callers have drained the lanes.
int commit_caps(vello_hip_ctx *c, const vello_hip_capacities &d) {
    const vello_hip_capacities old = c->caps;
    c->caps = d;
    int r = 0;
    for (auto &l : c->lanes)
        if ((r = alloc_lane_pools(c, l))) break;
    if (!r) return 0;
    (void)hipGetLastError();
    const std::string err = c->last_error;
    c->caps = old;
    for (auto &l : c->lanes) {
        int r2 = alloc_lane_pools(c, l);
        if (r2) return r2;  // not even the old pools: nothing left to render into, the error stands
    }
    c->last_error = "growing the pools failed, capacities unchanged: " + err;
    return r;
}

// scene-dependent buffers of one lane
int alloc_lane_scene(vello_hip_ctx *c, Lane &l, const SceneSlot &sc) {
    const vello_hip_layout &L = sc.layout;
    int r;
    if ((r = ensure(c, l.zero_region, sc.zero_bytes))) return r;
    if (!l.front_sync.ptr) {
        if ((r = ensure(c, l.front_sync, 256))) return r;
        HIP_TRY(c, hipMemset(l.front_sync.ptr, 0, 256));
        HIP_TRY(c, hipStreamSynchronize(nullptr));  // (the lanes' streams do not wait for the null stream)
        l.front_sync_value = 0;
    }
    if ((r = ensure(c, l.buf[VELLO_HIP_BUF_TAG_MONOIDS], (size_t)(sc.n_tag_words + 4u) * sizeof(TagMonoid)))) return r;
    if ((r = ensure(c, l.buf[VELLO_HIP_BUF_PATH_BBOXES], (size_t)(L.n_paths + 1u) * sizeof(PathBbox)))) return r;
    if ((r = ensure(c, l.buf[VELLO_HIP_BUF_DRAW_MONOIDS], (size_t)(L.n_draw_objects + 1u) * sizeof(DrawMonoid)))) return r;
    if ((r = ensure(c, l.buf[VELLO_HIP_BUF_CLIP_INP], (size_t)(L.n_clips + 1u) * sizeof(Clip)))) return r;
    if ((r = ensure(c, l.buf[VELLO_HIP_BUF_CLIP_BBOXES], (size_t)(L.n_clips + 1u) * sizeof(Bbox4)))) return r;
    if ((r = ensure(c, l.buf[VELLO_HIP_BUF_DRAW_BBOXES], (size_t)(L.n_paths + 1u) * sizeof(Bbox4)))) return r;
    if ((r = ensure(c, l.buf[VELLO_HIP_BUF_PATHS], (size_t)(align_up(L.n_paths, 256u) + 256u) * sizeof(Path)))) return r;
    if ((r = ensure(c, l.clip_stack, clip_scratch_words(L.n_clips) * 4u))) return r;
    if ((r = ensure(c, l.coarse_el, (size_t)(L.n_draw_objects + 1u) * sizeof(CoarseEl)))) return r;
    if ((r = ensure(c, l.heavy_list, (size_t)(sc.n_tag_words + 1u) * 64u))) return r;  // 4 lists x 4 tags per word x u32
    {
        // one arc per stroked segment at most
        const uint32_t n_seg_max = flatten_n_seg_max(L, sc.n_tag_words);
        if ((r = ensure(c, l.arc_items, (size_t)(flatten_arc_shard_cap(n_seg_max, true) > flatten_arc_shard_cap(n_seg_max, false) ? flatten_arc_shard_cap(n_seg_max, true) : flatten_arc_shard_cap(n_seg_max, false)) * FLATTEN_ARC_SHARDS * 64u))) return r;
    }
    return 0;
}

// Robust mode, before the first attempt: when the scene is large against the current pools, size them from
// vello_hip_estimate_capacities (estimate.rs's counting rules on the packed scene) instead of finding the demand by
// overflowing stage after stage.  The cheap test first: every path segment yields at least one line.
int presize_pools(vello_hip_ctx *c, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                         const vello_hip_render_params *params) {
    if (!scene || !layout || !params || layout->path_tag_base > layout->path_data_base || (size_t)layout->path_data_base * 4u > scene_len)
        return VELLO_HIP_OK;  // the upload refuses it with a message
    const uint8_t *tags = scene + (size_t)layout->path_tag_base * 4u;
    const size_t n_tags = ((size_t)layout->path_data_base - layout->path_tag_base) * 4u;
    uint64_t n_seg = 0;
    for (size_t i = 0; i < n_tags; i++) n_seg += (tags[i] & 3u) != 0u;
    const uint64_t n_tiles = (uint64_t)((params->width + 15u) / 16u) * ((params->height + 15u) / 16u);
    // (the cheap test stands for content at the scale and the stroke widths it was encoded with: under a view or a stroke scale the
    // estimator is always asked)
    if (!c->has_view && !c->has_stroke && 4u * n_seg <= c->caps.lines && 8u * n_seg <= c->caps.seg_counts && 4u * n_seg + 8u * layout->n_paths <= c->caps.tiles &&
        160u * n_tiles + 16u * n_seg <= c->caps.ptcl)
        return VELLO_HIP_OK;
    vello_hip_capacities est;
    const float view[6] = {c->view.m0, c->view.m1, c->view.m2, c->view.m3, c->view.t0, c->view.t1};
    const float stroke[2] = {c->stroke_scale, c->stroke_min};
    if (vello_hip_estimate_capacities_styled(scene, scene_len, layout, params, c->has_view ? view : nullptr, c->has_stroke ? stroke : nullptr, &est) !=
        VELLO_HIP_OK)
        return VELLO_HIP_OK;
    vello_hip_capacities d = c->caps;
    bool grew = false;
    auto want = [&](uint32_t &cap, uint32_t need) {
        if (need > cap) {
            cap = need;
            grew = true;
        }
    };
    want(d.lines, est.lines);
    want(d.bin_data, est.bin_data);
    want(d.tiles, est.tiles);
    want(d.seg_counts, est.seg_counts);
    want(d.segments, est.segments);
    want(d.ptcl, est.ptcl);
    if (d.segments < d.seg_counts) d.segments = d.seg_counts;
    if (!grew) return VELLO_HIP_OK;
    // The estimate comes from caller-supplied geometry (up to 0xffff0000 elements per pool): one that the device cannot
    // hold is not an error of this frame -- the pools stay and the overflow-and-grow loop of vello_hip_render finds the
    // real demand, which is usually far below the estimator's bound.
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return VELLO_HIP_OK;
    const size_t n_lanes = c->lanes.size(), held = pool_bytes(c, c->caps) * n_lanes, asked = pool_bytes(c, d) * n_lanes;
    if (asked > held && asked - held > free_b - free_b / 8u) return VELLO_HIP_OK;
    int r = sync_all(c);
    if (r) return r;
    if (commit_caps(c, d)) c->last_error.clear();  // capacities unchanged (commit_caps), fall back to the loop
    return VELLO_HIP_OK;
}

}  // namespace vk

extern "C" {

const char *vello_hip_last_error(vello_hip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : g_create_error.c_str(); }

int vello_hip_create(int device, uint32_t aa_mask, const vello_hip_capacities *caps, vello_hip_ctx **out) {
    if (!out) return VELLO_HIP_E_INVALID;
    *out = nullptr;
    const LaneQueues lane_queues = lane_queues_from_env();
    if (lane_queues == LaneQueues::Unknown) {
        g_create_error = "VELLO_HIP_DEBUG_LANE_QUEUES is none of default, least, greatest";
        return VELLO_HIP_E_INVALID;
    }
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev) {
        g_create_error = std::string("no usable HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count=0") +
                         "); the engine has no CPU fallback";
        return VELLO_HIP_E_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_create_error = "hipSetDevice failed";
        return VELLO_HIP_E_NO_DEVICE;
    }
    // The process's FIRST hardware queue is a poor place for a lane: with four frames in flight a context whose lane 0 sits on it
    // renders 8 % fewer frames per second than one whose lanes come second to fifth (profiles/r06_queue_order.txt: 2 110 against
    // 2 300 on the road map, rocprofv3's Queue_Id per stream).  HIP hands out hardware queues in the order streams are created,
    // and creates the null stream's lazily -- so the null stream is made to take its queue here, before the lanes' streams exist
    // (a caller that has used the device before gets the same order by itself).  Lanes with a priority of their own
    // (choose_lane_priority) sit in another pool of queues altogether; this claim is what lanes of the default priority rely on.
    {
        void *scratch = nullptr;
        if (hipMalloc(&scratch, 256) == hipSuccess) {
            (void)hipMemsetAsync(scratch, 0, 256, nullptr);
            (void)hipStreamSynchronize(nullptr);
            (void)hipFree(scratch);
        }
        (void)hipGetLastError();
    }
    vello_hip_ctx *c = new vello_hip_ctx();
    c->device = device;
    c->aa_mask = aa_mask ? (aa_mask & VELLO_HIP_AA_MASK_ALL) : VELLO_HIP_AA_MASK_ALL;
    // reference pool sizes, vello_encoding/src/config.rs:398-408
    vello_hip_capacities d{1u << 21, 1u << 18, 1u << 21, 1u << 21, 1u << 21, 1u << 20, 1u << 23};
    if (caps) {
        if (caps->lines) d.lines = caps->lines;
        if (caps->bin_data) d.bin_data = caps->bin_data;
        if (caps->tiles) d.tiles = caps->tiles;
        if (caps->seg_counts) d.seg_counts = caps->seg_counts;
        if (caps->segments) d.segments = caps->segments;
        if (caps->blend_spill) d.blend_spill = caps->blend_spill;
        if (caps->ptcl) d.ptcl = caps->ptcl;
    }
    // A segment pool the caller did not size follows the seg_counts pool (a whole frame has a segment per SegmentCount record,
    // coarse.wgsl:166).  One given explicitly is kept, smaller too: a frame with a damage rectangle needs the segments of its window
    // only, and k_path_tiling fails a frame whose coarse handed out more than the pool holds.
    if (d.segments < d.seg_counts && !(caps && caps->segments)) d.segments = d.seg_counts;
    c->caps = d;
    choose_lane_priority(c, lane_queues);
    auto fail = [&](const char *what) {
        g_create_error = std::string(what) + ": " + c->last_error;
        vello_hip_destroy(c);
        return VELLO_HIP_E_HIP;
    };
    if (int le = enable_coarse_lds()) {
        c->last_error = std::string("hipFuncSetAttribute(k_coarse, MaxDynamicSharedMemorySize): ") + hipGetErrorString((hipError_t)le);
        return fail("coarse LDS opt-in");
    }
    c->lanes.resize(1);
    if (alloc_lane_pools(c, c->lanes[0])) return fail("pool allocation");
    if (ensure(c, c->config, sizeof(Config))) return fail("config");
    if (ensure(c, c->mask8, 1024) || ensure(c, c->mask16, 8192)) return fail("mask lut");
    {
        std::vector<uint8_t> l8(1024), l16(8192);
        vello_hip_make_mask_lut(l8.data());
        vello_hip_make_mask_lut_16(l16.data());
        if (hipMemcpy(c->mask8.ptr, l8.data(), 1024, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(c->mask16.ptr, l16.data(), 8192, hipMemcpyHostToDevice) != hipSuccess)
            return fail("mask lut upload");
    }
    // Pre-warm: the first launch of a kernel loads its code object and, for the kernels with a scratch segment (fine, the
    // heavy flattener), makes the runtime allocate scratch for the queue -- ~20 ms that would otherwise land in the
    // caller's first frame.  One frame of an empty scene per enabled AA mode and fine specialisation.
    {
        std::vector<uint8_t> empty(1024u * 4u, 0);  // 1024 zero tag words = 4096 padded path tags, nothing else
        vello_hip_layout lay{};
        lay.path_tag_base = 0u;
        lay.path_data_base = lay.draw_tag_base = lay.draw_data_base = lay.transform_base = lay.style_base = 1024u;
        if (vello_hip_upload_scene(c, empty.data(), empty.size(), &lay, nullptr, 0) == VELLO_HIP_OK) {
            for (uint32_t aa = 0; aa < 3u; aa++) {
                if (((c->aa_mask >> aa) & 1u) == 0u) continue;
                for (int brushes = 0; brushes < 2; brushes++) {
                    c->force_brushes = brushes != 0;
                    vello_hip_render_params rp{16u, 16u, 0u, aa};
                    (void)vello_hip_render_resident(c, &rp, nullptr, 0);
                }
            }
            c->force_brushes = false;
            (void)sync_all(c);
            c->lanes[0].used = false;
            c->have_cfg = false;
        }
        c->shared.resident = false;  // the caller uploads its own scene
        c->last_error.clear();
    }
    *out = c;
    return VELLO_HIP_OK;
}

// Waits for everything the context has enqueued, then destroys its streams and events; the device buffers and the pinned staging
// blocks go with the structs that own them (DevBuf, Staging).
void vello_hip_destroy(vello_hip_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // (instance tables travel on the lanes' streams, with or without an upload stream)
    for (auto &l : c->lanes)
        if (l.stream) (void)hipStreamSynchronize(l.stream);
    if (c->upload_stream) (void)hipStreamSynchronize(c->upload_stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (auto &l : c->lanes) {
        l.return_events(c->event_pool);
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->upload_stream) {
        (void)hipEventDestroy(c->atlas_ready);
        (void)hipEventDestroy(c->lane_mark);
        (void)hipStreamDestroy(c->upload_stream);
    }
    if (c->pose_mark) (void)hipEventDestroy(c->pose_mark);
    if (c->base_ready) (void)hipEventDestroy(c->base_ready);  // (vello_hip_set_base_image)
    if (c->base_mark) (void)hipEventDestroy(c->base_mark);
    if (c->frame_done) (void)hipEventDestroy(c->frame_done);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    delete c;
}

int vello_hip_set_frames_in_flight(vello_hip_ctx *c, uint32_t n) {
    if (!c || n < 1 || n > MAX_LANES) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int r = sync_all(c);
    if (r) return r;
    size_t old = c->lanes.size();
    if (n > old) {
        c->lanes.resize(n);
        for (size_t i = old; i < n; i++) {
            if ((r = alloc_lane_pools(c, c->lanes[i]))) return r;
            if (c->shared.resident && (r = alloc_lane_scene(c, c->lanes[i], c->shared))) return r;
        }
    }
    if ((c->n_active == 1u) != (n == 1u)) {
        // fine's slicing threshold differs between one frame at a time and frames in flight (engine.h FINE_SLICE_MIN_FILLS*): the
        // slice items a frame of the scene was seen to ask for say nothing about the other mode -- unknown again (the default
        // capacity, and the next finished frame is read back)
        c->shared.slice_demand = -1;
        c->retained.slice_demand = -1;
        for (auto &l : c->lanes) l.own.slice_demand = -1;
    }
    c->n_active = n;  // shrinking keeps the extra lanes' buffers; only the rotation changes
    c->next_lane = 0;
    c->last_lane = 0;
    return VELLO_HIP_OK;
}

int vello_hip_lane_stream_priority(vello_hip_ctx *c, uint32_t lane, int *priority, int *device_least, int *device_greatest) {
    if (!c || lane >= c->lanes.size() || !c->lanes[lane].stream) return VELLO_HIP_E_INVALID;
    int p = 0, least = 0, greatest = 0;
#ifndef VELLO_SIMT_EMU  // (the emulator has no queues: one priority, 0)
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamGetPriority(c->lanes[lane].stream, &p));
    HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
#endif
    if (priority) *priority = p;
    if (device_least) *device_least = least;
    if (device_greatest) *device_greatest = greatest;
    return VELLO_HIP_OK;
}

int vello_hip_get_capacities(vello_hip_ctx *c, vello_hip_capacities *out) {
    if (!c || !out) return VELLO_HIP_E_INVALID;
    *out = c->caps;
    return VELLO_HIP_OK;
}

// The step the reference leaves as a TODO (lib.rs:753-764, "apply logic to determine whether we need to rerun
// coarse"): size every pool whose counter exceeded it for the reported demand.  A stage that overflows stops the
// stages behind it (bump.failed, shared/bump.wgsl:5-9), so a frame may need one call per overflowing stage.
int vello_hip_grow_pools(vello_hip_ctx *c, const vello_hip_bump *demand, vello_hip_capacities *new_caps) {
    if (!c || !demand) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    vello_hip_capacities d = c->caps;
    bool grew = false;
    // 25 % headroom, rounded up to 64 Ki elements; counters are u32, so is every pool
    auto want = [&](uint32_t &cap, uint64_t need) {
        if (need <= cap) return;
        uint64_t n = need + need / 4u;
        n = (n + 0xffffu) & ~(uint64_t)0xffffu;
        if (n > 0xffff0000ull) n = 0xffff0000ull;
        if (n > cap) {
            cap = (uint32_t)n;
            grew = true;
        }
    };
    want(d.lines, demand->lines);
    want(d.bin_data, (uint64_t)demand->binning + slot_of(c, c->lanes[c->last_lane]).layout.bin_data_start);
    want(d.tiles, demand->tile);
    want(d.seg_counts, demand->seg_counts);
    want(d.segments, demand->segments);
    want(d.blend_spill, demand->blend);
    if (c->have_cfg) {
        uint64_t dyn_start = (uint64_t)c->cfg.width_in_tiles * c->cfg.height_in_tiles * PTCL_INITIAL_ALLOC;
        want(d.ptcl, dyn_start + demand->ptcl + PTCL_INCREMENT);
    }
    if (d.segments < d.seg_counts) {
        d.segments = d.seg_counts;
        grew = true;
    }
    if (new_caps) *new_caps = d;
    if (!grew) {
        c->last_error = "grow_pools: no counter exceeds its pool";
        return VELLO_HIP_E_INVALID;
    }
    int r = sync_all(c);
    if (r) return r;
    if ((r = commit_caps(c, d))) return r;
    for (auto &l : c->lanes) l.used = false;  // the frames rendered into the old pools are void; their failure has been acted upon
    return VELLO_HIP_OK;
}

}  // extern "C"
