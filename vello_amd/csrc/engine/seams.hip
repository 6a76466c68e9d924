// The seams for tests, tools and several GPUs: buffer reads and writes, debug flags, stage and kernel times, frame gather, mask LUTs.
#include "ctx.h"

using namespace vk;

namespace vk {

hipEvent_t get_event(vello_hip_ctx *c) {
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

}  // namespace vk

namespace {

const char *kStageNames[VELLO_HIP_STAGE_COUNT] = {"pathtag_scan", "flatten",  "draw_scan", "clip",        "binning", "tile_alloc",
                                                  "path_count",   "backdrop", "coarse",    "path_tiling", "fine"};

int drain_events(vello_hip_ctx *c) {
    for (auto &l : c->lanes) {
        for (auto &ev : l.events) {
            float ms = 0.f;
            HIP_TRY(c, hipEventSynchronize(ev.b));
            HIP_TRY(c, hipEventElapsedTime(&ms, ev.a, ev.b));
            c->stage_ms[ev.stage] += ms;
            c->stage_count[ev.stage] += 1;
            if (ev.mid[0]) {  // a -> mid[0] (-> mid[1]) -> b: the stage's kernels one by one
                hipEvent_t pts[4] = {ev.a, ev.mid[0], ev.mid[1] ? ev.mid[1] : ev.b, ev.b};
                const int n_k = ev.mid[1] ? 3 : 2;
                for (int k = 0; k < n_k; k++) {
                    float kms = 0.f;
                    if (hipEventElapsedTime(&kms, pts[k], pts[k + 1]) == hipSuccess) c->kernel_ms[ev.stage][k] += kms;
                }
                c->kernel_count[ev.stage] += 1;
            }
        }
        l.return_events(c->event_pool);
    }
    return 0;
}

// brings the device copy of the Config up to the last frame's (vello_hip_render_instances leaves it to the reader)
int send_config(vello_hip_ctx *c) {
    if (!c->cfg_unsent) return 0;
    HIP_TRY(c, hipMemcpy(c->config.ptr, &c->cfg, sizeof(Config), hipMemcpyHostToDevice));
    c->cfg_unsent = false;
    return 0;
}

// what a buffer id shows of the lane that rendered last
struct BufView {
    void *ptr;
    size_t size;
};
BufView find_buf(vello_hip_ctx *c, int id) {
    Lane &l = c->lanes[c->last_lane];
    // (the bump allocators first, then the engine's own counters: the head of the lane's zero region)
    if (id == VELLO_HIP_BUF_BUMP) return {l.zero_region.ptr, l.zero_region.ptr ? sizeof(Control) : 0u};
    // (a frame of an indexed scene read the index's tag monoids, not its lane's)
    if (id == VELLO_HIP_BUF_TAG_MONOIDS && l.frame_indexed && l.which == LaneScene::Shared && c->shared.index.valid)
        return {c->shared.index.monoids.ptr, c->shared.index.monoids.size};
    const DevBuf &b = id == VELLO_HIP_BUF_SCENE ? slot_of(c, l).scene : id == VELLO_HIP_BUF_CONFIG ? c->config : l.buf[id];
    return {b.ptr, b.size};
}

// vello_encoding/src/mask.rs:11-98
const uint8_t PATTERN8[8] = {0, 5, 3, 7, 1, 4, 6, 2};
const uint8_t PATTERN16[16] = {1, 8, 4, 11, 15, 7, 3, 12, 0, 9, 5, 13, 2, 10, 6, 14};
uint32_t one_mask_n(double slope, double translation, bool is_pos, const uint8_t *pat, int n) {
    if (is_pos) translation = 1. - translation;
    uint32_t result = 0;
    double inv = 1.0 / (double)n;
    for (int i = 0; i < n; i++) {
        double y = ((double)i + 0.5) * inv;
        double x = ((double)pat[i] + 0.5) * inv;
        if (!is_pos) y = 1. - y;
        if ((x - (1.0 - translation)) * (1. - slope) - (y - translation) * slope >= 0.) result |= 1u << i;
    }
    return result;
}

// vello_hip_read_buffer / vello_hip_write_buffer: `host` is the destination or the source
int access_buffer(vello_hip_ctx *c, int id, void *host, size_t offset, size_t size, bool write) {
    if (!c || id < 0 || id >= VELLO_HIP_BUF_COUNT || !host) return VELLO_HIP_E_INVALID;
    const BufView b = find_buf(c, id);
    if (!b.ptr || offset + size > b.size) {
        c->last_error = write ? "write_buffer out of range" : "read_buffer out of range";
        return VELLO_HIP_E_INVALID;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int r = sync_all(c);
    if (r) return r;
    if (id == VELLO_HIP_BUF_CONFIG && (r = send_config(c))) return r;
    // (bytes written into an indexed scene: its index speaks for the bytes of the upload -- the frames from here on take the
    // per-frame path, until the next upload builds a new one)
    if (write && id == VELLO_HIP_BUF_SCENE && &slot_of(c, c->lanes[c->last_lane]) == &c->shared) c->shared.index.valid = false;
    if (write) HIP_TRY(c, hipMemcpy((char *)b.ptr + offset, host, size, hipMemcpyHostToDevice));
    else HIP_TRY(c, hipMemcpy(host, (const char *)b.ptr + offset, size, hipMemcpyDeviceToHost));
    return VELLO_HIP_OK;
}

}  // namespace

extern "C" {

void vello_hip_make_mask_lut(uint8_t out[1024]) {
    const int W = 32, H = 32, HALF = 16;
    for (int i = 0; i < W * H; i++) {
        int u = i % W, v = i / W;
        double y = ((double)(v % HALF) + 0.5) * (1.0 / (double)HALF);
        double x = ((double)u + 0.5) * (1.0 / (double)W);
        out[i] = (uint8_t)one_mask_n(y, x, v >= HALF, PATTERN8, 8);
    }
}

void vello_hip_make_mask_lut_16(uint8_t out[8192]) {
    const int W = 64, H = 64, HALF = 32;
    for (int i = 0; i < W * H; i++) {
        int u = i % W, v = i / W;
        double y = ((double)(v % HALF) + 0.5) * (1.0 / (double)HALF);
        double x = ((double)u + 0.5) * (1.0 / (double)W);
        uint32_t m = one_mask_n(y, x, v >= HALF, PATTERN16, 16);
        out[2 * i] = (uint8_t)(m & 0xff);
        out[2 * i + 1] = (uint8_t)(m >> 8);
    }
}

const char *vello_hip_stage_name(int stage) {
    if (stage < 0 || stage >= VELLO_HIP_STAGE_COUNT) return "?";
    return kStageNames[stage];
}

uint32_t vello_hip_stage_constant(int which) {
    switch (which) {
    case VELLO_HIP_SHAPE_PATHTAG_PART_TAGS: return PATHTAG_PART_WORDS * 4u;
    case VELLO_HIP_SHAPE_FLATTEN_BLOCK_TAGS: return FLATTEN_BLOCK_TAGS;
    case VELLO_HIP_SHAPE_DRAW_PART: return DRAW_PART;
    case VELLO_HIP_SHAPE_CLIP_PART: return CLIP_PART;
    case VELLO_HIP_SHAPE_DRAW_WORKGROUP: return DRAW_WG;
    case VELLO_HIP_SHAPE_COARSE_BATCH: return coarse_batch_draws();
    case VELLO_HIP_SHAPE_COARSE_GRID_BINS: return coarse_grid_bins();
    case VELLO_HIP_SHAPE_PATH_COUNT_CHUNK: return path_count_chunk(0);
    case VELLO_HIP_SHAPE_PATH_COUNT_CHUNK_SMALL: return path_count_chunk(1);
    case VELLO_HIP_SHAPE_PATH_COUNT_CHUNK_IN_FLIGHT: return path_count_chunk(2);
    case VELLO_HIP_SHAPE_PATH_TILING_WORKGROUP: return path_tiling_workgroup();
    case VELLO_HIP_SHAPE_BACKDROP_BLOCK_TILES: return backdrop_block_tiles();
    case VELLO_HIP_SHAPE_FRONT_MAX_TAGS: return FRONT_MAX_TAGS;
    case VELLO_HIP_SHAPE_FRONT_MAX_DRAW_OBJECTS: return FRONT_MAX_DRAW_OBJECTS;
    case VELLO_HIP_SHAPE_FRONT_TINY_SEGMENTS: return FRONT_TINY_SEGMENTS;
    case VELLO_HIP_SHAPE_FINE_WINDOW_WORDS: return fine_window_words();
    case VELLO_HIP_SHAPE_FINE_BATCH_FILLS: return fine_batch_fills();
    case VELLO_HIP_SHAPE_FINE_BATCH_SEGMENTS: return fine_batch_segments();
    case VELLO_HIP_SHAPE_FINE_ITEM_CAP: return fine_item_cap();
    case VELLO_HIP_SHAPE_FINE_SIMPLE_RECORDS: return fine_simple_records();
    case VELLO_HIP_SHAPE_FINE_PREFETCH_REACH: return fine_prefetch_reach();
    case VELLO_HIP_SHAPE_FINE_SLICE_FILLS: return FINE_SLICE_FILLS;
    case VELLO_HIP_SHAPE_FINE_SLICE_MIN_FILLS: return FINE_SLICE_MIN_FILLS;
    case VELLO_HIP_SHAPE_FINE_SLICE_MIN_FILLS_IN_FLIGHT: return FINE_SLICE_MIN_FILLS_IN_FLIGHT;
    case VELLO_HIP_SHAPE_FINE_SLICE_FILLS_FORCED: return FINE_SLICE_FILLS_FORCED;
    case VELLO_HIP_SHAPE_FINE_SLICE_MIN_FILLS_FORCED: return FINE_SLICE_MIN_FILLS_FORCED;
    case VELLO_HIP_SHAPE_FINE_HEAVY_WORDS: return FINE_HEAVY_WORDS;
    case VELLO_HIP_SHAPE_FINE_BUCKET_WORDS: return FINE_BUCKET_WORDS;
    case VELLO_HIP_SHAPE_FINE_BUCKETS: return FINE_WORK_BUCKETS;
    case VELLO_HIP_SHAPE_PTCL_INITIAL_ALLOC: return PTCL_INITIAL_ALLOC;
    case VELLO_HIP_SHAPE_PATH_BLEND_VEC_WORDS: return PATH_BLEND_VEC_WORDS;
    default: return 0u;
    }
}

size_t vello_hip_buffer_size(vello_hip_ctx *c, int id) {
    if (!c || id < 0 || id >= VELLO_HIP_BUF_COUNT) return 0;
    return find_buf(c, id).size;
}

int vello_hip_read_buffer(vello_hip_ctx *c, int id, void *dst, size_t offset, size_t size) { return access_buffer(c, id, dst, offset, size, false); }

int vello_hip_write_buffer(vello_hip_ctx *c, int id, const void *src, size_t offset, size_t size) {
    return access_buffer(c, id, const_cast<void *>(src), offset, size, true);
}

int vello_hip_set_debug_flags(vello_hip_ctx *c, uint32_t flags) {
    if (!c) return VELLO_HIP_E_INVALID;
    if ((c->debug_flags ^ flags) & VELLO_HIP_DEBUG_FINE_SLICES) {  // what earlier frames asked for says nothing about the other slice size
        c->shared.slice_demand = -1;
        c->retained.slice_demand = -1;
        for (auto &l : c->lanes) l.own.slice_demand = -1;
    }
    c->debug_flags = flags;
    return VELLO_HIP_OK;
}

int vello_hip_set_profiling(vello_hip_ctx *c, uint32_t stage_mask) {
    if (!c) return VELLO_HIP_E_INVALID;
    c->prof_mask = stage_mask;
    return VELLO_HIP_OK;
}

int vello_hip_get_stage_ms(vello_hip_ctx *c, float ms_out[VELLO_HIP_STAGE_COUNT], uint32_t count_out[VELLO_HIP_STAGE_COUNT]) {
    if (!c) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int r = drain_events(c);
    if (r) return r;
    for (int i = 0; i < VELLO_HIP_STAGE_COUNT; i++) {
        if (ms_out) ms_out[i] = c->stage_ms[i];
        if (count_out) count_out[i] = c->stage_count[i];
        c->stage_ms[i] = 0.f;
        c->stage_count[i] = 0;
    }
    return VELLO_HIP_OK;
}

int vello_hip_get_kernel_ms(vello_hip_ctx *c, int stage, float ms_out[3], uint32_t *count_out) {
    if (!c || stage < 0 || stage >= VELLO_HIP_STAGE_COUNT || !ms_out) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int r = drain_events(c);
    if (r) return r;
    for (int k = 0; k < 3; k++) {
        ms_out[k] = c->kernel_ms[stage][k];
        c->kernel_ms[stage][k] = 0.f;
    }
    if (count_out) *count_out = c->kernel_count[stage];
    c->kernel_count[stage] = 0;
    return VELLO_HIP_OK;
}

// The one exchange step of the path for a host that owns one context per GPU in ONE process: every
// context's finished frame goes to `dst_device` with hipMemcpyPeerAsync on that context's own copy stream -- the SDMA
// engines move it over the peer's own xGMI link, no CU is involved and the copies of different peers run concurrently
// -- ordered behind the frame the context enqueued last by an event, not by a host wait.  (One process per GPU, as
// bench.py runs, gathers with RCCL instead: vello_amd/distributed.py.)
int vello_hip_gather_frames(vello_hip_ctx *const *ctxs, uint32_t n, int dst_device, const void *const *src_frames, void *const *dst_frames,
                            size_t frame_bytes) {
    if (!ctxs || !src_frames || !dst_frames || n == 0) return VELLO_HIP_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        vello_hip_ctx *c = ctxs[i];
        if (!c || !src_frames[i] || !dst_frames[i]) return VELLO_HIP_E_INVALID;
        HIP_TRY(c, hipSetDevice(c->device));
        if (!c->copy_stream) {
            HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
            HIP_TRY(c, hipEventCreateWithFlags(&c->frame_done, hipEventDisableTiming));
            if (c->device != dst_device) {
                hipError_t e = hipDeviceEnablePeerAccess(dst_device, 0);  // direct xGMI path; already enabled is fine
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();  // staged copies still work
            }
        }
        HIP_TRY(c, hipEventRecord(c->frame_done, c->lanes[c->last_lane].stream));
        HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->frame_done, 0));
        HIP_TRY(c, hipMemcpyPeerAsync(dst_frames[i], dst_device, src_frames[i], c->device, frame_bytes, c->copy_stream));
    }
    return VELLO_HIP_OK;
}

int vello_hip_gather_wait(vello_hip_ctx *const *ctxs, uint32_t n) {
    if (!ctxs) return VELLO_HIP_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        vello_hip_ctx *c = ctxs[i];
        if (!c) return VELLO_HIP_E_INVALID;
        if (!c->copy_stream) continue;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    }
    return VELLO_HIP_OK;
}

}  // extern "C"
