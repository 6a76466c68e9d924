// Hit testing (vello_hip_pick): which draw object, and which instance, lies topmost under a point of the frame submitted last.
// The contract is in include/vello_hip.h; the arguments, the chunk sizes and the batch rule are in engine.h.  Two kernels read what
// the frame left in its lane -- the line soup, the draw monoids, the path boxes' draw flags -- and write a scratch table and the
// answers; nothing the frame path reads is written.
#include "ctx.h"
#include "pick_common.h"

namespace vk {

namespace {

// rule 3: a point outside the target, a NaN (every comparison false) or an infinity misses
__device__ __forceinline__ bool pick_in_target(float qx, float qy, float w, float h) { return qx >= 0.0f && qx < w && qy >= 0.0f && qy < h; }

}  // namespace

// k_pick_lines: rule 1, the winding of every path at every query of the batch.  A workgroup per PICK_LINES_CHUNK lines of the soup,
// a lane per line: the record is loaded once and kept in registers while the workgroup walks the batch's queries.  A query is the
// same for every lane (its two floats are scalar loads), and so is the test whether it lies in the target.  Per query and line the
// two half-open y tests run in f32 -- promotion to f64 is exact, so they are the contract's -- and almost every lane fails both: the
// f64 cross product and the atomic are under a branch that a wave with no survivor jumps over.  A survivor adds +1 or -1 (as
// 0xffffffff: the table is u32 and wraps) to winding[q][path_ix]; the sum does not depend on the order of the adds, nor on the order
// of the soup.  d is formed in f64 without contraction (the translation unit is compiled with -ffp-contract=off, as the f32 rules of
// common.h need): four differences, two products, one difference, each rounded on its own.
__global__ void __launch_bounds__(256) k_pick_lines(PickArgs a) {
    const uint32_t ix = blockIdx.x * PICK_LINES_CHUNK + threadIdx.x;
    LineSoup l{};
    bool counted = false;
    if (ix < a.n_lines) {
        l = pick_load_line(a.lines, ix);
        counted = l.path_ix < a.n_paths;
    }
    const float w = (float)a.width, h = (float)a.height;
    for (uint32_t q = 0; q < a.nq; q++) {
        const float qx = a.points[2u * (size_t)(a.q0 + q)], qy = a.points[2u * (size_t)(a.q0 + q) + 1u];
        if (!pick_in_target(qx, qy, w, h)) continue;
        const bool up = counted && l.p0y <= qy && qy < l.p1y;
        const bool down = counted && l.p1y <= qy && qy < l.p0y;
        if (up || down) {
            const double p0x = (double)l.p0x, p0y = (double)l.p0y, p1x = (double)l.p1x, p1y = (double)l.p1y;
            const double d = (p1x - p0x) * ((double)qy - p0y) - ((double)qx - p0x) * (p1y - p0y);
            uint32_t *cell = a.winding + (size_t)q * a.n_paths + l.path_ix;
            if (up && d < 0.0) atomicAdd(cell, 1u);
            if (down && d > 0.0) atomicAdd(cell, 0xffffffffu);
        }
    }
}

// k_pick_resolve: rules 2 to 4, a workgroup per query.  The draw objects are walked in chunks of PICK_DRAW_CHUNK, a lane each.  The
// clip stack of the contract is its prefix-sum form: v is +1 on a BeginClip whose path is not hit, -1 (wrapping) on an EndClip whose
// patched path is not hit, and a paint draw is a candidate when its path is hit and the exclusive prefix of v is 0 -- a workgroup
// scan per chunk (wave DPP scans and one LDS hop, block256_incl_scan_u32) plus the carry of the chunks before.  A lane's candidates
// only grow, so it keeps the last; the workgroup's largest is the answer, held as index + 1 so that 0 is "none".  Thread 0 then
// finds the owner -- the last entry of the draw-tag prefix that is <= the index -- and writes the two words.
__global__ void __launch_bounds__(256) k_pick_resolve(PickArgs a) {
    __shared__ uint32_t sh_scan[4];
    __shared__ uint32_t sh_best[4];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const int lane = (int)(tid & 63u), wv = (int)(tid >> 6);
    const float qx = a.points[2u * (size_t)(a.q0 + q)], qy = a.points[2u * (size_t)(a.q0 + q) + 1u];
    uint32_t best = 0u;
    if (pick_in_target(qx, qy, (float)a.width, (float)a.height)) {
        const uint32_t *winding = a.winding + (size_t)q * a.n_paths;
        const uint32_t n_chunks = (uint32_t)(((uint64_t)a.n_draw + PICK_DRAW_CHUNK - 1u) / PICK_DRAW_CHUNK);
        uint32_t carry = 0u;
        for (uint32_t c = 0; c < n_chunks; c++) {
            const uint64_t ix64 = (uint64_t)c * PICK_DRAW_CHUNK + tid;
            const bool live = ix64 < a.n_draw;
            const uint32_t ix = (uint32_t)ix64;
            const uint32_t tag = live ? a.draw_tags[ix] : DRAWTAG_NOP;
            const bool paint = pick_is_paint(tag), begin = tag == DRAWTAG_BEGIN_CLIP, end = tag == DRAWTAG_END_CLIP;
            bool hit = false;
            if (paint || begin || end) {
                const uint32_t path_ix = a.draw_monoids[ix].path_ix;
                if (path_ix < a.n_paths) {  // (an EndClip nothing matched keeps an index of its own: it may be n_paths)
                    const uint32_t wn = winding[path_ix];
                    hit = (a.path_bboxes[path_ix].draw_flags & DRAW_INFO_FLAGS_FILL_RULE_BIT) != 0u ? (wn & 1u) != 0u : wn != 0u;
                }
            }
            const uint32_t v = begin && !hit ? 1u : end && !hit ? 0xffffffffu : 0u;
            uint32_t total;
            const uint32_t incl = block256_incl_scan_u32(v, sh_scan, &total);
            if (paint && hit && carry + (incl - v) == 0u) best = ix + 1u;
            carry += total;
        }
    }
    best = wave_incl_scan_max_u32(best, lane);
    if (lane == 63) sh_best[wv] = best;
    __syncthreads();
    if (tid != 0u) return;
    best = maxu(maxu(sh_best[0], sh_best[1]), maxu(sh_best[2], sh_best[3]));
    uint32_t draw_ix = PICK_NONE, inst = PICK_NONE;
    if (best != 0u) {
        draw_ix = best - 1u;
        if (a.prefix != nullptr && a.n_inst != 0u) {
            uint32_t lo = 0u, hi = a.n_inst - 1u;  // the last entry <= draw_ix: empty instances repeat an offset, the last of a run holds the draw
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1u) >> 1;
                if (a.prefix[mid] <= draw_ix) lo = mid;
                else hi = mid - 1u;
            }
            inst = lo;
        }
    }
    a.out[2u * (size_t)(a.q0 + q)] = draw_ix;
    a.out[2u * (size_t)(a.q0 + q) + 1u] = inst;
}

void launch_pick_lines(const PickArgs &a, hipStream_t s) {
    const uint32_t wgs = (uint32_t)(((uint64_t)a.n_lines + PICK_LINES_CHUNK - 1u) / PICK_LINES_CHUNK);
    if (wgs == 0u || a.n_paths == 0u || a.nq == 0u) return;
    hipLaunchKernelGGL(k_pick_lines, dim3(wgs), dim3(256), 0, s, a);
}

void launch_pick_resolve(const PickArgs &a, hipStream_t s) {
    if (a.nq == 0u) return;
    hipLaunchKernelGGL(k_pick_resolve, dim3(a.nq), dim3(256), 0, s, a);
}

}  // namespace vk

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
using namespace vk;

static_assert(PICK_NONE == VELLO_HIP_PICK_NONE && PICK_MAX_POINTS == VELLO_HIP_PICK_MAX_POINTS && sizeof(vello_hip_pick_hit) == 8,
              "k_pick_resolve writes vello_hip_pick_hit entries");

namespace vk {

// Why `bytes` bytes at `p` are not what a kernel of this context may be handed as device memory (nullptr: they are): the test
// vello_hip_render_retained applies to device poses.  The emulated build has one address space and tests the alignment only.
const char *not_device_memory(vello_hip_ctx *c, const void *p, size_t bytes) {
    if ((reinterpret_cast<uintptr_t>(p) & 3u) != 0u) return "is not a multiple of 4";
#ifndef VELLO_SIMT_EMU
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    hipPointerAttribute_t attr{};
    hipError_t e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)const_cast<void *>(p));
    if (e == hipSuccess) e = hipPointerGetAttributes(&attr, base);
    (void)hipGetLastError();  // a host address is an error here: do not leave it for the next launch check
    if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != c->device) return "is not device memory of the context's device";
    if ((uint64_t)(uintptr_t)p + bytes > (uint64_t)(uintptr_t)base + size) return "runs past the end of its allocation";
#else
    (void)c;
    (void)bytes;
#endif
    return nullptr;
}

// "The frame" of a query: the lane of the frame submitted last, its scene and -- a frame composed from instances -- the draw-tag
// prefix: the lane's own table, or the retained list's copy.  nullptr, or why there is no frame to answer against.
const char *query_frame(vello_hip_ctx *c, QueryFrame &q) {
    Lane &l = c->lanes[c->last_lane];
    if (!c->have_cfg || !l.used || !l.flatten_ran || !l.zero_region.ptr) return "no frame has been rendered";
    const SceneSlot &sc = slot_of(c, l);
    if (!sc.resident || l.frame_generation != sc.generation) return "the scene of the last frame has been replaced since";
    q.lane = &l;
    q.scene = &sc;
    q.prefix = nullptr;
    q.n_inst = 0u;
    if (l.which == LaneScene::Own && l.own.composed && l.compose_n != 0u) {
        q.prefix = (const uint32_t *)l.compose_table.ptr + 2u * ((size_t)l.compose_n + 1u);
        q.n_inst = l.compose_n;
    } else if (l.which == LaneScene::Retained && c->retained_n != 0u) {
        q.prefix = (const uint32_t *)c->retained_prefix.ptr;
        q.n_inst = c->retained_n;
    }
    return nullptr;
}

// Waits for the query's frame and judges it as vello_hip_sync does -- without that call's side effects.  `who` heads the message.
int judge_frame(vello_hip_ctx *c, const char *who, Lane &l, Bump &bump) {
    HIP_TRY(c, hipStreamSynchronize(l.stream));
    HIP_TRY(c, hipMemcpy(&bump, l.zero_region.ptr, sizeof bump, hipMemcpyDeviceToHost));
    if (bump.failed == 0u) return VELLO_HIP_OK;
    const std::string head = std::string(who) + ": ";
    if ((bump.failed & FAILED_SCENE) != 0u) {
        c->last_error = head + "the frame was discarded (its path tag stream or its poses contradict its scene)";
        return VELLO_HIP_E_INVALID;
    }
    if ((bump.failed & FAILED_INTERNAL) != 0u) {
        c->last_error = head + "the frame was discarded (an engine-internal wait gave up)";
        return VELLO_HIP_E_INTERNAL;
    }
    c->last_error = head + "the frame overflowed a pool (bump.failed=" + std::to_string(bump.failed) + "): its line soup is short";
    return VELLO_HIP_E_CAPACITY;
}

}  // namespace vk

extern "C" {

uint32_t vello_hip_pick_constant(int which) {
    switch (which) {
    case VELLO_HIP_PICK_LINES_PER_WORKGROUP: return PICK_LINES_CHUNK;
    case VELLO_HIP_PICK_DRAWS_PER_STEP: return PICK_DRAW_CHUNK;
    case VELLO_HIP_PICK_SMALL_BATCH: return PICK_BATCH_FORCED;
    case VELLO_HIP_PICK_SCRATCH_BYTES: return (uint32_t)PICK_SCRATCH_BYTES;
    case VELLO_HIP_PICK_RECT_LINES_PER_WORKGROUP: return REGION_LINES_CHUNK;
    case VELLO_HIP_PICK_RECT_DRAWS_PER_WORKGROUP: return REGION_DRAW_CHUNK;
    default: return 0u;
    }
}

int vello_hip_pick_ms(vello_hip_ctx *c, float *ms_out) {
    if (!c || !ms_out) return VELLO_HIP_E_INVALID;
    *ms_out = c->pick_ms;
    return VELLO_HIP_OK;
}

int vello_hip_pick(vello_hip_ctx *c, const float *points, uint32_t n, int points_is_device, void *src_stream, vello_hip_pick_hit *out,
                   int out_is_device) {
    if (!c) return VELLO_HIP_E_INVALID;
    if (n == 0u) return VELLO_HIP_OK;
    auto refuse = [&](const std::string &why) {
        c->last_error = "pick: " + why;
        return VELLO_HIP_E_INVALID;
    };
    if (!points) return refuse("points is NULL");
    if (!out) return refuse("out is NULL");
    if (n > VELLO_HIP_PICK_MAX_POINTS) return refuse(std::to_string(n) + " points (at most VELLO_HIP_PICK_MAX_POINTS = " + std::to_string(VELLO_HIP_PICK_MAX_POINTS) + ")");
    if (src_stream && !points_is_device) return refuse("src_stream goes with points in device memory");
    QueryFrame qf;
    if (const char *why = query_frame(c, qf)) return refuse(why);
    Lane &l = *qf.lane;
    const SceneSlot &sc = *qf.scene;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * 8u;
    if (points_is_device)
        if (const char *why = not_device_memory(c, points, bytes)) return refuse(std::string("the address of device points ") + why);
    if (out_is_device)
        if (const char *why = not_device_memory(c, out, bytes)) return refuse(std::string("the address of a device result ") + why);

    hipStream_t st = l.stream;
    Bump bump;
    if (int r = judge_frame(c, "pick", l, bump)) return r;

    const Config &cfg = l.frame_cfg;
    PickArgs a{};
    a.lines = (const LineSoup *)l.buf[VELLO_HIP_BUF_LINES].ptr;
    a.n_lines = bump.lines < cfg.lines_size ? bump.lines : cfg.lines_size;
    a.n_paths = cfg.layout.n_paths;
    a.n_draw = cfg.layout.n_draw_objects;
    a.draw_tags = (const uint32_t *)sc.scene.ptr + cfg.layout.draw_tag_base;
    a.draw_monoids = (const DrawMonoid *)l.buf[VELLO_HIP_BUF_DRAW_MONOIDS].ptr;
    a.path_bboxes = (const PathBbox *)l.buf[VELLO_HIP_BUF_PATH_BBOXES].ptr;
    a.width = cfg.target_width;
    a.height = cfg.target_height;
    a.prefix = qf.prefix;
    a.n_inst = qf.n_inst;

    const uint32_t batch = pick_batch(a.n_paths, (c->debug_flags & VELLO_HIP_DEBUG_PICK_SMALL_BATCHES) != 0u);
    const size_t row_bytes = (size_t)a.n_paths * 4u;
    int r;
    if ((r = ensure(c, c->pick_winding, (size_t)(batch < n ? batch : n) * row_bytes))) return r;
    if (!points_is_device && (r = ensure(c, c->pick_points, bytes))) return r;
    if (!out_is_device && (r = ensure(c, c->pick_out, bytes))) return r;
    a.winding = (uint32_t *)c->pick_winding.ptr;
    if (points_is_device) {
        a.points = points;
        if (src_stream) {  // behind what the caller's stream has been given so far
            if (!c->pose_mark) HIP_TRY(c, hipEventCreateWithFlags(&c->pose_mark, hipEventDisableTiming));
            HIP_TRY(c, hipEventRecord(c->pose_mark, (hipStream_t)src_stream));
            HIP_TRY(c, hipStreamWaitEvent(st, c->pose_mark, 0));
        }
    } else {
        HIP_TRY(c, hipMemcpyAsync(c->pick_points.ptr, points, bytes, hipMemcpyHostToDevice, st));
        a.points = (const float *)c->pick_points.ptr;
    }
    a.out = out_is_device ? reinterpret_cast<uint32_t *>(out) : (uint32_t *)c->pick_out.ptr;
    // with profiling on (vello_hip_set_profiling, any stage): two events around the launches, read by vello_hip_pick_ms
    const bool prof = c->prof_mask != 0u;
    hipEvent_t ev_a = prof ? get_event(c) : nullptr, ev_b = prof ? get_event(c) : nullptr;
    c->pick_ms = 0.f;
    if (prof) HIP_TRY(c, hipEventRecord(ev_a, st));
    for (uint32_t q0 = 0; q0 < n; q0 += batch) {
        a.q0 = q0;
        a.nq = n - q0 < batch ? n - q0 : batch;
        if (row_bytes) HIP_TRY(c, hipMemsetAsync(a.winding, 0, (size_t)a.nq * row_bytes, st));
        launch_pick_lines(a, st);
        HIP_TRY(c, hipGetLastError());
        launch_pick_resolve(a, st);
        HIP_TRY(c, hipGetLastError());
    }
    if (prof) HIP_TRY(c, hipEventRecord(ev_b, st));
    if (!out_is_device) HIP_TRY(c, hipMemcpyAsync(out, c->pick_out.ptr, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (prof) {
        (void)hipEventElapsedTime(&c->pick_ms, ev_a, ev_b);
        c->event_pool.push_back(ev_a);
        c->event_pool.push_back(ev_b);
    }
    return VELLO_HIP_OK;
}

}  // extern "C"
