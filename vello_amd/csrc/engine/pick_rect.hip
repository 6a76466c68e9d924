// Marquee selection (vello_hip_pick_rect): which draw objects, and which instances, a rectangle of the frame submitted last touches
// and which it encloses.  The contract is in include/vello_hip.h; the arguments, the chunk sizes and the scratch layout are in
// engine.h.  Four kernels read what the frame left in its lane -- the line soup, the draw monoids, the path boxes -- and write the
// context's scratch and the answers; nothing the frame path reads is written, no workgroup waits for another.
#include <cstring>

#include "ctx.h"
#include "pick_common.h"

namespace vk {

namespace {

// min and max of a line's two coordinates such that a NaN in EITHER makes one of them NaN, which fails every comparison of the box
// test: a NaN `a` leaves lo = b but hi = a, a NaN `b` leaves hi = a but lo = b.  (minf / maxf of common.h drop a NaN first operand.)
__device__ __forceinline__ float region_lo(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float region_hi(float a, float b) { return b > a ? b : a; }

__device__ __forceinline__ uint32_t *region_meets(const RegionArgs &a) { return a.scratch; }
__device__ __forceinline__ uint32_t *region_winding(const RegionArgs &a) { return a.scratch + a.n_paths; }
__device__ __forceinline__ uint32_t *region_inst(const RegionArgs &a) { return a.scratch + 2u * (size_t)a.n_paths; }
__device__ __forceinline__ uint32_t *region_counts(const RegionArgs &a) { return region_inst(a) + a.n_inst; }
__device__ __forceinline__ uint32_t *region_totals(const RegionArgs &a) { return region_counts(a) + 4u; }

// What rule 2 needs of one draw object: the lane's term of the clip stack's prefix-sum form (+1 on a BeginClip whose path is not
// TOUCH, -1, wrapping, on an EndClip whose patched path is not TOUCH) and, for a paint draw, TOUCH and the two box tests of its path.
struct RegionDraw {
    uint32_t v;
    bool paint, touch, boxed, nonempty;
};
__device__ __forceinline__ RegionDraw region_draw(const RegionArgs &a, uint64_t ix64) {
    RegionDraw d{0u, false, false, false, false};
    if (ix64 >= a.n_draw) return d;
    const uint32_t ix = (uint32_t)ix64;
    const uint32_t tag = a.draw_tags[ix];
    d.paint = pick_is_paint(tag);
    const bool begin = tag == DRAWTAG_BEGIN_CLIP, end = tag == DRAWTAG_END_CLIP;
    if (d.paint || begin || end) {
        const uint32_t path_ix = a.draw_monoids[ix].path_ix;
        if (path_ix < a.n_paths) {  // (an EndClip nothing matched keeps an index of its own: it may be n_paths)
            const PathBbox bb = a.path_bboxes[path_ix];
            const uint32_t wn = region_winding(a)[path_ix];
            const bool hit = (bb.draw_flags & DRAW_INFO_FLAGS_FILL_RULE_BIT) != 0u ? (wn & 1u) != 0u : wn != 0u;
            d.touch = hit || region_meets(a)[path_ix] != 0u;
            // (i32 and f32 are both exact in f64)
            d.boxed = (double)a.r.x0 <= (double)bb.x0 && (double)bb.x1 <= (double)a.r.x1 && (double)a.r.y0 <= (double)bb.y0 && (double)bb.y1 <= (double)a.r.y1;
            d.nonempty = bb.x0 < bb.x1 && bb.y0 < bb.y1;
        }
    }
    d.v = begin && !d.touch ? 1u : end && !d.touch ? 0xffffffffu : 0u;
    return d;
}

// adds the number of lanes of the wave for which `p` holds to *cell (one atomic per wave, none for an empty one)
__device__ __forceinline__ void region_count(bool p, uint32_t *cell, uint32_t lane) {
    const unsigned long long m = __ballot(p);
    if (lane == 0u && m != 0ull) atomicAdd(cell, (uint32_t)__popcll(m));
}

}  // namespace

// k_region_lines: rule 1, MEETS of every path and its winding at C.  A workgroup per REGION_LINES_CHUNK lines of the soup, a lane per
// line.  R' and C are arguments: wave-uniform.  The f32 box test against R' and the pick's two half-open y tests against cy run first
// -- promotion to f64 is exact, so they are the contract's -- and the f64 products are under a branch that a wave with no survivor
// jumps over.  For a small marquee that is almost every wave; for a large one most lines of the soup pass the box test and meet R',
// and an atomic per line would queue up on the few words of the large paths.  The soup is largely ordered by path, so a lane ORs its
// path's word only where the lane to its left within its row of 16 (one DPP row shift) does not OR the same word: a run of lines of
// one path issues one atomic per row (the whole-target marquee on the headline scene: 19 us against 204 us with an atomic per line,
// profiles/pick_rect.txt).  A line the ray from C crosses adds +1 or -1 (wrapping) to its path's winding word as
// k_pick_lines does.  d is formed in f64 without contraction (the translation unit is compiled with -ffp-contract=off): per corner
// two differences, two products, one difference, each rounded on its own -- the corners share the differences and the products, which
// rounds nothing differently.
__global__ void __launch_bounds__(256) k_region_lines(RegionArgs a) {
    const uint32_t tid = threadIdx.x;
    const uint32_t ix = blockIdx.x * REGION_LINES_CHUNK + tid;
    LineSoup l{};
    bool counted = false;
    if (ix < a.n_lines) {
        l = pick_load_line(a.lines, ix);
        counted = l.path_ix < a.n_paths;
    }
    const Region r = a.r;
    const bool box = counted && region_lo(l.p0x, l.p1x) < r.x1 && region_hi(l.p0x, l.p1x) > r.x0 && region_lo(l.p0y, l.p1y) < r.y1 &&
                     region_hi(l.p0y, l.p1y) > r.y0;
    const bool up = counted && l.p0y <= r.cy && r.cy < l.p1y;
    const bool down = counted && l.p1y <= r.cy && r.cy < l.p0y;
    bool meets = false;
    if (box || up || down) {
        const double p0x = (double)l.p0x, p0y = (double)l.p0y;
        const double ex = (double)l.p1x - p0x, ey = (double)l.p1y - p0y;
        if (box) {
            const double ax = ex * ((double)r.y0 - p0y), bx = ex * ((double)r.y1 - p0y);
            const double ay = ((double)r.x0 - p0x) * ey, by = ((double)r.x1 - p0x) * ey;
            const double d00 = ax - ay, d10 = ax - by, d01 = bx - ay, d11 = bx - by;  // (x0, y0), (x1, y0), (x0, y1), (x1, y1)
            const bool all_pos = d00 > 0.0 && d10 > 0.0 && d01 > 0.0 && d11 > 0.0;
            const bool all_neg = d00 < 0.0 && d10 < 0.0 && d01 < 0.0 && d11 < 0.0;
            meets = !all_pos && !all_neg;
        }
        if (up || down) {
            const double d = ex * ((double)r.cy - p0y) - ((double)r.cx - p0x) * ey;
            uint32_t *cell = region_winding(a) + l.path_ix;
            if (up && d < 0.0) atomicAdd(cell, 1u);
            if (down && d > 0.0) atomicAdd(cell, 0xffffffffu);
        }
    }
    // (every lane of the wave is here: the row shift reads lanes, not survivors)
    const uint32_t key = meets ? l.path_ix : 0xffffffffu;
    const uint32_t left = row_shr<1>(key);  // (unspecified in the first lane of a row)
    const bool first = (tid & 15u) == 0u || left != key;
    if (meets && first) atomicOr(region_meets(a) + l.path_ix, 1u);
}

// The draw pass, rule 2, a lane per draw object across as many workgroups as it takes.  The clip stack of the contract is its
// prefix-sum form as in k_pick_resolve: a paint draw qualifies when the exclusive prefix of the terms before it is 0.  The carry
// between workgroups is made by two launches instead of one workgroup's walk or a look-back: k_region_draw_totals leaves each
// chunk's sum, k_region_draws adds up the sums of the chunks before its own (a strided read and one workgroup scan) and then scans
// its own chunk again -- the terms are a tag, a monoid and three scratch words away, cheaper to recompute than to store.
__global__ void __launch_bounds__(256) k_region_draw_totals(RegionArgs a) {
    __shared__ uint32_t sh_scan[4];
    const RegionDraw d = region_draw(a, (uint64_t)blockIdx.x * REGION_DRAW_CHUNK + threadIdx.x);
    uint32_t total;
    (void)block256_incl_scan_u32(d.v, sh_scan, &total);
    if (threadIdx.x == 0u) region_totals(a)[blockIdx.x] = total;
}

// A TOUCHED draw writes its word (every other live lane writes 0) and, in a frame composed from instances, finds its owner by the
// pick's binary search -- the last entry of the prefix that is <= its index -- and ORs its bits into the owner's scratch word; so does
// a paint draw with a non-empty path box that is not ENCLOSED (REGION_NOT_ALL: rule 3's second condition).
__global__ void __launch_bounds__(256) k_region_draws(RegionArgs a) {
    __shared__ uint32_t sh_scan[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t ix64 = (uint64_t)blockIdx.x * REGION_DRAW_CHUNK + tid;
    uint32_t before = 0u, carry;
    for (uint32_t j = tid; j < blockIdx.x; j += 256u) before += region_totals(a)[j];
    (void)block256_incl_scan_u32(before, sh_scan, &carry);
    const RegionDraw d = region_draw(a, ix64);
    uint32_t total;
    const uint32_t incl = block256_incl_scan_u32(d.v, sh_scan, &total);
    const bool touched = d.paint && d.touch && carry + (incl - d.v) == 0u;
    const bool enclosed = touched && d.boxed;
    const uint32_t word = (touched ? REGION_TOUCHED : 0u) | (enclosed ? REGION_ENCLOSED : 0u);
    const bool live = ix64 < a.n_draw;
    const uint32_t ix = (uint32_t)ix64;
    if (live && a.draws_out != nullptr) a.draws_out[ix] = word;
    const uint32_t bits = word | (d.paint && d.nonempty && !enclosed ? REGION_NOT_ALL : 0u);
    if (bits != 0u && a.n_inst != 0u) {
        uint32_t lo = 0u, hi = a.n_inst - 1u;  // empty instances repeat an offset, the last of a run holds the draw
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (a.prefix[mid] <= ix) lo = mid;
            else hi = mid - 1u;
        }
        atomicOr(region_inst(a) + lo, bits);
    }
    region_count(touched, region_counts(a) + 0, tid & 63u);
    region_count(enclosed, region_counts(a) + 1, tid & 63u);
}

// k_region_instances: rule 3, a lane per instance: its scratch word to its two bits, and the instances' two counts.
__global__ void __launch_bounds__(256) k_region_instances(RegionArgs a) {
    const uint32_t tid = threadIdx.x;
    const uint64_t k = (uint64_t)blockIdx.x * 256u + tid;
    const uint32_t s = k < a.n_inst ? region_inst(a)[k] : 0u;
    const bool touched = (s & REGION_TOUCHED) != 0u;
    const bool enclosed = (s & REGION_ENCLOSED) != 0u && (s & REGION_NOT_ALL) == 0u;
    if (k < a.n_inst && a.instances_out != nullptr) a.instances_out[k] = (touched ? REGION_TOUCHED : 0u) | (enclosed ? REGION_ENCLOSED : 0u);
    region_count(touched, region_counts(a) + 2, tid & 63u);
    region_count(enclosed, region_counts(a) + 3, tid & 63u);
}

void launch_region_lines(const RegionArgs &a, hipStream_t s) {
    const uint32_t wgs = (uint32_t)(((uint64_t)a.n_lines + REGION_LINES_CHUNK - 1u) / REGION_LINES_CHUNK);
    if (wgs == 0u || a.n_paths == 0u) return;
    hipLaunchKernelGGL(k_region_lines, dim3(wgs), dim3(256), 0, s, a);
}

void launch_region_draws(const RegionArgs &a, hipStream_t s) {
    const uint32_t wgs = region_draw_chunks(a.n_draw);
    if (wgs == 0u) return;
    hipLaunchKernelGGL(k_region_draw_totals, dim3(wgs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_region_draws, dim3(wgs), dim3(256), 0, s, a);
}

void launch_region_instances(const RegionArgs &a, hipStream_t s) {
    const uint32_t wgs = (uint32_t)(((uint64_t)a.n_inst + 255u) / 256u);
    if (wgs == 0u) return;
    hipLaunchKernelGGL(k_region_instances, dim3(wgs), dim3(256), 0, s, a);
}

}  // namespace vk

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
using namespace vk;

static_assert(REGION_TOUCHED == VELLO_HIP_REGION_TOUCHED && REGION_ENCLOSED == VELLO_HIP_REGION_ENCLOSED && sizeof(vello_hip_region_counts) == 16,
              "k_region_draws and k_region_instances write the header's bits and its counts");

extern "C" {

int vello_hip_pick_rect_sizes(vello_hip_ctx *c, uint32_t *n_draws_out, uint32_t *n_instances_out) {
    if (!c) return VELLO_HIP_E_INVALID;
    QueryFrame qf;
    if (const char *why = query_frame(c, qf)) {
        c->last_error = std::string("pick_rect_sizes: ") + why;
        return VELLO_HIP_E_INVALID;
    }
    if (n_draws_out) *n_draws_out = qf.lane->frame_cfg.layout.n_draw_objects;
    if (n_instances_out) *n_instances_out = qf.n_inst;
    return VELLO_HIP_OK;
}

int vello_hip_pick_rect(vello_hip_ctx *c, const float rect[4], uint32_t *draws_out, uint32_t n_draws, uint32_t *instances_out, uint32_t n_instances,
                        int out_is_device, vello_hip_region_counts *counts_out) {
    if (!c) return VELLO_HIP_E_INVALID;
    auto refuse = [&](const std::string &why) {
        c->last_error = "pick_rect: " + why;
        return VELLO_HIP_E_INVALID;
    };
    if (!rect) return refuse("rect is NULL");
    if (!draws_out && !instances_out && !counts_out) return refuse("draws_out, instances_out and counts_out are all NULL");
    QueryFrame qf;
    if (const char *why = query_frame(c, qf)) return refuse(why);
    Lane &l = *qf.lane;
    const Config &cfg = l.frame_cfg;
    const uint32_t n_draw = cfg.layout.n_draw_objects, n_inst = qf.n_inst;
    if (draws_out && n_draws != n_draw) return refuse("n_draws is " + std::to_string(n_draws) + ", the frame has " + std::to_string(n_draw) + " draw objects");
    if (instances_out && n_inst == 0u) return refuse("instances_out on a frame that has no instances");
    if (instances_out && n_instances != n_inst) return refuse("n_instances is " + std::to_string(n_instances) + ", the frame has " + std::to_string(n_inst) + " instances");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t draw_bytes = (size_t)n_draw * 4u, inst_bytes = (size_t)n_inst * 4u;
    if (out_is_device) {
        if (draws_out)
            if (const char *why = not_device_memory(c, draws_out, draw_bytes)) return refuse(std::string("the address of device draws_out ") + why);
        if (instances_out)
            if (const char *why = not_device_memory(c, instances_out, inst_bytes)) return refuse(std::string("the address of device instances_out ") + why);
    }

    hipStream_t st = l.stream;
    Bump bump;
    if (int r = judge_frame(c, "pick_rect", l, bump)) return r;
    c->pick_ms = 0.f;

    RegionArgs a{};
    vello_hip_region_counts counts{};
    if (!region_of(rect, cfg.target_width, cfg.target_height, a.r)) {  // an empty R' selects nothing
        if (out_is_device) {
            if (draws_out && draw_bytes) HIP_TRY(c, hipMemsetAsync(draws_out, 0, draw_bytes, st));
            if (instances_out) HIP_TRY(c, hipMemsetAsync(instances_out, 0, inst_bytes, st));
            HIP_TRY(c, hipStreamSynchronize(st));
        } else {
            if (draws_out) memset(draws_out, 0, draw_bytes);
            if (instances_out) memset(instances_out, 0, inst_bytes);
        }
        if (counts_out) *counts_out = counts;
        return VELLO_HIP_OK;
    }

    const SceneSlot &sc = *qf.scene;
    a.lines = (const LineSoup *)l.buf[VELLO_HIP_BUF_LINES].ptr;
    a.n_lines = bump.lines < cfg.lines_size ? bump.lines : cfg.lines_size;
    a.n_paths = cfg.layout.n_paths;
    a.n_draw = n_draw;
    a.n_inst = n_inst;
    a.draw_tags = (const uint32_t *)sc.scene.ptr + cfg.layout.draw_tag_base;
    a.draw_monoids = (const DrawMonoid *)l.buf[VELLO_HIP_BUF_DRAW_MONOIDS].ptr;
    a.path_bboxes = (const PathBbox *)l.buf[VELLO_HIP_BUF_PATH_BBOXES].ptr;
    a.prefix = qf.prefix;
    int r;
    if ((r = ensure(c, c->region_scratch, region_scratch_words(a.n_paths, n_inst, n_draw) * 4u))) return r;
    a.scratch = (uint32_t *)c->region_scratch.ptr;
    const bool staged = !out_is_device && (draws_out || instances_out);
    if (staged && (r = ensure(c, c->region_out, draw_bytes + inst_bytes))) return r;
    uint32_t *stage_draws = (uint32_t *)c->region_out.ptr, *stage_inst = stage_draws + n_draw;
    a.draws_out = !draws_out ? nullptr : out_is_device ? draws_out : stage_draws;
    a.instances_out = !instances_out ? nullptr : out_is_device ? instances_out : stage_inst;
    // with profiling on (vello_hip_set_profiling, any stage): two events around the launches, read by vello_hip_pick_ms
    const bool prof = c->prof_mask != 0u;
    hipEvent_t ev_a = prof ? get_event(c) : nullptr, ev_b = prof ? get_event(c) : nullptr;
    if (prof) HIP_TRY(c, hipEventRecord(ev_a, st));
    // (the chunk sums behind the counts are all written before they are read)
    HIP_TRY(c, hipMemsetAsync(a.scratch, 0, (2u * (size_t)a.n_paths + n_inst + 4u) * 4u, st));
    launch_region_lines(a, st);
    HIP_TRY(c, hipGetLastError());
    launch_region_draws(a, st);
    HIP_TRY(c, hipGetLastError());
    launch_region_instances(a, st);
    HIP_TRY(c, hipGetLastError());
    if (prof) HIP_TRY(c, hipEventRecord(ev_b, st));
    if (!out_is_device) {
        if (draws_out && draw_bytes) HIP_TRY(c, hipMemcpyAsync(draws_out, stage_draws, draw_bytes, hipMemcpyDeviceToHost, st));
        if (instances_out) HIP_TRY(c, hipMemcpyAsync(instances_out, stage_inst, inst_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipMemcpyAsync(&counts, a.scratch + 2u * (size_t)a.n_paths + n_inst, sizeof counts, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (prof) {
        (void)hipEventElapsedTime(&c->pick_ms, ev_a, ev_b);
        c->event_pool.push_back(ev_a);
        c->event_pool.push_back(ev_b);
    }
    if (counts_out) *counts_out = counts;
    return VELLO_HIP_OK;
}

}  // extern "C"
