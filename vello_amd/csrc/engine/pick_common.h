// What the kernels of the two queries on a finished frame share (vello_hip_pick: pick.hip, vello_hip_pick_rect: pick_rect.hip).
#pragma once
#include "common.h"

namespace vk {

// A LineSoup record (24 B, 8-byte aligned) as three 8-byte loads, as k_path_count reads it (path.hip load_line).
struct __attribute__((aligned(8))) PickWords2 { uint32_t a, b; };
__device__ __forceinline__ LineSoup pick_load_line(const LineSoup *__restrict__ lines, uint32_t ix) {
    const PickWords2 *p = reinterpret_cast<const PickWords2 *>(lines + ix);
    const PickWords2 w0 = p[0], w1 = p[1], w2 = p[2];
    LineSoup l;
    l.path_ix = w0.a; l.pad = w0.b;
    l.p0x = __uint_as_float(w1.a); l.p0y = __uint_as_float(w1.b);
    l.p1x = __uint_as_float(w2.a); l.p1y = __uint_as_float(w2.b);
    return l;
}

// the draw objects a query can name: fill colour, the three gradients, image, blurred rounded rect
__device__ __forceinline__ bool pick_is_paint(uint32_t tag) {
    return tag == DRAWTAG_FILL_COLOR || tag == DRAWTAG_FILL_LIN_GRADIENT || tag == DRAWTAG_FILL_RAD_GRADIENT || tag == DRAWTAG_FILL_SWEEP_GRADIENT ||
           tag == DRAWTAG_FILL_IMAGE || tag == DRAWTAG_BLURRED_ROUNDED_RECT;
}

}  // namespace vk
