// TEST-ONLY device check of common.h's floating-point half: the f32 transcendentals (sincos_cr, atan2_cr, asin_cr, acos_cr,
// pow_cr, exp_cr -- fp64_math.h's own kernels, ocml's fp64 routines and the routing between them), fp64_math.h's fp64 results
// themselves, and the plain f32 rules (no contraction in dot, fmaf only in xf_apply, correctly rounded sqrtf and / in length
// and normalize, rintf ties-to-even, span, denormals kept).  In the SIMT-emulated build ocml's names resolve to glibc, the
// very functions the CPU oracle calls, so only a device run sees what ships; tests/test_gpu_math_rules.py compares the bits
// that come back with the oracle's own vo_sinf ... vo_expf (tests/math_ref.c).
//
// The same file is the HOST TWIN: `g++ -x c++ -DVELLO_SIMT_EMU -I tests/simt_emu` compiles it through the emulator's
// hip_runtime.h shim, the two entry points then loop on the CPU over the same apply_f32 / apply_f64.  tests/math_rules.py
// builds that at test time; its fp64 results are what the device's must equal bit for bit.
//
// A sample is (a[i], b[i]); the functions of more than two arguments also read the samples after it (indices wrap at n):
//   dot        a . b with a = (a[i], b[i]), b = (a[i+1], b[i+1])
//   length / normalize   of (a[i], b[i])
//   xf_apply   the transform {a[i], b[i], a[i+1], b[i+1], a[i+2], b[i+2]} applied to the point (a[i+3], b[i+3])
// Every argument comes from memory, so no call can be folded.  Built into libvello_devcheck.so beside primitives.hip.
#include "../../vello_amd/csrc/engine/common.h"

namespace {

enum MathFn : uint32_t {
    FN_SIN, FN_COS, FN_ATAN2, FN_ASIN, FN_ACOS, FN_POW, FN_EXP,                                  // f(a) or f(a, b); atan2_cr(y = a, x = b)
    FN_DOT, FN_LENGTH, FN_NORMALIZE_X, FN_NORMALIZE_Y, FN_XF_APPLY_X, FN_XF_APPLY_Y, FN_ROUND_TE, FN_SPAN,
    FN_COUNT
};
enum F64Fn : uint32_t { F64_SINCOS_S, F64_SINCOS_C, F64_POW_POS, F64_COUNT };

// flatten.hip:142 (flatten.wgsl:668-672), restated: flatten.hip is a kernel source and cannot be included
__device__ __forceinline__ vk::vec2 xf_apply(const vk::Xform &t, vk::vec2 p) {
    float px = fmaf(t.m0, p.x, fmaf(t.m2, p.y, t.t0));
    float py = fmaf(t.m1, p.x, fmaf(t.m3, p.y, t.t1));
    return vk::v2(px, py);
}

__device__ inline uint32_t apply_f32(uint32_t fn, const float *a, const float *b, uint32_t n, uint32_t i) {
    const uint32_t i1 = (i + 1u) % n, i2 = (i + 2u) % n, i3 = (i + 3u) % n;
    const float x = a[i], y = b[i];
    float r = 0.0f;
    switch (fn) {
        case FN_SIN: { float s, c; vk::sincos_cr(x, s, c); r = s; break; }   // as the flattener calls them: one sincos_cr
        case FN_COS: { float s, c; vk::sincos_cr(x, s, c); r = c; break; }
        case FN_ATAN2: r = vk::atan2_cr(x, y); break;
        case FN_ASIN: r = vk::asin_cr(x); break;
        case FN_ACOS: r = vk::acos_cr(x); break;
        case FN_POW: r = vk::pow_cr(x, y); break;
        case FN_EXP: r = vk::exp_cr(x); break;
        case FN_DOT: r = vk::dot(vk::v2(x, y), vk::v2(a[i1], b[i1])); break;
        case FN_LENGTH: r = vk::length(vk::v2(x, y)); break;
        case FN_NORMALIZE_X: r = vk::normalize(vk::v2(x, y)).x; break;
        case FN_NORMALIZE_Y: r = vk::normalize(vk::v2(x, y)).y; break;
        case FN_XF_APPLY_X: r = xf_apply(vk::Xform{x, y, a[i1], b[i1], a[i2], b[i2]}, vk::v2(a[i3], b[i3])).x; break;
        case FN_XF_APPLY_Y: r = xf_apply(vk::Xform{x, y, a[i1], b[i1], a[i2], b[i2]}, vk::v2(a[i3], b[i3])).y; break;
        case FN_ROUND_TE: r = vk::roundf_te(x); break;
        case FN_SPAN: return vk::span(x, y);
        default: break;
    }
    return __float_as_uint(r);
}

// the caller keeps the arguments inside the documented domains: |a| <= SINCOS_MAX_ARG; a > 0 finite and |b| <= 8
__device__ inline unsigned long long apply_f64(uint32_t fn, float a, float b) {
    double r;
    if (fn == F64_POW_POS) {
        r = vk::f64::pow_pos((double)a, (double)b);
    } else {
        double s, c;
        vk::f64::sincos_medium((double)a, s, c);
        r = fn == F64_SINCOS_S ? s : c;
    }
    return (unsigned long long)__double_as_longlong(r);
}

#ifndef VELLO_SIMT_EMU
// grid-stride loops over exactly n samples
__global__ void __launch_bounds__(256) k_math(uint32_t fn, const float *a, const float *b, uint32_t n, uint32_t *out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = apply_f32(fn, a, b, n, i);
}
__global__ void __launch_bounds__(256) k_f64(uint32_t fn, const float *a, const float *b, uint32_t n, unsigned long long *out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = apply_f64(fn, a[i], b[i]);
}

// host arrays in, host array out; `wide` selects the fp64 kernel and 8-byte results
int run_on_device(bool wide, uint32_t fn, const float *a, const float *b, uint32_t n, void *out) {
    const size_t in_bytes = (size_t)n * sizeof(float), out_bytes = (size_t)n * (wide ? 8u : 4u);
    float *d_a = nullptr, *d_b = nullptr;
    void *d_out = nullptr;
    hipError_t e = hipMalloc((void **)&d_a, in_bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&d_b, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_a, a, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_b, b, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_out, 0, out_bytes);
    if (e == hipSuccess) {
        const uint32_t blocks = (n + 255u) / 256u < 1024u ? (n + 255u) / 256u : 1024u;
        if (wide)
            hipLaunchKernelGGL(k_f64, dim3(blocks), dim3(256), 0, 0, fn, d_a, d_b, n, (unsigned long long *)d_out);
        else
            hipLaunchKernelGGL(k_math, dim3(blocks), dim3(256), 0, 0, fn, d_a, d_b, n, (uint32_t *)d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_a);
    (void)hipFree(d_b);
    (void)hipFree(d_out);
    return (int)e;
}
#endif

}  // namespace

// out_bits[i] = the raw f32 bits (span: the u32) of function `fn` (MathFn) at sample i.  Returns 0 when the function ran,
// -1 for an unknown function, a hipError_t otherwise.
extern "C" int vello_devcheck_math(uint32_t fn, const float *a, const float *b, uint32_t n, uint32_t *out_bits) {
    if (fn >= FN_COUNT) return -1;
    if (n == 0) return 0;
#ifdef VELLO_SIMT_EMU
    for (uint32_t i = 0; i < n; i++) out_bits[i] = apply_f32(fn, a, b, n, i);
    return 0;
#else
    return run_on_device(false, fn, a, b, n, out_bits);
#endif
}

// out_bits64[i] = the raw fp64 bits of f64::sincos_medium's s or c at (double)a[i], or of f64::pow_pos((double)a[i], (double)b[i])
extern "C" int vello_devcheck_f64(uint32_t fn, const float *a, const float *b, uint32_t n, unsigned long long *out_bits64) {
    if (fn >= F64_COUNT) return -1;
    if (n == 0) return 0;
#ifdef VELLO_SIMT_EMU
    for (uint32_t i = 0; i < n; i++) out_bits64[i] = apply_f64(fn, a[i], b[i]);
    return 0;
#else
    return run_on_device(true, fn, a, b, n, out_bits64);
#endif
}
