/* TEST-ONLY: the reference of tests/test_math_rules.py and tests/test_gpu_math_rules.py.  It includes the oracle's own
 * vo_internal.h, so the transcendentals ARE vo_sinf ... vo_expf (glibc's fp64 value rounded once) and the plain f32 rules
 * are the oracle's vdot / vlen / vnorm / vo_round / vo_span, compiled with the oracle's flags (-ffp-contract=off
 * -fno-fast-math -mfma; tests/math_rules.py builds it at test time).  Function numbers and the sample layout are those of
 * tests/device_checks/math.hip.
 *
 * hard[i] is set when the long double value of the function (64 mantissa bits) lies within 2^-50 (relative) of the midpoint
 * between two adjacent f32 values: the only place where two honest "fp64 value rounded once" implementations may differ
 * (glibc stays under 1 fp64 ulp, ocml is documented at no more than 2). */
#include "vo_internal.h"
#include <float.h>

enum { FN_SIN, FN_COS, FN_ATAN2, FN_ASIN, FN_ACOS, FN_POW, FN_EXP,
       FN_DOT, FN_LENGTH, FN_NORMALIZE_X, FN_NORMALIZE_Y, FN_XF_APPLY_X, FN_XF_APPLY_Y, FN_ROUND_TE, FN_SPAN, FN_COUNT };

/* flatten.wgsl:668-672, as oracle/vo_front.c spells it (a static function there) */
static vec2 xf_apply(const vo_xform *t, vec2 p) {
    float px = fmaf(t->m[0], p.x, fmaf(t->m[2], p.y, t->t[0]));
    float py = fmaf(t->m[1], p.x, fmaf(t->m[3], p.y, t->t[1]));
    return v2(px, py);
}

static int near_f32_midpoint(long double v) {
    if (!(fabsl(v) <= LDBL_MAX) || v == 0.0L) return 0; /* NaN, inf and exact zeros have no rounding to argue about */
    const long double av = fabsl(v), tol = av * 0x1p-50L;
    const long double overflow = 0x1.ffffffp127L; /* FLT_MAX + ulp/2: the midpoint between FLT_MAX and inf */
    const float f = (float)av;                    /* round to nearest */
    if (isinf(f)) return fabsl(av - overflow) <= tol;
    const float hi = nextafterf(f, INFINITY);
    const long double up = isinf(hi) ? overflow : ((long double)f + (long double)hi) * 0.5L;
    if (fabsl(av - up) <= tol) return 1;
    if (f > 0.0f && fabsl(av - ((long double)f + (long double)nextafterf(f, 0.0f)) * 0.5L) <= tol) return 1;
    return 0;
}

/* err_ulps[i] = distance, in fp64 ulps of the long double value, between the fp64 result bits64[i] of f64::sincos_medium's s (0)
 * or c (1) or of f64::pow_pos (2) at (a[i], b[i]) and that value; results in or below the fp64 denormals are not measured (0). */
int f64_error_ulps(uint32_t fn, const float *a, const float *b, uint32_t n, const uint64_t *bits64, double *err_ulps) {
    if (fn > 2u) return -1;
    for (uint32_t i = 0; i < n; i++) {
        double got;
        memcpy(&got, &bits64[i], 8);
        const long double v = fn == 0u ? sinl((long double)a[i]) : fn == 1u ? cosl((long double)a[i]) : powl((long double)a[i], (long double)b[i]);
        int e;
        (void)frexpl(v, &e); /* |v| in [2^(e-1), 2^e): one fp64 ulp is 2^(e-53) */
        if (v == 0.0L)
            err_ulps[i] = got == 0.0 ? 0.0 : HUGE_VAL;
        else if (e < -1020 || e > 1023) /* beyond fp64's normal range (pow_pos of an f32 reaches 2^+-1192) */
            err_ulps[i] = 0.0;
        else
            err_ulps[i] = (double)ldexpl(fabsl((long double)got - v), 53 - e);
    }
    return 0;
}

int math_ref(uint32_t fn, const float *a, const float *b, uint32_t n, uint32_t *out_bits, uint8_t *hard) {
    if (fn >= FN_COUNT) return -1;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t i1 = (i + 1u) % n, i2 = (i + 2u) % n, i3 = (i + 3u) % n;
        const float x = a[i], y = b[i];
        const vo_xform t = {{x, y, a[i1], b[i1]}, {a[i2], b[i2]}};
        float r = 0.0f;
        long double v = 0.0L; /* stays 0 for the plain rules: they are exact definitions, never hard */
        switch (fn) {
            case FN_SIN: r = vo_sinf(x); v = sinl((long double)x); break;
            case FN_COS: r = vo_cosf(x); v = cosl((long double)x); break;
            case FN_ATAN2: r = vo_atan2f(x, y); v = atan2l((long double)x, (long double)y); break;
            case FN_ASIN: r = vo_asinf(x); v = asinl((long double)x); break;
            case FN_ACOS: r = vo_acosf(x); v = acosl((long double)x); break;
            case FN_POW: r = vo_powf(x, y); v = powl((long double)x, (long double)y); break;
            case FN_EXP: r = vo_expf(x); v = expl((long double)x); break;
            case FN_DOT: r = vdot(v2(x, y), v2(a[i1], b[i1])); break;
            case FN_LENGTH: r = vlen(v2(x, y)); break;
            case FN_NORMALIZE_X: r = vnorm(v2(x, y)).x; break;
            case FN_NORMALIZE_Y: r = vnorm(v2(x, y)).y; break;
            case FN_XF_APPLY_X: r = xf_apply(&t, v2(a[i3], b[i3])).x; break;
            case FN_XF_APPLY_Y: r = xf_apply(&t, v2(a[i3], b[i3])).y; break;
            case FN_ROUND_TE: r = vo_round(x); break;
            default: break;
        }
        out_bits[i] = fn == FN_SPAN ? vo_span(x, y) : f2bits(r);
        hard[i] = (uint8_t)near_f32_midpoint(v);
    }
    return 0;
}
