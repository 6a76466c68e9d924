"""common.h's floating-point rules on the host: the g++ twin of tests/device_checks/math.hip (the same sincos_cr, atan2_cr,
pow_cr ... through the emulator's hip_runtime.h shim) against the oracle's own vo_sinf ... vo_expf and plain f32 arithmetic
(tests/math_ref.c), on the input set the device test uses (tests/math_rules.py).

In this build ocml's names are glibc's, so what is checked here without a GPU is the project's own code: the routing conditions
(|x| <= 512, x > 0 && |y| <= x / 64, x > 0 && x < inf && |y| <= 8), atan2_cr's Taylor path, f64::sincos_medium and
f64::pow_pos at the routing edges, and that the host twin keeps the plain rules.  tests/test_gpu_math_rules.py asks the same
of the gfx950 build.  The reference itself is pinned against a 200-bit evaluation where mpmath is installed."""
import numpy as np
import pytest

from tests import math_rules as M


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    return M.Reference(tmp_path_factory.mktemp("math_ref"))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return M.build_host_twin(tmp_path_factory.mktemp("math_twin"))


@pytest.mark.parametrize("fn", M.F32_FUNCTIONS)
def test_host_twin_equals_oracle(fn, twin, reference):
    a, b = M.inputs(fn)
    assert len(a) >= M.N_RANDOM
    want, hard = reference(fn)
    got = twin.f32_bits(fn, a, b)
    wrong, far = M.mismatches(got, want, hard)
    assert len(wrong) == 0, M.describe(fn, wrong, got, want)
    assert len(far) == 0, "hard-flagged, but more than one ulp apart: " + M.describe(fn, far, got, want)


def test_hard_flags_stay_within_the_cap(reference):
    # a condition on the committed seeds, not a measurement: 2^-50 of each side of a midpoint is ~2^-26 of all values,
    # so a quarter of a million samples expect ~0.004 flags per function; the plain rules never flag
    counts = {fn: int(reference(fn)[1].sum()) for fn in M.F32_FUNCTIONS}
    assert all(c <= M.MAX_HARD for c in counts.values()), counts
    assert all(counts[fn] == 0 for fn in M.F32_FUNCTIONS if fn not in M.TRANSCENDENTALS), counts


@pytest.mark.parametrize("fn", M.F64_FUNCTIONS)
def test_own_fp64_kernels_stay_within_two_ulps(fn, twin, reference):
    # The f32 comparison above cannot see an fp64 error of a few ulps (it moves ~2^-27 of the f32 results), yet the hard flag's
    # window of 2^-50 is only wide enough for implementations within 2 fp64 ulps (what ocml documents and what
    # tests/test_fp64_math.py asks of its own sweep).  The device returns these very bits (test_gpu_math_rules.py), so the
    # bound holds there too.  Dropping pow_pos's z_lo term gives 4.0 ulps on this set.
    a, b = M.f64_inputs(fn)
    err = reference.f64_error_ulps(fn, a, b, twin.f64_bits(fn, a, b))
    worst = int(np.argmax(err))
    assert err[worst] < 2.0, f"{fn}: {err[worst]:.3f} fp64 ulps at a={a[worst]!r} b={b[worst]!r}; {int((err >= 2.0).sum())} of {len(a)} samples at 2 or more"


def _correctly_rounded_f32(values):
    """200-bit mpmath values -> f32 bit patterns by ONE rounding to nearest-even.  Through fp64 first (vectorised), and exactly
    wherever the fp64 value is itself an f32 midpoint or overflows, the only cases in which two roundings differ from one."""
    import mpmath

    def exact(v):
        if v == 0:
            return np.float32(0)
        m, e = mpmath.frexp(abs(v))                                    # |v| = m 2^e, 0.5 <= m < 1
        q = max(int(e) - 24, -149)                                     # the f32 quantum at |v| is 2^q
        n = int(mpmath.nint(mpmath.ldexp(abs(v), -q)))                 # nint rounds ties to even; the scaling is exact
        r = np.ldexp(np.float64(n), q)
        return np.float32(np.inf if r >= 2.0 ** 128 else r) * np.float32(1 if v > 0 else -1)

    d = np.array([float(v) if abs(v) < mpmath.mpf(2) ** 1000 else np.copysign(np.inf, float(mpmath.sign(v))) for v in values])
    with np.errstate(over="ignore"):
        f = d.astype(np.float32)
    # where the fp64 value is a tie between two f32 values (or beyond fp64's finite range), the 200-bit value decides
    lo, hi = np.nextafter(f, np.float32(-np.inf)).astype(np.float64), np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tie = (d == (f.astype(np.float64) + lo) / 2) | (d == (f.astype(np.float64) + hi) / 2) | ~np.isfinite(d) | (np.abs(d) >= 2.0 ** 127)
    for i in np.flatnonzero(tie & (d != f.astype(np.float64))):
        f[i] = exact(values[i])
    return f.view(np.uint32)


@pytest.mark.parametrize("fn", M.TRANSCENDENTALS)
def test_oracle_is_the_correctly_rounded_value(fn, reference):
    mpmath = pytest.importorskip("mpmath")
    a, b = M.inputs(fn)
    want, hard = reference(fn)
    # finite arguments inside the function's real domain (mpmath has no signed zeros, infinities or C's special cases: those are
    # glibc's by definition and the device is held to them in test_gpu_math_rules.py); hard samples are exactly where the
    # fp64 value rounded once may miss the correctly rounded one
    ok = np.isfinite(a) & np.isfinite(b) & ~hard
    if fn in ("asin", "acos"):
        ok &= np.abs(a) <= 1
    if fn == "pow":
        ok &= a > 0
    if fn == "atan2":
        ok &= (a != 0) | (b > 0)
    idx = np.flatnonzero(ok)
    idx = np.sort(np.random.default_rng(2024).choice(idx, 1 << 15, replace=False))
    f = {"sin": mpmath.sin, "cos": mpmath.cos, "asin": mpmath.asin, "acos": mpmath.acos, "exp": mpmath.exp}
    with mpmath.workprec(200):
        if fn == "atan2":
            values = [mpmath.atan2(mpmath.mpf(float(y)), mpmath.mpf(float(x))) for y, x in zip(a[idx], b[idx])]
        elif fn == "pow":
            values = [mpmath.power(mpmath.mpf(float(x)), mpmath.mpf(float(y))) for x, y in zip(a[idx], b[idx])]
        else:
            values = [f[fn](mpmath.mpf(float(x))) for x in a[idx]]
        exact = _correctly_rounded_f32(values)
    got = want[idx]
    zero = ((got | exact) & 0x7FFFFFFF) == 0                         # (the sign of a zero is C's rule, not a rounding)
    wrong = np.flatnonzero((got != exact) & ~zero)
    assert len(wrong) == 0, M.describe(fn, idx[wrong], exact_full(exact, idx, len(a)), want)


def exact_full(exact, idx, n):
    full = np.zeros(n, dtype=np.uint32)
    full[idx] = exact
    return full
