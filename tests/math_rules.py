"""Shared by tests/test_math_rules.py (CPU) and tests/test_gpu_math_rules.py (device): the seeded inputs, the oracle's reference
(tests/math_ref.c around oracle/vo_internal.h), the host twin of tests/device_checks/math.hip, and the bit comparison.

The numeric rule under test (common.h, "numeric rules"): an f32 transcendental is an fp64 evaluation rounded once to f32, which
is what the oracle computes with glibc.  Two honest implementations of that rule may differ only where the exact value sits
next to the midpoint of two f32 values; math_ref.c flags those samples ("hard", within 2^-50 relative, by long double).  The
plain f32 rules (dot, length, normalize, xf_apply, roundf_te, span) are exact definitions: no allowance anywhere."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# function numbers of tests/device_checks/math.hip and tests/math_ref.c
F32_FUNCTIONS = ["sin", "cos", "atan2", "asin", "acos", "pow", "exp",
                 "dot", "length", "normalize_x", "normalize_y", "xf_apply_x", "xf_apply_y", "roundf_te", "span"]
TRANSCENDENTALS = F32_FUNCTIONS[:7]
F64_FUNCTIONS = ["sincos_medium_s", "sincos_medium_c", "pow_pos"]
N_RANDOM = 1 << 18       # random arguments per function, beside the explicit edge lists
MAX_HARD = 4             # cap on hard-flagged samples per function (a condition of the seeds below; ~0.3 expected over all)
SEEDS = {"sincos": 1101, "atan2": 1102, "asin_acos": 1103, "pow": 1104, "exp": 1105, "plain": 1106}

f32 = np.float32
INF, NAN, FLT_MAX = f32(np.inf), f32(np.nan), np.finfo(np.float32).max
DENORM_MIN = np.uint32(1).view(f32)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=f32)


def _bits(rng, n, lo=0, hi=1 << 32):
    return rng.integers(lo, hi, n, dtype=np.uint64).astype(np.uint32).view(f32)


def _uniform(rng, lo, hi, n):
    return rng.uniform(lo, hi, n).astype(f32)


def _signs(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, f32(1), f32(-1))


def _around(values, steps=1):
    """every value with its `steps` f32 neighbours on either side"""
    out = [np.asarray(values, dtype=f32)]
    up = down = out[0]
    for _ in range(steps):
        up, down = np.nextafter(up, INF), np.nextafter(down, -INF)
        out += [up, down]
    return np.concatenate(out)


def _pairs(a_values, b_values):
    a, b = np.meshgrid(np.asarray(a_values, dtype=f32), np.asarray(b_values, dtype=f32), indexing="ij")
    return a.ravel(), b.ravel()


def _cat(parts):
    a = np.ascontiguousarray(np.concatenate([np.asarray(p[0], dtype=f32) for p in parts]))
    b = np.ascontiguousarray(np.concatenate([np.asarray(p[1], dtype=f32) for p in parts]))
    assert a.shape == b.shape
    return a, b


def _sincos_inputs():
    rng, q = np.random.default_rng(SEEDS["sincos"]), N_RANDOM // 4
    k = np.arange(0, 513, dtype=np.float64) * (np.pi / 2)      # k pi/2 rounded to f32, every k up to 512
    a = np.concatenate([
        _uniform(rng, -3.2, 3.2, q), _uniform(rng, -512, 512, q), _uniform(rng, -0.1, 0.1, q),
        _bits(rng, q),                                           # sincos_large, denormals, inf, NaN
        SPECIALS, k.astype(f32), (-k).astype(f32), _around([512.0, -512.0]), [FLT_MAX, -FLT_MAX, DENORM_MIN, -DENORM_MIN]]).astype(f32)
    return a, np.zeros_like(a)


def _atan2_inputs():
    """a = y, b = x (atan2_cr(y, x)); the fast path is x > 0 && |y| <= x / 64"""
    rng, q = np.random.default_rng(SEEDS["atan2"]), N_RANDOM // 4
    with np.errstate(all="ignore"):
        x_any = _bits(rng, q, 1, 0x7F800000)                     # any positive finite f32, denormals included
        y_fast = (x_any * _uniform(rng, -1, 1, q) / f32(64)).astype(f32)
        h = q // 2
        x_den, y_den = _bits(rng, h, 1, 0x00800000), _bits(rng, h, 1, 0x00800000) * _signs(rng, h)
        x_big = _bits(rng, q - h, 0x7E000000, 0x7F800000)        # quotients that underflow: tiny y over huge x
        y_tiny = _bits(rng, q - h, 1, 0x01000000) * _signs(rng, q - h)
        # the bound itself: |y| == 0.015625f * x exactly and one ulp to either side, for every exponent and a few mantissas
        xb = np.concatenate([np.ldexp(f32(m), np.arange(-149, 128)).astype(f32) for m in (1.0, 1.5, 1.9999999)])
        xb = xb[(xb > 0) & np.isfinite(xb)]
        yb = _around(f32(0.015625) * xb)
        xb3 = np.tile(xb, 3)
    return _cat([
        (y_fast, x_any), (_uniform(rng, -1e3, 1e3, q), _uniform(rng, -1e3, 1e3, q)), (_bits(rng, q), _bits(rng, q)),
        (y_den, x_den), (y_tiny, x_big),
        (yb, xb3), (-yb, xb3),
        _pairs(np.concatenate([SPECIALS, [1.0, -1.0, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX]]),
               np.concatenate([SPECIALS, [1.0, -1.0, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX]]))])


def _asin_acos_inputs():
    rng, h = np.random.default_rng(SEEDS["asin_acos"]), N_RANDOM // 2
    r = np.exp(rng.uniform(np.log(0.1), np.log(1e6), h)).astype(f32)
    arc = (f32(1) - f32(0.25) / r).astype(f32)                   # flatten_arc's argument, computed in f32
    near_one = (f32(1) - np.ldexp(f32(1), -np.arange(1, 25))).astype(f32)
    outside = [np.nextafter(f32(1), INF), np.nextafter(f32(-1), -INF), 2.0, -2.0]
    a = np.concatenate([_uniform(rng, -1, 1, h), arc, near_one, -near_one, SPECIALS, [1.0, -1.0], outside,
                        _bits(rng, 256, 1, 0x00800000), -_bits(rng, 256, 1, 0x00800000)]).astype(f32)
    return a, np.zeros_like(a)


# tests/fp64_math_check.cpp's exponent list
POW_EXPONENTS = np.array([2.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0, 0.5, 1.5, 1.0 / 3.0, 2.0, 7.3, -2.0 / 3.0, -8.0], dtype=f32)


def _pow_bases(rng, n):
    """the four distributions of tests/fp64_math_check.cpp, interleaved as there"""
    x = np.empty(n, dtype=f32)
    x[0::4] = np.exp(_uniform(rng, -14, 7, len(x[0::4])))        # the inverse integral's arguments, log-uniform 1e-6 ... 1e3
    x[1::4] = _uniform(rng, 0.5, 2.0, len(x[1::4]))              # around 1
    x[2::4] = _uniform(rng, 0.0, 100.0, len(x[2::4]))
    x[3::4] = _bits(rng, len(x[3::4]), 1, 0x7F800000)            # any positive f32 incl. denormals
    return x


def _pow_inputs():
    """a = x, b = y (pow_cr(x, y)); f64::pow_pos serves x > 0 && x < inf && |y| <= 8, ocml the rest"""
    rng, q = np.random.default_rng(SEEDS["pow"]), N_RANDOM // 4
    x0 = _pow_bases(rng, 2 * q)
    y0 = POW_EXPONENTS[(np.arange(2 * q) >> 2) % len(POW_EXPONENTS)]
    x1, y1 = _pow_bases(rng, q), _uniform(rng, 2, 10, q)         # the blur's 2 r1 / r0 across the routing bound ...
    x2, y2 = _uniform(rng, 0, 64, q), _uniform(rng, 2, 10, q)    # ... over pixel distances, which include 0
    x2[::16] = 0.0
    eights = _around([8.0, -8.0])
    x_special = np.concatenate([[0.0, -0.0, -2.0, -3.0, -2.5, -0.3, np.inf, -np.inf, np.nan, DENORM_MIN, FLT_MAX, 1.0, -1.0],
                                # tests/fp64_math_check.cpp's special bases (the mantissa split at sqrt(1/2), sqrt(2))
                                [1.1754944e-38, 0.70710677, 0.70710683, 1.4142135, 1.4142137, 8.0, 0.125, 0.5, 2.0, 10.0]]).astype(f32)
    y_special = np.concatenate([POW_EXPONENTS, eights, [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 2.0, 3.0, -3.0, 2.5, -2.5, 9.0, 100.0]])
    n = 4096
    with np.errstate(all="ignore"):
        edges = [
            (np.exp(_uniform(rng, -16.5, -10.5, n)), np.full(n, 8.0)),       # pow_pos into the f32 denormals and below
            (np.exp(_uniform(rng, 10.9, 11.2, n)), np.full(n, 8.0)),         # pow_pos across the f32 overflow threshold
            (np.exp(_uniform(rng, 10.9, 11.2, n)), np.full(n, -8.0)),
            (_uniform(rng, 1, 20, n), _uniform(rng, 25, 50, n)),             # ocml across the overflow threshold
            (_uniform(rng, 0.05, 1, n), _uniform(rng, 25, 50, n)),           # ocml into the denormals
            (_pow_bases(rng, n), np.tile(eights, n // len(eights) + 1)[:n])]
    return _cat([(x0, y0), (x1, y1), (x2, y2)] + edges + [_pairs(x_special, y_special)])


def _exp_inputs():
    rng, h = np.random.default_rng(SEEDS["exp"]), N_RANDOM // 2
    t = _uniform(rng, 0, 12, h)
    a = np.concatenate([_uniform(rng, -110, 90, h), -(t * t),    # the blur's argument
                        _around([88.72284, -87.33655, -103.97208], 2), SPECIALS, [DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX]]).astype(f32)
    return a, np.zeros_like(a)


def _plain_inputs():
    """One set for dot, length, normalize, xf_apply, roundf_te and span.  Kinds come in runs, because dot and xf_apply read
    the samples after their own (see math.hip)."""
    rng, q = np.random.default_rng(SEEDS["plain"]), N_RANDOM // 4
    h = q // 2
    with np.errstate(all="ignore"):
        spread = lambda n, lo, hi: (np.exp2(rng.uniform(lo, hi, n)) * _signs(rng, n)).astype(f32)   # noqa: E731
        ties = (np.arange(-2048, 2048, dtype=np.float64) + 0.5).astype(f32)                         # exact ties of rintf
        big_ties = _around(np.ldexp(f32(1), np.arange(20, 26)).astype(f32) + f32(0.5), 2)
        edge31 = _around([2147483648.0, -2147483648.0, 4294967296.0, -4294967296.0, 0.5, -0.5, 1.5, 2.5, -1.5, -2.5], 2)
        span_a, span_b = _pairs(np.concatenate([edge31, SPECIALS, [1.0, -3.75, FLT_MAX]]),
                                np.concatenate([edge31, SPECIALS, [1.0, -3.75, -FLT_MAX]]))
    return _cat([
        (_bits(rng, q), _bits(rng, q)),
        (_uniform(rng, -1e3, 1e3, q), _uniform(rng, -1e3, 1e3, q)),
        (spread(q, -80, 40), spread(q, -80, 40)),                            # products that underflow into the denormals
        (_bits(rng, h, 1, 0x00800000) * _signs(rng, h), _bits(rng, h, 1, 0x00800000) * _signs(rng, h)),   # denormal operands
        (spread(q - h, -149, -100), _uniform(rng, -4, 4, q - h)),
        (ties, ties[::-1]), (big_ties, -big_ties), (_uniform(rng, -3e3, 3e3, 4096), _uniform(rng, -3e3, 3e3, 4096)),
        (span_a, span_b)])


_INPUT_SETS = {"sin": "sincos", "cos": "sincos", "atan2": "atan2", "asin": "asin_acos", "acos": "asin_acos", "pow": "pow", "exp": "exp"}
_BUILDERS = {"sincos": _sincos_inputs, "atan2": _atan2_inputs, "asin_acos": _asin_acos_inputs, "pow": _pow_inputs, "exp": _exp_inputs,
             "plain": _plain_inputs}
_cache = {}


def inputs(fn_name):
    """(a, b): the f32 argument arrays of one function; identical on every machine (seeded), never modified"""
    key = _INPUT_SETS.get(fn_name, "plain")
    if key not in _cache:
        a, b = _BUILDERS[key]()
        a.setflags(write=False)
        b.setflags(write=False)
        _cache[key] = (a, b)
    return _cache[key]


def f64_inputs(fn_name):
    """the sincos / pow sets restricted to the documented domains of f64::sincos_medium and f64::pow_pos"""
    if fn_name == "pow_pos":
        a, b = inputs("pow")
        keep = (a > 0) & np.isfinite(a) & (np.abs(b) <= 8)
    else:
        a, b = inputs("sin")
        keep = np.abs(a) <= 512
    return np.ascontiguousarray(a[keep]), np.ascontiguousarray(b[keep])


# ---------------- the libraries ----------------
def _bind(lib, name, out_ptr_count):
    fn = getattr(lib, name)
    fn.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * out_ptr_count
    fn.restype = ctypes.c_int
    return fn


def build_reference(directory):
    """tests/math_ref.c with the oracle's flags -> math_ref(fn, a, b, n, out_bits, hard)"""
    so = os.path.join(str(directory), "libmath_ref.so")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                    "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "math_ref.c"), "-o", so, "-lm"], check=True)
    lib = ctypes.CDLL(so)
    return _bind(lib, "math_ref", 2), _bind(lib, "f64_error_ulps", 2)


def build_host_twin(directory):
    """g++ build of tests/device_checks/math.hip through the emulator's hip_runtime.h shim (the recipe of test_fp64_math.py)"""
    so = os.path.join(str(directory), "libmath_twin.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DVELLO_SIMT_EMU", "-ffp-contract=off", "-fno-fast-math", "-mfma",
                    "-I", os.path.join(ROOT, "tests", "simt_emu"), "-x", "c++",
                    os.path.join(ROOT, "tests", "device_checks", "math.hip"), "-o", so, "-lm"], check=True)
    return MathLib(ctypes.CDLL(so))


DEVCHECK_PATH = os.path.join(ROOT, "tests", "device_checks", "libvello_devcheck.so")


def load_device_library():
    """the gfx950 build; a library from before math.hip existed is an error, not a skip"""
    hint = "run `__graft_entry__.build()`"
    assert os.path.exists(DEVCHECK_PATH), f"tests/device_checks/libvello_devcheck.so missing: {hint}"
    lib = ctypes.CDLL(DEVCHECK_PATH)
    for name in ("vello_devcheck_math", "vello_devcheck_f64"):
        assert hasattr(lib, name), f"tests/device_checks/libvello_devcheck.so has no {name} (built before math.hip): {hint}"
    return MathLib(lib)


class MathLib:
    """vello_devcheck_math / vello_devcheck_f64 of either build of math.hip"""

    def __init__(self, lib):
        self._math, self._f64 = _bind(lib, "vello_devcheck_math", 1), _bind(lib, "vello_devcheck_f64", 1)

    def f32_bits(self, fn_name, a, b):
        out = np.zeros(len(a), dtype=np.uint32)
        rc = self._math(F32_FUNCTIONS.index(fn_name), a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data)
        assert rc == 0, f"vello_devcheck_math({fn_name}) failed: {rc}"
        return out

    def f64_bits(self, fn_name, a, b):
        out = np.zeros(len(a), dtype=np.uint64)
        rc = self._f64(F64_FUNCTIONS.index(fn_name), a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data)
        assert rc == 0, f"vello_devcheck_f64({fn_name}) failed: {rc}"
        return out


class Reference:
    """per function: the oracle's bits and the hard flags over inputs(fn); computed once, read-only"""

    def __init__(self, directory):
        (self._ref, self._ulps), self._done = build_reference(directory), {}

    def __call__(self, fn_name):
        if fn_name not in self._done:
            a, b = inputs(fn_name)
            bits, hard = np.zeros(len(a), dtype=np.uint32), np.zeros(len(a), dtype=np.uint8)
            rc = self._ref(F32_FUNCTIONS.index(fn_name), a.ctypes.data, b.ctypes.data, len(a), bits.ctypes.data, hard.ctypes.data)
            assert rc == 0
            hard = hard.astype(bool)
            bits.setflags(write=False)
            hard.setflags(write=False)
            self._done[fn_name] = (bits, hard)
        return self._done[fn_name]


    def f64_error_ulps(self, fn_name, a, b, bits64):
        """error of fp64 results of f64::sincos_medium / f64::pow_pos in fp64 ulps, against the long double value"""
        err = np.zeros(len(a), dtype=np.float64)
        bits64 = np.ascontiguousarray(bits64, dtype=np.uint64)
        rc = self._ulps(F64_FUNCTIONS.index(fn_name), a.ctypes.data, b.ctypes.data, len(a), bits64.ctypes.data, err.ctypes.data)
        assert rc == 0
        return err


# ---------------- comparison ----------------
def canonical_nan(bits):
    """as tests/parity.canonical_nan_words: every f32 NaN pattern becomes one quiet NaN; everything else, signed zeros
    included, stays as it is"""
    w = np.array(bits, dtype=np.uint32)
    w[((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)] = 0x7FC00000
    return w


def canonical_nan64(bits):
    w = np.array(bits, dtype=np.uint64)
    w[((w & 0x7FF0000000000000) == 0x7FF0000000000000) & ((w & 0x000FFFFFFFFFFFFF) != 0)] = 0x7FF8000000000000
    return w


def _ordered(bits):
    """f32 bit patterns as integers in value order (-0 and +0 adjacent), so that a difference counts ulps"""
    w = bits.astype(np.int64)
    return np.where(w & 0x80000000, -(w & 0x7FFFFFFF) - 1, w)


def mismatches(got_bits, want_bits, hard):
    """(indices that differ and are not flagged hard, flagged indices that differ by more than one f32 ulp)"""
    got, want = canonical_nan(got_bits), canonical_nan(want_bits)
    differ = got != want
    far = np.abs(_ordered(got) - _ordered(want)) > 1
    is_nan = lambda w: ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)   # noqa: E731
    far |= differ & (is_nan(got) | is_nan(want))
    return np.flatnonzero(differ & ~hard), np.flatnonzero(differ & hard & far)


def describe(fn_name, idx, got_bits, want_bits, limit=6):
    a, b = inputs(fn_name)
    rows = [f"  a={a[i]!r} ({a[i:i + 1].view(np.uint32)[0]:#010x}) b={b[i]!r} ({b[i:i + 1].view(np.uint32)[0]:#010x}): "
            f"got {int(got_bits[i]):#010x}, oracle {int(want_bits[i]):#010x}" for i in idx[:limit]]
    return f"{fn_name}: {len(idx)} of {len(a)} samples differ\n" + "\n".join(rows)
