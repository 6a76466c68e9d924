"""Device check of common.h's floating-point rules (tests/device_checks/math.hip in libvello_devcheck.so): the gfx950 build's
sin_cr ... exp_cr, dot, length, normalize, xf_apply, roundf_te and span against the oracle's own functions
(tests/math_ref.c), and the fp64 bits of f64::sincos_medium and f64::pow_pos against the g++ build of the same header.

The emulator suite cannot see any of this: there ocml's atan2 / asin / acos / exp / pow / sincos are glibc's, the functions the
oracle calls, and fp contraction, denormal flushing, the rounding of sqrtf, / and fp64 division are the host compiler's.  Only
samples flagged hard (exact value within 2^-50 of an f32 midpoint, tests/math_rules.py) may differ, and then by one ulp.

Figures (samples, hard-flagged, mismatches per function; wall time) are in profiles/device_math.txt."""
import time

import numpy as np
import pytest

from tests import math_rules as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(built):
    return M.load_device_library()


def test_gpu_f32_rules_equal_the_oracle(device, tmp_path):
    reference = M.Reference(tmp_path)
    failures = []
    for fn in M.F32_FUNCTIONS:
        a, b = M.inputs(fn)
        want, hard = reference(fn)
        t0 = time.perf_counter()
        got = device.f32_bits(fn, a, b)
        dt = time.perf_counter() - t0
        wrong, far = M.mismatches(got, want, hard)
        print(f"{fn}: samples {len(a)}, hard-flagged {int(hard.sum())}, device mismatches {len(wrong)}, "
              f"hard ones beyond 1 ulp {len(far)}, device call {dt * 1e3:.1f} ms")
        if len(wrong):
            failures.append(M.describe(fn, wrong, got, want))
        if len(far):
            failures.append("hard-flagged, but more than one ulp apart: " + M.describe(fn, far, got, want))
    assert not failures, "the gfx950 build differs from the oracle:\n" + "\n".join(failures)


def test_gpu_fp64_bits_equal_the_host_build(device, tmp_path):
    twin = M.build_host_twin(tmp_path)
    failures = []
    for fn in M.F64_FUNCTIONS:
        a, b = M.f64_inputs(fn)
        assert len(a) > M.N_RANDOM // 2
        got, want = M.canonical_nan64(device.f64_bits(fn, a, b)), M.canonical_nan64(twin.f64_bits(fn, a, b))
        bad = np.flatnonzero(got != want)
        print(f"{fn}: samples {len(a)}, device fp64 results differing from the host build {len(bad)}")
        if len(bad):
            rows = [f"  a={a[i]!r} b={b[i]!r}: device {int(got[i]):#018x}, host {int(want[i]):#018x}" for i in bad[:6]]
            failures.append(f"{fn}: {len(bad)} of {len(a)} fp64 results differ\n" + "\n".join(rows))
    assert not failures, "gfx950 and g++ builds of fp64_math.h disagree:\n" + "\n".join(failures)
