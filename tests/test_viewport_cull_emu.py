"""Viewport culling (vello_hip_set_viewport_cull) on the SIMT-emulated build of the kernel sources: each flush site of flatten and
each kernel set, the staging bypass, the boundaries of the rule, the fuzzer, the option's life cycle and the public layers, all
against the CPU oracle with its soup filtered by the rule (tests/cull_parity.py).  The large scenes are the GPU suite's."""
import pytest

from tests import cull_parity as cp
from tests.emu_lib import emu_library_path


def _emu_engine_factory():
    import vello_amd

    return lambda caps: vello_amd.Engine(capacities=caps)


def test_emu_cull_light_pass(emu_engine):
    cp.check_light_pass(emu_engine, "emu_cull_light")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_emu_cull_stroked_polylines(emu_engine, stroke_kernel):
    cp.check_stroked_polylines(emu_engine, f"emu_cull_polylines_{int(stroke_kernel)}", stroke_kernel)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
@pytest.mark.parametrize("case", range(4))
def test_emu_cull_curves(emu_engine, case, which):
    cp.check_curves(emu_engine, "emu_cull_curves", case, which, in_flight=case in (1, 3))


@pytest.mark.parametrize("case", range(2))
def test_emu_cull_random_view(emu_engine, case):
    cp.check_random_view(emu_engine, "emu_cull_random", case)


def test_emu_cull_small_scene_fusion(emu_engine):
    cp.check_small_scene_fusion(emu_engine, "emu_cull_front")


def test_emu_cull_tiger(emu_engine):
    cp.check_tiger(emu_engine, "emu_cull_tiger")


def test_emu_cull_staging_bypass(emu_engine):
    cp.check_staging_bypass(emu_engine, "emu_cull_bypass")


def test_emu_cull_boundaries(emu_engine):
    cp.check_boundaries(emu_engine, "emu_cull_edges")


def test_emu_cull_fuzz(emu_engine):
    cp.check_fuzz(emu_engine, "emu_cull_fuzz", range(0, 12), extreme=False)


def test_emu_cull_fuzz_extreme(emu_engine):
    cp.check_fuzz(emu_engine, "emu_cull_fuzzx", [s for s in range(0, 14) if s not in (2, 5)], extreme=True)


@pytest.mark.slow
def test_emu_cull_fuzz_more_seeds(emu_engine):
    cp.check_fuzz(emu_engine, "emu_cull_fuzz", range(12, 60), extreme=False)
    cp.check_fuzz(emu_engine, "emu_cull_fuzzx", [s for s in range(14, 40) if s != 25], extreme=True)


def test_emu_cull_toggle_resident(emu_engine):
    cp.check_toggle_resident(emu_engine, "emu_cull_toggle")


def test_emu_cull_line_pool(emu_engine):
    cp.check_line_pool(_emu_engine_factory(), "emu_cull_pool")


def test_emu_cull_renderer_option(emu_engine):
    cp.check_renderer_option("emu_cull_renderer")


def test_emu_cull_null_context(emu_engine):
    assert emu_engine._lib.vello_hip_set_viewport_cull(None, 1) == -1
