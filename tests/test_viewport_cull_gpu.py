"""Viewport culling (vello_hip_set_viewport_cull) on the MI355X: the cases of test_viewport_cull_emu.py on the real kernels -- wave
ballots, the LDS exchange between the four waves, the fused reservations -- and the large scenes that only fit here."""
import json
import os

import pytest

from tests import cull_parity as cp
from tests import parity

pytestmark = pytest.mark.gpu
OUT = os.path.dirname(parity.DUMP_DIR)  # (beside the parity suite's dumps)


def _record(name, stats):
    """|R|, |S| and the soup's size of a large case, for profiles/viewport_cull.txt (best effort: the assertions are the test)."""
    print(f"{name}: {stats}, retained cullable lines {stats['soup'] - stats['S']}")
    try:
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, "viewport_cull_soup_sizes.jsonl"), "a") as f:
            f.write(json.dumps(dict(stats, case=name)) + "\n")
    except OSError:
        pass


def test_gpu_cull_light_pass(gpu_engine):
    cp.check_light_pass(gpu_engine, "gpu_cull_light")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_gpu_cull_stroked_polylines(gpu_engine, stroke_kernel):
    cp.check_stroked_polylines(gpu_engine, f"gpu_cull_polylines_{int(stroke_kernel)}", stroke_kernel)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
@pytest.mark.parametrize("case", range(4))
def test_gpu_cull_curves(gpu_engine, case, which):
    cp.check_curves(gpu_engine, "gpu_cull_curves", case, which)


@pytest.mark.parametrize("case", range(2))
def test_gpu_cull_random_view(gpu_engine, case):
    cp.check_random_view(gpu_engine, "gpu_cull_random", case)


def test_gpu_cull_small_scene_fusion(gpu_engine):
    cp.check_small_scene_fusion(gpu_engine, "gpu_cull_front")


def test_gpu_cull_tiger(gpu_engine):
    cp.check_tiger(gpu_engine, "gpu_cull_tiger")


def test_gpu_cull_staging_bypass(gpu_engine):
    _record("heavy_strokes_346x259", cp.check_staging_bypass(gpu_engine, "gpu_cull_bypass"))


def test_gpu_cull_boundaries(gpu_engine):
    cp.check_boundaries(gpu_engine, "gpu_cull_edges")


def test_gpu_cull_fuzz(gpu_engine):
    cp.check_fuzz(gpu_engine, "gpu_cull_fuzz", range(0, 60), extreme=False)


def test_gpu_cull_fuzz_extreme(gpu_engine):
    cp.check_fuzz(gpu_engine, "gpu_cull_fuzzx", [s for s in range(0, 40) if s not in (2, 5, 25)], extreme=True)


def test_gpu_cull_toggle_resident(gpu_engine):
    cp.check_toggle_resident(gpu_engine, "gpu_cull_toggle")


def test_gpu_cull_line_pool(gpu_engine):
    import vello_amd

    cp.check_line_pool(lambda caps: vello_amd.Engine(device=0, capacities=caps), "gpu_cull_pool")


def test_gpu_cull_renderer_option(gpu_engine):
    cp.check_renderer_option("gpu_cull_renderer")


@pytest.mark.parametrize("size", [1600, 800])
def test_gpu_cull_d2(gpu_engine, size):
    # bench.py's headline scene, whole (17 % of its lines are off the target) and its top-left 800 x 800 (78 %), pools of D2_CAPS
    import bench
    import vello_amd
    import workloads
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    packed, layout = workloads.paris_like_scene_d2().resolve()
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    stats = {}
    cp.compare_culled_frame(eng, packed, layout, size, size, cp.WHITE, AaConfig.Msaa16, f"gpu_cull_d2_{size}", oracle=Oracle(capacity_scale=8),
                            exact_soup=False, stats=stats)
    _record(f"d2_{size}", stats)


def test_gpu_cull_mmark_view(gpu_engine):
    # the 50 000-element mmark scene, a 1024 x 576 window into the middle of it at 1.5 x
    import workloads
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    packed, layout = cp.view_of(workloads.mmark_scene(), 600, 500, 1.5).resolve()
    gpu_engine.set_auto_grow(True)
    stats = {}
    try:
        cp.compare_culled_frame(gpu_engine, packed, layout, 1024, 576, cp.WHITE, AaConfig.Msaa16, "gpu_cull_mmark_view", oracle=Oracle(capacity_scale=8),
                                exact_soup=False, stats=stats)
    finally:
        gpu_engine.set_auto_grow(False)
    _record("mmark_view_1024x576", stats)
