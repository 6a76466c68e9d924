"""Damage rectangles (vello_hip_set_damage_rect) on the MI355X: the cases of test_damage_rect_emu.py on the real kernels -- the
wave-uniform window in k_coarse's ballots and early exits, k_fine's 16-byte and dword stores into device memory -- and bench.py's d2
at 1600 x 1600, which only fits here."""
import pytest

from tests import damage_parity as dp
from tests import placement_parity as plp

pytestmark = pytest.mark.gpu
MEM = plp.TorchMemory()


def _gpu_engine_factory():
    import vello_amd

    return lambda caps: vello_amd.Engine(device=0, capacities=caps)


@pytest.mark.parametrize("rect", sorted(dp.RECTS))
@pytest.mark.parametrize("config", sorted(dp.CONFIGS))
def test_gpu_damage_matrix(gpu_engine, config, rect):
    dp.check_matrix(gpu_engine, MEM, "gpu_damage", config, rect)


def test_gpu_damage_larger_than_target(gpu_engine):
    dp.check_larger_than_target(gpu_engine, MEM, "gpu_damage_larger")


@pytest.mark.parametrize("part", range(dp.STORE_PARTS))
def test_gpu_damage_fine_store(gpu_engine, part):
    dp.check_store(gpu_engine, MEM, "gpu_damage_store", part)


@pytest.mark.parametrize("part", range(2))
def test_gpu_damage_empty(gpu_engine, part):
    dp.check_empty(gpu_engine, MEM, "gpu_damage_empty", dp.EMPTY_RECTS[part::2])


def test_gpu_damage_pick_after(gpu_engine):
    dp.check_pick_after_damage(gpu_engine, MEM, "gpu_damage_pick")


def test_gpu_damage_refused(gpu_engine):
    dp.check_refused(gpu_engine, _gpu_engine_factory()(None), "gpu_damage_refused")


def test_gpu_damage_slices(gpu_engine):
    dp.check_slices(gpu_engine, MEM, "gpu_damage_slices")


def test_gpu_damage_slice_demand(gpu_engine):
    dp.check_slice_demand(gpu_engine, "gpu_damage_slice_demand")


def test_gpu_damage_blend_spill(gpu_engine):
    dp.check_blend_spill(gpu_engine, MEM, "gpu_damage_blend")


@pytest.mark.parametrize("toggle", [False, True])
def test_gpu_damage_in_flight(gpu_engine, toggle):
    dp.check_in_flight(dp.in_flight_engine(_gpu_engine_factory()), MEM, "gpu_damage_in_flight", toggle)


def test_gpu_damage_with_viewport_cull(gpu_engine):
    dp.check_with_viewport_cull(gpu_engine, MEM, "gpu_damage_cull")


def test_gpu_damage_with_view(gpu_engine):
    dp.check_with_view(gpu_engine, "gpu_damage_view")


def test_gpu_damage_retained_painted(gpu_engine):
    dp.check_retained_painted(gpu_engine, "gpu_damage_painted")


def test_gpu_damage_morphed(gpu_engine):
    dp.check_morphed(gpu_engine, "gpu_damage_morphed")


def test_gpu_damage_render_frame(gpu_engine):
    dp.check_render_frame(gpu_engine, "gpu_damage_render_frame")


def test_gpu_damage_instances(gpu_engine):
    dp.check_instances(gpu_engine, "gpu_damage_instances")


def test_gpu_damage_indexed_scene(gpu_engine):
    dp.check_indexed(gpu_engine, "gpu_damage_indexed")


def test_gpu_damage_fused_front(gpu_engine):
    dp.check_fused_front(gpu_engine, MEM, "gpu_damage_front")


def test_gpu_damage_run_stages(gpu_engine):
    dp.check_run_stages(gpu_engine, "gpu_damage_run_stages")


def test_gpu_damage_segment_pool(gpu_engine):
    dp.check_segment_pool(_gpu_engine_factory(), MEM, "gpu_damage_pool")


def test_gpu_damage_renderer(gpu_engine):
    dp.check_renderer("gpu_damage_renderer")


def test_gpu_damage_d2(gpu_engine):
    # bench.py's headline scene at 1600 x 1600, MSAA16, pools of D2_CAPS: a 256 x 256 window in the middle, and one tile
    import bench
    import vello_amd
    import workloads
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    packed, layout = workloads.paris_like_scene_d2().resolve()
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    ref = dp.Reference(packed, layout, 1600, 1600, dp.WHITE, AaConfig.Msaa16, oracle=Oracle(capacity_scale=8))
    for rect in ((700, 700, 956, 956), (800, 800, 816, 816)):
        dp.compare_damaged_frame(eng, ref, rect, f"gpu_damage_d2_{rect}", mem=MEM, no_cull=True, front=False)
