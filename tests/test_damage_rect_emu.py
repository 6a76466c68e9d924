"""Damage rectangles (vello_hip_set_damage_rect) on the SIMT-emulated build of the kernel sources: k_coarse's tile window at tile,
quadrant and bin edges in both of its forms, k_fine's store held to the rectangle, empty and refused rectangles, slices, the blend
spill, frames in flight, the other per-frame options beside it, the pools and the public layers -- all against the CPU oracle's
WHOLE frame (tests/damage_parity.py)."""
import pytest

from tests import damage_parity as dp
from tests import placement_parity as plp

MEM = plp.HostMemory()


def _emu_engine_factory():
    import vello_amd

    return lambda caps: vello_amd.Engine(capacities=caps)


@pytest.mark.parametrize("rect", sorted(dp.RECTS))
@pytest.mark.parametrize("config", sorted(dp.CONFIGS))
def test_emu_damage_matrix(emu_engine, config, rect):
    dp.check_matrix(emu_engine, MEM, "emu_damage", config, rect)


def test_emu_damage_larger_than_target(emu_engine):
    dp.check_larger_than_target(emu_engine, MEM, "emu_damage_larger")


@pytest.mark.parametrize("part", range(dp.STORE_PARTS))
def test_emu_damage_fine_store(emu_engine, part):
    dp.check_store(emu_engine, MEM, "emu_damage_store", part)


@pytest.mark.parametrize("part", range(2))
def test_emu_damage_empty(emu_engine, part):
    dp.check_empty(emu_engine, MEM, "emu_damage_empty", dp.EMPTY_RECTS[part::2])


def test_emu_damage_pick_after(emu_engine):
    dp.check_pick_after_damage(emu_engine, MEM, "emu_damage_pick")


def test_emu_damage_refused(emu_engine):
    dp.check_refused(emu_engine, _emu_engine_factory()(None), "emu_damage_refused")


def test_emu_damage_slices(emu_engine):
    dp.check_slices(emu_engine, MEM, "emu_damage_slices")


def test_emu_damage_slice_demand(emu_engine):
    dp.check_slice_demand(emu_engine, "emu_damage_slice_demand")


def test_emu_damage_blend_spill(emu_engine):
    dp.check_blend_spill(emu_engine, MEM, "emu_damage_blend")


@pytest.mark.parametrize("toggle", [False, True])
def test_emu_damage_in_flight(emu_engine, toggle):
    dp.check_in_flight(dp.in_flight_engine(_emu_engine_factory()), MEM, "emu_damage_in_flight", toggle)


def test_emu_damage_with_viewport_cull(emu_engine):
    dp.check_with_viewport_cull(emu_engine, MEM, "emu_damage_cull")


def test_emu_damage_with_view(emu_engine):
    dp.check_with_view(emu_engine, "emu_damage_view")


def test_emu_damage_retained_painted(emu_engine):
    dp.check_retained_painted(emu_engine, "emu_damage_painted")


def test_emu_damage_morphed(emu_engine):
    dp.check_morphed(emu_engine, "emu_damage_morphed")


def test_emu_damage_render_frame(emu_engine):
    dp.check_render_frame(emu_engine, "emu_damage_render_frame")


def test_emu_damage_instances(emu_engine):
    dp.check_instances(emu_engine, "emu_damage_instances")


def test_emu_damage_indexed_scene(emu_engine):
    dp.check_indexed(emu_engine, "emu_damage_indexed")


def test_emu_damage_fused_front(emu_engine):
    dp.check_fused_front(emu_engine, MEM, "emu_damage_front")


def test_emu_damage_run_stages(emu_engine):
    dp.check_run_stages(emu_engine, "emu_damage_run_stages")


def test_emu_damage_segment_pool(emu_engine):
    dp.check_segment_pool(_emu_engine_factory(), MEM, "emu_damage_pool")


def test_emu_damage_renderer(emu_engine):
    dp.check_renderer("emu_damage_renderer")
