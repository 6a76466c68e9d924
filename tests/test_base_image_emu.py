"""Base images (vello_hip_set_base_image) on the SIMT-emulated build of the kernel sources: k_fine_base's two load forms in
start_list and blend_pass, in place and under a damage rectangle, every entry point, the refusals and the public layers -- all
against the palette expectation built from the CPU oracle's whole frames (tests/base_image_parity.py)."""
import pytest

from tests import base_image_parity as bp
from tests import placement_parity as plp

MEM = plp.HostMemory()


def _emu_engine_factory():
    import vello_amd

    return lambda caps: vello_amd.Engine(capacities=caps)


@pytest.mark.parametrize("config", sorted(bp.CONFIGS))
def test_emu_base_image_matrix(emu_engine, config):
    bp.check_matrix(emu_engine, MEM, "emu_base", config)


@pytest.mark.parametrize("aa", [0, 1, 2])
def test_emu_base_image_brushes(emu_engine, aa):
    bp.check_brushes(emu_engine, MEM, "emu_base_brushes", aa)


@pytest.mark.parametrize("aa", [1, 2])
def test_emu_base_image_slices(emu_engine, aa):
    bp.check_slices(emu_engine, MEM, "emu_base_slices", aa)


def test_emu_base_image_blend_spill(emu_engine):
    bp.check_blend_spill(emu_engine, MEM, "emu_base_blend")


@pytest.mark.parametrize("aa", [0, 1, 2])
def test_emu_base_image_in_place(emu_engine, aa):
    bp.check_in_place(emu_engine, MEM, "emu_base_in_place", aa)


@pytest.mark.parametrize("aa", [0, 2])
def test_emu_base_image_damage_separate(emu_engine, aa):
    bp.check_damage_separate(emu_engine, MEM, "emu_base_damage", aa)


def test_emu_base_image_uniform_is_base_color(emu_engine):
    bp.check_uniform(emu_engine, MEM, "emu_base_uniform")


def test_emu_base_image_no_instances(emu_engine):
    bp.check_no_instances(emu_engine, MEM, "emu_base_n0")


@pytest.mark.parametrize("aa", [0, 2])
def test_emu_base_image_in_flight(emu_engine, aa):
    bp.check_in_flight(bp.dp.in_flight_engine(_emu_engine_factory()), MEM, "emu_base_in_flight", aa)


def test_emu_base_image_render_frame(emu_engine):
    bp.check_render_frame(emu_engine, MEM, "emu_base_render_frame")


def test_emu_base_image_out_none(emu_engine):
    bp.check_out_none(emu_engine, MEM, "emu_base_out_none")


def test_emu_base_image_host_target(emu_engine):
    bp.check_host_target(emu_engine, MEM, "emu_base_host_target")


def test_emu_base_image_morphed(emu_engine):
    bp.check_morphed(emu_engine, MEM, "emu_base_morphed")


def test_emu_base_image_retained_painted(emu_engine):
    bp.check_retained_painted(emu_engine, MEM, "emu_base_retained")


def test_emu_base_image_with_view(emu_engine):
    bp.check_with_view(emu_engine, MEM, "emu_base_view")


def test_emu_base_image_with_stroke_scale(emu_engine):
    bp.check_with_stroke_scale(emu_engine, MEM, "emu_base_stroke")


def test_emu_base_image_run_stages(emu_engine):
    bp.check_run_stages(emu_engine, MEM, "emu_base_run_stages")


def test_emu_base_image_failed_frame(emu_engine):
    bp.check_failed_frame(_emu_engine_factory(), MEM, "emu_base_failed")


def test_emu_base_image_refusals(emu_engine):
    bp.check_refusals(emu_engine, MEM, "emu_base_refusals")


def test_emu_base_image_engine_binding(emu_engine):
    bp.check_engine_binding(emu_engine, MEM, "emu_base_binding")


def test_emu_base_image_renderer(emu_engine):
    bp.check_renderer(MEM, "emu_base_renderer")
