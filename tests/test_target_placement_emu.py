"""Target strides, offsets and non-square atlases on the SIMT-emulated build of the kernel sources (tests/placement_parity.py): numpy
arrays stand for device memory here."""
import numpy as np
import pytest

from tests import placement_parity as pp

MEM = pp.HostMemory()


def test_emu_placement_matrix_reaches_every_store_path():
    pp.check_matrix_inputs()


@pytest.mark.parametrize("ti", range(len(pp.TARGETS)), ids=[f"{w}x{h}" for w, h in pp.TARGETS])
def test_emu_placement_matrix(emu_engine, ti):
    pp.check_matrix_target(emu_engine, MEM, "emu_place", ti)


def test_emu_placement_render_host_odd_stride(emu_engine):
    pp.check_render_host(emu_engine, "emu_place_render_host")


def test_emu_placement_render_device(emu_engine):
    pp.check_render_device(emu_engine, MEM, "emu_place_render_device")


def test_emu_placement_render_frame(emu_engine):
    pp.check_render_frame(emu_engine, MEM, "emu_place_render_frame")


def test_emu_placement_render_instances(emu_engine):
    pp.check_render_instances(emu_engine, MEM, "emu_place_render_instances")


def test_emu_placement_renderer_host(emu_engine):
    pp.check_renderer(MEM, "emu_place_renderer_host", device=False)


@pytest.mark.parametrize("aa", [0, 1, 2])
def test_emu_placement_brushes(emu_engine, aa):
    from vello_amd import AaConfig

    pp.check_brushes(emu_engine, MEM, f"emu_place_brushes_aa{aa}", AaConfig(aa))


def test_emu_placement_fine_slices(emu_engine):
    pp.check_fine_slices(emu_engine, MEM, "emu_place_slices")


def test_emu_placement_contact_sheet_in_flight(emu_engine):
    pp.check_contact_sheet(emu_engine, MEM, "emu_place_sheet")


def test_emu_placement_refusals(emu_engine):
    pp.check_refusals(emu_engine, MEM, "emu_place_refused")


@pytest.mark.parametrize("which", range(len(pp.ATLASES)), ids=[f"{a[0]}x{a[1]}" for a in pp.ATLASES])
def test_emu_atlas_not_square_write_image(emu_engine, which):
    pp.check_atlas(emu_engine, "emu_atlas_write", which)


@pytest.mark.parametrize("which", range(len(pp.ATLASES)), ids=[f"{a[0]}x{a[1]}" for a in pp.ATLASES])
def test_emu_atlas_not_square_copy_images(emu_engine, which):
    pp.check_atlas(emu_engine, "emu_atlas_copy", which, device_source=lambda a: np.array(a, copy=True))
