"""Per-instance paints (vello_hip_render_instances_painted) on the SIMT-emulated build of the kernel sources: the checks of
tests/paint_parity.py -- k_compose_scene's painted form against a numpy composition, the painted frame against the CPU oracle.  The
cut of the symbol map is the GPU suite's."""
import numpy as np
import pytest

from tests import paint_parity as pp


def _target(w, h):
    return np.zeros((h, w, 4), dtype=np.uint8)  # (stands for device memory in the emulated build)


def test_emu_paints_mask_bits(emu_engine):
    pp.check_mask_bits(emu_engine, "emu_paint_mask")


def test_emu_paints_chunk_boundaries(emu_engine):
    pp.check_chunk_boundaries(emu_engine, "emu_paint_chunks")


@pytest.mark.parametrize("steps", [2, pytest.param(8, marks=pytest.mark.slow)])
def test_emu_paints_long_chunks(emu_engine, steps):
    pp.check_long_chunks(emu_engine, "emu_paint_long", steps)


def test_emu_paints_unstaged(emu_engine):
    pp.check_unstaged(emu_engine, "emu_paint_unstaged")


def test_emu_paints_no_colour_words(emu_engine):
    pp.check_no_colour_words(emu_engine, "emu_paint_words")


def test_emu_paints_colour_values(emu_engine):
    pp.check_colour_values(emu_engine, "emu_paint_values")


def test_emu_paints_occlusion(emu_engine):
    pp.check_occlusion(emu_engine, "emu_paint_occlusion")


def test_emu_paints_host_agreement(emu_engine):
    pp.check_host_agreement(emu_engine, "emu_paint_host")


def test_emu_paints_null_and_empty(emu_engine):
    pp.check_null_and_empty(emu_engine, "emu_paint_null")


def test_emu_paints_life_cycle(emu_engine):
    pp.check_life_cycle(emu_engine, "emu_paint_life", _target, lambda t: t)


def test_emu_paints_errors(emu_engine):
    pp.check_errors(emu_engine, "emu_paint_errors", _target, lambda t: t)


def test_paint_struct_matches_header_and_shim():
    pp.check_struct_mirrors()
