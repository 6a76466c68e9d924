"""Marquee selection (vello_hip_pick_rect) on the SIMT-emulated build of the kernel sources: k_region_lines, the two kernels of the
draw pass and k_region_instances against the numpy reference of tests/region_parity.py, exactly, and against the oracle's image.
Device memory is host memory here: a numpy array passed with out_is_device stands for a device output."""
import numpy as np

from tests import region_parity as rg
from tests.test_pick_emu import _Dev as _PickDev


class _Dev(_PickDev):
    @staticmethod
    def words(n, fill=0):
        return np.full(n, fill, dtype=np.uint32)

    @staticmethod
    def words_numpy(r):
        return r


def _make_engine(caps):
    import vello_amd

    return vello_amd.Engine(capacities=caps)


def test_emu_pick_rect_reference_agrees_with_the_image(built):
    """The numpy reference alone satisfies the image check (no engine involved)."""
    rg.check_image(None, "ref_rect_image", answer=lambda o, rect: rg.reference(o, rect)[0])


def test_emu_pick_rect_square(emu_engine):
    rg.check_hand_square(emu_engine, "emu_rect_square")


def test_emu_pick_rect_hand_shapes(emu_engine):
    rg.check_hand_shapes(emu_engine, "emu_rect_shapes")


def test_emu_pick_rect_brush_fragments(emu_engine):
    rg.check_brush_fragments(emu_engine, "emu_rect_brushes")


def test_emu_pick_rect_clip_scene(emu_engine):
    rg.check_clip_scene(emu_engine, "emu_rect_clips")


def test_emu_pick_rect_clip_fragments(emu_engine):
    rg.check_clip_fragments(emu_engine, "emu_rect_clip_fragments")


def test_emu_pick_rect_image(emu_engine):
    rg.check_image(emu_engine, "emu_rect_image")


def test_emu_pick_rect_soup_shapes(emu_engine):
    rg.check_soup_shapes(emu_engine, "emu_rect_soup")


def test_emu_pick_rect_draw_shapes(emu_engine):
    rg.check_draw_shapes(emu_engine, "emu_rect_draws")


def test_emu_pick_rect_three_draws(emu_engine):
    rg.check_three_draws(emu_engine, "emu_rect_three")


def test_emu_pick_rect_instances(emu_engine):
    rg.check_instances(emu_engine, "emu_rect_instances", _Dev)


def test_emu_pick_rect_retained_painted(emu_engine):
    rg.check_retained_painted(emu_engine, "emu_rect_painted", _Dev)


def test_emu_pick_rect_culling(emu_engine):
    rg.check_culling(emu_engine, "emu_rect_cull")


def test_emu_pick_rect_which_frame(emu_engine):
    rg.check_which_frame(emu_engine, "emu_rect_which", _Dev)


def test_emu_pick_rect_sinks(emu_engine):
    rg.check_sinks(emu_engine, "emu_rect_sinks", _Dev)


def test_emu_pick_rect_refusals(emu_engine):
    rg.check_refusals(_make_engine, "emu_rect_refusals", _Dev)


def test_emu_pick_rect_failed_frame(emu_engine):
    rg.check_failed_frame(_make_engine, "emu_rect_failed", _Dev)


def test_emu_pick_rect_constants_and_flags(emu_engine):
    import vello_amd

    c = emu_engine.pick_constants()
    assert c["rect_lines_per_workgroup"] >= 64 and c["rect_draws_per_workgroup"] >= 64
    assert (vello_amd.REGION_TOUCHED, vello_amd.REGION_ENCLOSED) == (1, 2)
