"""Hit testing (vello_hip_pick) on the SIMT-emulated build of the kernel sources: k_pick_lines and k_pick_resolve against the numpy
reference of tests/pick_parity.py, exactly, and against the oracle's image.  Device memory is host memory here: a numpy array passed
with points_is_device stands for device points, and a device result is reached through the C entry point."""
import numpy as np

from tests import pick_parity as pk


class _Dev:
    @staticmethod
    def to_device(a):
        return np.ascontiguousarray(a, dtype=np.float32)

    @staticmethod
    def target(w, h):
        return np.zeros((h, w, 4), dtype=np.uint8)

    @staticmethod
    def to_numpy(t):
        return t

    @staticmethod
    def result(n, fill=0):
        return np.full((n, 2), fill, dtype=np.uint32)

    @staticmethod
    def result_numpy(r):
        return r


def _make_engine(caps):
    import vello_amd

    return vello_amd.Engine(capacities=caps)


def test_emu_pick_reference_agrees_with_the_image(built):
    """The numpy reference alone satisfies the image check (no engine involved)."""
    pk.check_image(None, "ref_image", pick=pk.reference)


def test_emu_pick_square(emu_engine):
    pk.check_hand_square(emu_engine, "emu_pick_square")


def test_emu_pick_hand_shapes(emu_engine):
    pk.check_hand_shapes(emu_engine, "emu_pick_shapes")


def test_emu_pick_brush_fragments(emu_engine):
    pk.check_brush_fragments(emu_engine, "emu_pick_brushes")


def test_emu_pick_clip_fragments(emu_engine):
    pk.check_clip_fragments(emu_engine, "emu_pick_clip_fragments")


def test_emu_pick_clip_scene(emu_engine):
    pk.check_clip_scene(emu_engine, "emu_pick_clips")


def test_emu_pick_image(emu_engine):
    pk.check_image(emu_engine, "emu_pick_image")


def test_emu_pick_soup_shapes(emu_engine):
    pk.check_soup_shapes(emu_engine, "emu_pick_soup")


def test_emu_pick_draw_shapes(emu_engine):
    pk.check_draw_shapes(emu_engine, "emu_pick_draws")


def test_emu_pick_query_counts(emu_engine):
    pk.check_query_counts(emu_engine, "emu_pick_counts")


def test_emu_pick_instances(emu_engine):
    pk.check_instances(emu_engine, "emu_pick_instances", _Dev)


def test_emu_pick_which_frame(emu_engine):
    pk.check_which_frame(emu_engine, "emu_pick_which", _Dev)


def test_emu_pick_sources(emu_engine):
    pk.check_sources(emu_engine, "emu_pick_sources", _Dev)


def test_emu_pick_refusals(emu_engine):
    pk.check_refusals(_make_engine, "emu_pick_refusals", _Dev)


def test_emu_pick_failed_frame(emu_engine):
    pk.check_failed_frame(_make_engine, "emu_pick_failed", _Dev)
