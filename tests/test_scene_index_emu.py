"""The scene index (vello_hip_scene_index_builds) on the SIMT-emulated build of the kernel sources: indexed frames against their
VELLO_HIP_DEBUG_NO_SCENE_INDEX twins and the CPU oracle, one index under many views, invalidation, first frames after an upload and
an overrunning tag stream (tests/scene_index_parity.py).  A frame of these scenes takes two seconds here, so the twins run the whole
product of kernel sets and frames in flight on the mixed scene only and every other scene once with each kernel set and each number of
frames in flight; the GPU suite runs the product on all of them."""
import numpy as np
import pytest

from tests import scene_index_parity as sp


def _target(w, h):
    return np.zeros((h, w, 4), dtype=np.uint8)  # (stands for device memory in the emulated build)


TWINS = [("mixed", k, n) for k in ("flatten_coop", "flatten_alone") for n in (1, 3)]
TWINS += [(w, k, n) for w in sp.CASES[1:] for k, n in (("flatten_coop", 1), ("flatten_alone", 3))]
TWINS += [("fills_only", "flatten_coop", 3), ("strokes_only", "flatten_alone", 1)]  # (the empty lists under the other launch shape too)


@pytest.mark.parametrize("which,kernels,in_flight", TWINS)
def test_emu_scene_index_twin(emu_engine, which, kernels, in_flight):
    sp.check_twin(emu_engine, which, kernels, in_flight, f"emu_index_{which}_{kernels}_{in_flight}", _target, lambda t: t, back_half=False)


def test_emu_scene_index_many_frames(emu_engine):
    sp.check_many_frames(emu_engine, "emu_index_many")


def test_emu_scene_index_invalidation(emu_engine):
    import vello_amd

    sp.check_invalidation(emu_engine, vello_amd.Engine(), "emu_index_invalidation", _target, lambda t: t)


def test_emu_scene_index_first_frames(emu_engine):
    sp.check_first_frames(emu_engine, "emu_index_first", _target, lambda t: t)


def test_emu_scene_index_overrun(emu_engine):
    sp.check_overrun(emu_engine, "emu_index_overrun")


def test_emu_scene_index_small_scenes_have_none(emu_engine):
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.stroke_styles_scene().resolve()
    before = emu_engine.scene_index_builds()
    emu_engine.render(packed, layout, 128, 128, sp.WHITE, AaConfig.Msaa8)
    assert emu_engine.scene_index_builds() == before
    assert emu_engine._lib.vello_hip_scene_index_builds(None) == 0
