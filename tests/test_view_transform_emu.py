"""The view transform (vello_hip_set_view_transform) on the SIMT-emulated build of the kernel sources: views, scenes, stream shapes,
life cycle, errors, culling, the estimator and the public layers against the CPU oracle on the composed scene (tests/view_parity.py).
The large scenes are the GPU suite's."""
import numpy as np
import pytest

from tests import view_parity as vp


def _target(w, h):
    return np.zeros((h, w, 4), dtype=np.uint8)  # (stands for device memory in the emulated build)


def _engine_factory():
    import vello_amd

    return lambda caps: vello_amd.Engine(capacities=caps)


def test_emu_view_identity_equals_off(emu_engine):
    vp.check_identity(emu_engine, "emu_view_identity")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_emu_view_polygons_polylines(emu_engine, stroke_kernel):
    vp.check_polygons_polylines(emu_engine, f"emu_view_lines_{int(stroke_kernel)}", stroke_kernel)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
@pytest.mark.parametrize("case", range(3))
def test_emu_view_curves(emu_engine, case, which):
    vp.check_curves(emu_engine, "emu_view_curves", which, case)


@pytest.mark.parametrize("ref", [False, True])
def test_emu_view_stroke_styles(emu_engine, ref):
    vp.check_stroke_styles(emu_engine, f"emu_view_stroke_styles_{int(ref)}", ref)


@pytest.mark.parametrize("scene", vp.BRUSH_SCENES)
def test_emu_view_brushes(emu_engine, scene):
    vp.check_brushes(emu_engine, "emu_view", scene)


@pytest.mark.parametrize("scene", ["clip_blend_scene", "many_clips_scene"])
def test_emu_view_clips(emu_engine, scene):
    vp.check_clips(emu_engine, "emu_view", scene)


def test_emu_view_tiger(emu_engine):
    vp.check_tiger(emu_engine, "emu_view_tiger")


def test_emu_view_front_fusion(emu_engine):
    vp.check_front_fusion(emu_engine, "emu_view_front")


def test_emu_view_fuzz(emu_engine):
    vp.check_fuzz(emu_engine, "emu_view_fuzz", range(0, 10), extreme=False)


def test_emu_view_fuzz_extreme(emu_engine):
    vp.check_fuzz(emu_engine, "emu_view_fuzzx", [s for s in range(0, 10) if s not in (2, 5)], extreme=True)


def test_emu_view_stream_shapes(emu_engine):
    vp.check_stream_shapes(emu_engine, "emu_view_shapes")


def test_emu_view_trans_ix_minus_one(emu_engine):
    vp.check_trans_ix_minus_one(emu_engine, "emu_view_zero_width_clip_first")


def test_emu_view_four_frames_in_flight(emu_engine):
    vp.check_in_flight(emu_engine, "emu_view_in_flight", _target, lambda t: t)


def test_emu_view_render_frame_and_run_stages(emu_engine):
    vp.check_render_frame_and_stages(emu_engine, "emu_view_stages", _target, lambda t: t)


def test_emu_view_render_frame_does_not_reallocate(emu_engine):
    vp.check_no_reallocation(emu_engine, "emu_view_no_realloc", _target, lambda t: t)


def test_emu_view_errors(emu_engine):
    vp.check_errors(emu_engine, "emu_view_errors")


def test_emu_view_with_culling(emu_engine):
    vp.check_culled(emu_engine, "emu_view_cull")


def test_emu_view_estimator_and_auto_grow(emu_engine):
    vp.check_estimator(_engine_factory(), "emu_view_estimate")


def test_emu_view_renderer_params(emu_engine):
    vp.check_renderer("emu_view_renderer")
