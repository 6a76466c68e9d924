"""The view transform (vello_hip_set_view_transform) on the MI355X: the cases of test_view_transform_emu.py on the real kernels, and the
large scenes that only fit here -- the road map under a pan sequence, with and without viewport culling, and the mmark window of the
cull suite expressed as a view of the whole scene instead of a re-encoded one."""
import numpy as np
import pytest

from tests import view_parity as vp

pytestmark = pytest.mark.gpu


def _target(w, h):
    import torch

    return torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")


def _numpy(t):
    return t.cpu().numpy()


def test_gpu_view_identity_equals_off(gpu_engine):
    vp.check_identity(gpu_engine, "gpu_view_identity")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_gpu_view_polygons_polylines(gpu_engine, stroke_kernel):
    vp.check_polygons_polylines(gpu_engine, f"gpu_view_lines_{int(stroke_kernel)}", stroke_kernel)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
@pytest.mark.parametrize("case", range(3))
def test_gpu_view_curves(gpu_engine, case, which):
    vp.check_curves(gpu_engine, "gpu_view_curves", which, case)


@pytest.mark.parametrize("ref", [False, True])
def test_gpu_view_stroke_styles(gpu_engine, ref):
    vp.check_stroke_styles(gpu_engine, f"gpu_view_stroke_styles_{int(ref)}", ref)


@pytest.mark.parametrize("scene", vp.BRUSH_SCENES)
def test_gpu_view_brushes(gpu_engine, scene):
    vp.check_brushes(gpu_engine, "gpu_view", scene)


@pytest.mark.parametrize("scene", ["clip_blend_scene", "many_clips_scene"])
def test_gpu_view_clips(gpu_engine, scene):
    vp.check_clips(gpu_engine, "gpu_view", scene)


def test_gpu_view_tiger(gpu_engine):
    vp.check_tiger(gpu_engine, "gpu_view_tiger")


def test_gpu_view_front_fusion(gpu_engine):
    vp.check_front_fusion(gpu_engine, "gpu_view_front")


def test_gpu_view_fuzz(gpu_engine):
    vp.check_fuzz(gpu_engine, "gpu_view_fuzz", range(0, 40), extreme=False)


def test_gpu_view_fuzz_extreme(gpu_engine):
    vp.check_fuzz(gpu_engine, "gpu_view_fuzzx", [s for s in range(0, 30) if s not in (2, 5, 25)], extreme=True)


def test_gpu_view_stream_shapes(gpu_engine):
    vp.check_stream_shapes(gpu_engine, "gpu_view_shapes")


def test_gpu_view_trans_ix_minus_one(gpu_engine):
    vp.check_trans_ix_minus_one(gpu_engine, "gpu_view_zero_width_clip_first")


def test_gpu_view_four_frames_in_flight(gpu_engine):
    vp.check_in_flight(gpu_engine, "gpu_view_in_flight", _target, _numpy)


def test_gpu_view_render_frame_and_run_stages(gpu_engine):
    vp.check_render_frame_and_stages(gpu_engine, "gpu_view_stages", _target, _numpy)


def test_gpu_view_render_frame_does_not_reallocate(gpu_engine):
    vp.check_no_reallocation(gpu_engine, "gpu_view_no_realloc", _target, _numpy)


def test_gpu_view_errors(gpu_engine):
    vp.check_errors(gpu_engine, "gpu_view_errors")


def test_gpu_view_with_culling(gpu_engine):
    vp.check_culled(gpu_engine, "gpu_view_cull")


def test_gpu_view_estimator_and_auto_grow(gpu_engine):
    import vello_amd

    vp.check_estimator(lambda caps: vello_amd.Engine(device=0, capacities=caps), "gpu_view_estimate")


def test_gpu_view_renderer_params(gpu_engine):
    vp.check_renderer("gpu_view_renderer")


@pytest.mark.parametrize("cull", [False, True])
def test_gpu_view_d2_pan(gpu_engine, cull):
    # bench.py's headline scene, resident once, its top-left 800 x 800 under three views of a pan sequence (pools of D2_CAPS)
    import bench
    import vello_amd
    import workloads
    from oracle.oracle import Oracle
    from vello_amd import AaConfig, Affine

    packed, layout = workloads.paris_like_scene_d2().resolve()
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    for k, (dx, dy) in enumerate(((0.0, 0.0), (-137.5, -61.25), (-400.0, -333.0))):
        v = Affine.translate(dx, dy)
        kw = dict(exact_soup=False, require_culling=True) if cull else {}
        vp.compare_view_frame(eng, packed, layout, v, 800, 800, vp.WHITE, AaConfig.Msaa16, f"gpu_view_d2_pan{k}_cull{int(cull)}", culled=cull,
                              oracle=Oracle(capacity_scale=8), differs=k > 0, **kw)


def test_gpu_view_mmark_window(gpu_engine):
    # the 50 000-element mmark scene, a 1024 x 576 window into the middle of it at 1.5 x: the cull suite's case as a VIEW of the scene
    import workloads
    from oracle.oracle import Oracle
    from vello_amd import AaConfig, Affine

    packed, layout = workloads.mmark_scene().resolve()
    v = Affine.translate(-600.0, -500.0) * Affine.scale(1.5)
    gpu_engine.set_auto_grow(True)
    try:
        vp.compare_view_frame(gpu_engine, packed, layout, v, 1024, 576, vp.WHITE, AaConfig.Msaa16, "gpu_view_mmark_window", culled=True,
                              oracle=Oracle(capacity_scale=8), exact_soup=False, require_culling=True)
    finally:
        gpu_engine.set_auto_grow(False)
