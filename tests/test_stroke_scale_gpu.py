"""The per-frame stroke scale (vello_hip_set_stroke_scale) on the MI355X: the cases of test_stroke_scale_emu.py on the real kernels --
k_style_widths in its 8-byte and its dword form at every partition size -- with the tiger at 512 x 512 and the retained list's poses
in a torch tensor on the GPU."""
import numpy as np
import pytest

from tests import morph_parity as mp
from tests import stroke_scale_parity as sp

pytestmark = pytest.mark.gpu


class _Memory(mp.GpuMemory):
    def target(self, w, h):
        import torch

        t = super().target(w, h)
        torch.cuda.synchronize()  # (the engine's streams do not wait for torch's)
        return t


MEM = _Memory()


def _poses(poses):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32)).to("cuda")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("n", sp.PARTITIONS)
def test_gpu_stroke_scale_partitions(gpu_engine, n, odd):
    sp.check_partition(gpu_engine, "gpu_stroke_scale_part", n, odd)


def test_gpu_stroke_scale_branches(gpu_engine):
    sp.check_branches(gpu_engine, "gpu_stroke_scale_branches")


def test_gpu_stroke_scale_off_state(gpu_engine):
    sp.check_off_state(gpu_engine, "gpu_stroke_scale_off")


def test_gpu_stroke_scale_front_fusion(gpu_engine):
    sp.check_front_fusion(gpu_engine, "gpu_stroke_scale_front")


def test_gpu_stroke_scale_tiny_fused(gpu_engine):
    sp.check_tiny_fused(gpu_engine, "gpu_stroke_scale_tiny")


def test_gpu_stroke_scale_indexed(gpu_engine):
    sp.check_indexed(gpu_engine, "gpu_stroke_scale_indexed")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_gpu_stroke_scale_stroked_lines(gpu_engine, stroke_kernel):
    sp.check_stroked_lines(gpu_engine, "gpu_stroke_scale_lines", stroke_kernel)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
def test_gpu_stroke_scale_curves(gpu_engine, which):
    sp.check_curves(gpu_engine, "gpu_stroke_scale_curves", which)


def test_gpu_stroke_scale_area(gpu_engine):
    sp.check_area(gpu_engine, "gpu_stroke_scale_area")


def test_gpu_stroke_scale_tiger(gpu_engine):
    sp.check_tiger(gpu_engine, "gpu_stroke_scale_tiger")


def test_gpu_stroke_scale_view(gpu_engine):
    sp.check_view(gpu_engine, "gpu_stroke_scale_view")


def test_gpu_stroke_scale_culled(gpu_engine):
    sp.check_culled(gpu_engine, "gpu_stroke_scale_culled")


def test_gpu_stroke_scale_damage(gpu_engine):
    sp.check_damage(gpu_engine, "gpu_stroke_scale_damage")


def test_gpu_stroke_scale_morph(gpu_engine):
    sp.check_morph(gpu_engine, "gpu_stroke_scale_morph")


def test_gpu_stroke_scale_render_frame(gpu_engine):
    sp.check_render_frame(gpu_engine, "gpu_stroke_scale_render_frame")


def test_gpu_stroke_scale_instances_painted(gpu_engine):
    sp.check_instances_painted(gpu_engine, "gpu_stroke_scale_instances")


def test_gpu_stroke_scale_retained_painted(gpu_engine):
    sp.check_retained_painted(gpu_engine, "gpu_stroke_scale_retained", device_poses=_poses)


def test_gpu_stroke_scale_in_flight(gpu_engine):
    sp.check_in_flight(gpu_engine, MEM, "gpu_stroke_scale_in_flight")


def test_gpu_stroke_scale_queries_and_stages(gpu_engine):
    sp.check_queries_and_stages(gpu_engine, "gpu_stroke_scale_queries")


def test_gpu_stroke_scale_refusals(gpu_engine):
    sp.check_refusals(gpu_engine, MEM, "gpu_stroke_scale_refusals")


def test_gpu_stroke_scale_estimator_and_auto_grow(gpu_engine):
    import vello_amd

    sp.check_estimator(lambda caps: vello_amd.Engine(device=0, capacities=caps), "gpu_stroke_scale_estimate")


def test_gpu_stroke_scale_engine_binding(gpu_engine):
    sp.check_engine_binding(gpu_engine, "gpu_stroke_scale_binding")


def test_gpu_stroke_scale_renderer_params(gpu_engine):
    sp.check_renderer("gpu_stroke_scale_renderer")
