"""The scene index (vello_hip_scene_index_builds) on the MI355X: the cases of test_scene_index_emu.py on the real kernels -- the merged
first flatten launch of frames in flight, k_frame_begin, lanes that truly overlap."""
import pytest

from tests import scene_index_parity as sp

pytestmark = pytest.mark.gpu


def _target(w, h):
    import torch

    return torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")


def _numpy(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("in_flight", [1, 3])
@pytest.mark.parametrize("kernels", ["flatten_coop", "flatten_alone"])
@pytest.mark.parametrize("which", sp.CASES)
def test_gpu_scene_index_twin(gpu_engine, which, kernels, in_flight):
    sp.check_twin(gpu_engine, which, kernels, in_flight, f"gpu_index_{which}_{kernels}_{in_flight}", _target, _numpy)


def test_gpu_scene_index_many_frames(gpu_engine):
    sp.check_many_frames(gpu_engine, "gpu_index_many")


def test_gpu_scene_index_invalidation(gpu_engine):
    import vello_amd

    sp.check_invalidation(gpu_engine, vello_amd.Engine(device=0), "gpu_index_invalidation", _target, _numpy)


def test_gpu_scene_index_first_frames(gpu_engine):
    sp.check_first_frames(gpu_engine, "gpu_index_first", _target, _numpy)


def test_gpu_scene_index_overrun(gpu_engine):
    sp.check_overrun(gpu_engine, "gpu_index_overrun")
