"""Hit testing (vello_hip_pick) on the MI355X: the checks of test_pick_emu.py on the real kernels, with device points and device
results in torch tensors, and device points written by a torch op on another stream and passed with src_stream."""
import numpy as np
import pytest

from tests import pick_parity as pk

pytestmark = pytest.mark.gpu


class _Dev:
    @staticmethod
    def to_device(a):
        import torch

        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")
        torch.cuda.synchronize()  # (the engine's streams do not wait for torch's)
        return t

    @staticmethod
    def target(w, h):
        import torch

        t = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return t

    @staticmethod
    def to_numpy(t):
        return t.cpu().numpy()

    @staticmethod
    def result(n, fill=0):
        import torch

        t = torch.full((n, 2), int(fill), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return t

    @staticmethod
    def result_numpy(r):
        return r.cpu().numpy().view(np.uint32)


def _host_memory(pts):
    """Host memory handed in as device memory, which the GPU build must refuse: pageable memory and pinned memory."""
    import torch

    pageable = np.ascontiguousarray(pts, dtype=np.float32).copy()
    pinned = torch.from_numpy(pageable.copy()).pin_memory()
    assert pinned.is_pinned() and not pinned.is_cuda
    return {"pageable": pageable, "pinned": pinned}


def _make_engine(caps):
    import vello_amd

    return vello_amd.Engine(device=0, capacities=caps)


def test_gpu_pick_square(gpu_engine):
    pk.check_hand_square(gpu_engine, "gpu_pick_square")


def test_gpu_pick_hand_shapes(gpu_engine):
    pk.check_hand_shapes(gpu_engine, "gpu_pick_shapes")


def test_gpu_pick_brush_fragments(gpu_engine):
    pk.check_brush_fragments(gpu_engine, "gpu_pick_brushes")


def test_gpu_pick_clip_fragments(gpu_engine):
    pk.check_clip_fragments(gpu_engine, "gpu_pick_clip_fragments")


def test_gpu_pick_clip_scene(gpu_engine):
    pk.check_clip_scene(gpu_engine, "gpu_pick_clips")


def test_gpu_pick_image(gpu_engine):
    pk.check_image(gpu_engine, "gpu_pick_image")


def test_gpu_pick_soup_shapes(gpu_engine):
    pk.check_soup_shapes(gpu_engine, "gpu_pick_soup")


def test_gpu_pick_draw_shapes(gpu_engine):
    pk.check_draw_shapes(gpu_engine, "gpu_pick_draws")


def test_gpu_pick_query_counts(gpu_engine):
    pk.check_query_counts(gpu_engine, "gpu_pick_counts")


def test_gpu_pick_instances(gpu_engine):
    pk.check_instances(gpu_engine, "gpu_pick_instances", _Dev)


def test_gpu_pick_which_frame(gpu_engine):
    pk.check_which_frame(gpu_engine, "gpu_pick_which", _Dev)


def test_gpu_pick_sources(gpu_engine):
    pk.check_sources(gpu_engine, "gpu_pick_sources", _Dev)


def test_gpu_pick_source_stream(gpu_engine):
    """Device points written by a torch op on another stream, passed as src_stream: the pick waits for the write."""
    import torch

    from vello_amd import AaConfig

    e = gpu_engine
    w, h = 120, 90
    o, _ = pk.scene_frame(e, pk.resolve(pk.clip_scene()), w, h, AaConfig.Msaa8)
    pts = pk.probe_points(w, h, 15, step=5)
    a = _Dev.to_device(pts)
    d = torch.zeros_like(a)
    out = _Dev.result(len(pts))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d.copy_(a * 1.0)  # (a kernel on the side stream writes the points)
        r = e.pick(d, out=out, src_stream=side)
    assert r is out
    assert np.array_equal(_Dev.result_numpy(out), pk.reference(o, pts))  # (the call blocks: the result is written)
    side.synchronize()
    assert e.sync() == 0


def test_gpu_pick_refusals(gpu_engine):
    pk.check_refusals(_make_engine, "gpu_pick_refusals", _Dev, host_memory=_host_memory)


def test_gpu_pick_failed_frame(gpu_engine):
    pk.check_failed_frame(_make_engine, "gpu_pick_failed", _Dev)
