"""Per-frame paints of retained instance lists on the MI355X: the cases of test_retained_paints_emu.py on the real kernels, with
device paints and poses in torch tensors on the GPU, and paints and poses written by torch ops on another stream."""
import numpy as np
import pytest

from tests import repaint_parity as rq
from tests import retained_parity as rp

pytestmark = pytest.mark.gpu


def _target(w, h):
    import torch

    t = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the engine's streams do not wait for torch's)
    return t


def _numpy(t):
    return t.cpu().numpy()


def _poses(poses):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32)).to("cuda")
    torch.cuda.synchronize()
    return t


def _paints(paints):
    """A PAINT_DTYPE array as an int32 tensor of n x 2 (flags, rgba) on the GPU."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(paints).view(np.int32).reshape(-1, 2).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def _host_memory(paints):
    """Host memory handed in as device memory, which the GPU build must refuse: pageable and pinned."""
    import torch

    pageable = np.ascontiguousarray(paints).view(np.int32).reshape(-1, 2).copy()
    pinned = torch.from_numpy(pageable).pin_memory()
    assert pinned.is_pinned() and not pinned.is_cuda
    return {"pageable": pageable, "pinned": pinned}


@pytest.mark.parametrize("pose_source", ["host", "device"])
@pytest.mark.parametrize("paint_source", ["host", "device"])
def test_gpu_repaint_oracle(gpu_engine, pose_source, paint_source):
    rq.check_oracle(gpu_engine, f"gpu_repaint_{pose_source}_{paint_source}", pose_source, paint_source, device_poses=_poses, device_paints=_paints)


@pytest.mark.parametrize("view,cull", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("paint_source", ["host", "device"])
def test_gpu_repaint_equals_painted_instance_frame(gpu_engine, view, cull, paint_source):
    from vello_amd import Affine

    v = Affine.translate(20.0, -9.0) * Affine.rotate(0.25) * Affine.scale(1.3) if view else None
    rq.check_bitwise(gpu_engine, f"gpu_repaint_bits_{int(view)}{int(cull)}_{paint_source}", view=v, cull=cull,
                     pose_source="device" if paint_source == "host" else "host", paint_source=paint_source, device_poses=_poses, device_paints=_paints)


def test_gpu_repaint_occlusion_follows_frame_colours(gpu_engine):
    rq.check_occlusion(gpu_engine, "gpu_repaint_occlusion", device_paints=_paints)


def test_gpu_repaint_all_keep_is_unpainted_frame(gpu_engine):
    rq.check_all_keep(gpu_engine, "gpu_repaint_keep", device_paints=_paints)


def test_gpu_repaint_kernel_shapes(gpu_engine):
    rq.check_shapes(gpu_engine, "gpu_repaint_shapes", device_poses=_poses, device_paints=_paints)


def test_gpu_repaint_life_cycle(gpu_engine):
    rq.check_life_cycle(gpu_engine, "gpu_repaint_life", _target, _numpy, device_poses=_poses, device_paints=_paints)


def test_gpu_repaint_source_stream(gpu_engine):
    """Device paints and poses written by torch ops on another stream, passed as src_stream, and overwritten on that stream right
    after the call: the frame waits for the writes and shows the first contents; nothing waits on the host in between."""
    import torch

    import vello_amd
    from tests import instance_parity as ip
    from vello_amd import AaConfig

    e = gpu_engine
    w, h, aa = 96, 64, AaConfig.Msaa8
    lib = vello_amd.FragmentLibrary([ip.polygon(5), ip.polygon(8)])
    lib.upload(e)
    inst = ip.scatter(np.random.default_rng(2), 6, 2, w, h, scale=(0.8, 2.0))
    n = len(inst)
    x1, x2 = rp.turned(inst, w, h, 1), rp.turned(inst, w, h, 2)
    p1, p2 = rq.paint_list(rq.frame_paints(n, 0), n), rq.paint_list(rq.frame_paints(n, 1), n)
    e.retain_instances(inst)
    xa, xb, pa, pb = _poses(x1), _poses(x2), _paints(p1), _paints(p2)
    dx, dp = torch.zeros_like(xa), torch.zeros_like(pa)
    out = _target(w, h)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dx.copy_(xa * 1.0)  # (kernels on the side stream write the poses and the paints)
        dp.copy_(pa + 0)
        e.render_retained(w, h, rq.BLACK, aa, transforms=dx, paints=dp, out=out, src_stream=side)
        dx.copy_(xb)
        dp.copy_(pb)
    assert e.sync() == 0
    side.synchronize()
    assert np.array_equal(_numpy(out), rq.want(lib, inst, x1, p1, w, h, rq.BLACK, aa)), "the frame does not show the paints and poses it was enqueued with"
    assert np.array_equal(_numpy(dx), x2) and np.array_equal(_numpy(dp), p2.view(np.int32).reshape(-1, 2))
    # device paints alone (host poses) behind the side stream
    with torch.cuda.stream(side):
        dp.copy_(pa + 0)
        e.render_retained(w, h, rq.BLACK, aa, transforms=x2, paints=dp, out=out, src_stream=side)
        dp.copy_(pb)
    assert e.sync() == 0
    side.synchronize()
    assert np.array_equal(_numpy(out), rq.want(lib, inst, x2, p1, w, h, rq.BLACK, aa)), "device paints with host poses behind src_stream"


def test_gpu_repaint_errors(gpu_engine):
    rq.check_errors(gpu_engine, "gpu_repaint_errors", _target, _numpy, device_poses=_poses, device_paints=_paints, host_memory=_host_memory)


def test_gpu_repaint_no_masks(gpu_engine):
    rq.check_no_masks(gpu_engine, "gpu_repaint_no_masks", _target, _numpy)


def test_gpu_repaint_device_flags(gpu_engine):
    rq.check_device_flags(gpu_engine, "gpu_repaint_flags", _target, _numpy, device_paints=_paints)


def test_gpu_repaint_pool_overflow(gpu_engine):
    import vello_amd

    rq.check_overflow(lambda caps: vello_amd.Engine(device=0, capacities=caps), "gpu_repaint_overflow", device_poses=_poses, device_paints=_paints)
