"""Retained instance lists on the MI355X: the cases of test_retained_instances_emu.py on the real kernels, with device poses in torch
tensors on the GPU; poses written by a torch op on another stream; and the symbol map that only fits here -- 64 fragments, 30 000
instances, 1600 x 1600, MSAA16 -- for one frame under a turned pose set from a device tensor, every intermediate against the oracle."""
import numpy as np
import pytest

from tests import retained_parity as rp

pytestmark = pytest.mark.gpu


def _target(w, h):
    import torch

    t = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the engine's streams do not wait for torch's)
    return t


def _numpy(t):
    return t.cpu().numpy()


def _device(poses):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32)).to("cuda")
    torch.cuda.synchronize()
    return t


def _host_memory(poses):
    """Host memory handed in as device memory, which the GPU build must refuse: ordinary pageable memory, whose address the runtime
    does not know, and pinned memory, which it knows and reports as host memory."""
    import torch

    pageable = np.ascontiguousarray(poses, dtype=np.float32)
    pinned = torch.from_numpy(pageable).pin_memory()
    assert pinned.is_pinned() and not pinned.is_cuda
    return {"pageable": pageable, "pinned": pinned}


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_gpu_retained_polygons_polylines(gpu_engine, stroke_kernel):
    rp.check_frame(gpu_engine, f"gpu_ret_lines_{int(stroke_kernel)}", ["polygons", "polylines"], flags={"stroke_kernel": stroke_kernel}, n=5, base=rp.WHITE,
                   device=_device)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
def test_gpu_retained_curves(gpu_engine, which):
    rp.check_frame(gpu_engine, f"gpu_ret_curves_{which}", ["cardioid", "stroke_styles", "funky"], flags={which: True}, n=5, base=rp.WHITE, source="device",
                   device=_device)


def test_gpu_retained_brushes(gpu_engine):
    rp.check_frame(gpu_engine, "gpu_ret_brushes", ["solid", "linear", "radial", "sweep", "image", "blur"], n=13, paints=rp.some_paints, source="device",
                   device=_device)


def test_gpu_retained_layers(gpu_engine):
    rp.check_frame(gpu_engine, "gpu_ret_layers", ["clip", "blend", "clip_blend", "solid"], n=9, device=_device)


def test_gpu_retained_msaa8_painted(gpu_engine):
    from vello_amd import AaConfig

    rp.check_frame(gpu_engine, "gpu_ret_msaa8", ["solid", "blur", "clip"], n=9, aas=(AaConfig.Msaa8,), paints=rp.some_paints, w=128, h=96, device=_device)


@pytest.mark.parametrize("view,cull", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("source", ["host", "device"])
def test_gpu_retained_equals_instance_frame(gpu_engine, view, cull, source):
    from vello_amd import Affine

    v = Affine.translate(20.0, -9.0) * Affine.rotate(0.25) * Affine.scale(1.3) if view else None
    rp.check_bitwise(gpu_engine, f"gpu_ret_bits_{int(view)}{int(cull)}_{source}", view=v, cull=cull, source=source, device=_device, painted=source == "host")


def test_gpu_retained_kernel_shapes(gpu_engine):
    rp.check_shapes(gpu_engine, "gpu_ret_shapes", device=_device)


def test_gpu_retained_pose_sources(gpu_engine):
    rp.check_sources(gpu_engine, "gpu_ret_sources", device=_device)


def test_gpu_retained_source_stream(gpu_engine):
    """Device poses written by a torch op on another stream, passed as src_stream, and overwritten on that stream right after the
    call: the frame waits for the write and shows the first contents; nothing waits on the host in between."""
    import torch

    import vello_amd
    from tests import instance_parity as ip
    from vello_amd import AaConfig

    e = gpu_engine
    w, h, aa = 96, 64, AaConfig.Msaa8
    lib = vello_amd.FragmentLibrary([ip.polygon(5), ip.polygon(8)])
    lib.upload(e)
    inst = ip.scatter(np.random.default_rng(2), 6, 2, w, h, scale=(0.8, 2.0))
    first, second = rp.turned(inst, w, h, 1), rp.turned(inst, w, h, 2)
    e.retain_instances(inst)
    a, b = _device(first), _device(second)
    d = torch.zeros_like(a)
    out = _target(w, h)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d.copy_(a * 1.0)  # (a kernel on the side stream writes the poses)
        e.render_retained(w, h, rp.BLACK, aa, transforms=d, out=out, src_stream=side)
        d.copy_(b)
    assert e.sync() == 0
    side.synchronize()
    assert np.array_equal(_numpy(out), rp.want(lib, rp.posed(inst, first), w, h, rp.BLACK, aa)), "the frame does not show the poses it was enqueued with"
    assert np.array_equal(_numpy(d), second)


def test_gpu_retained_life_cycle(gpu_engine):
    rp.check_life_cycle(gpu_engine, "gpu_ret_life", _target, _numpy, device=_device)


def test_gpu_retained_pool_overflow(gpu_engine):
    import vello_amd

    rp.check_overflow(lambda caps: vello_amd.Engine(device=0, capacities=caps), "gpu_ret_overflow", device=_device)


def test_gpu_retained_errors(gpu_engine):
    rp.check_errors(gpu_engine, "gpu_ret_errors", _target, _numpy, device=_device, host_memory=_host_memory)


def test_gpu_retained_device_nan(gpu_engine):
    rp.check_device_nan(gpu_engine, "gpu_ret_nan", _target, _numpy, device=_device)


def test_gpu_retained_symbol_map(gpu_engine):
    import bench
    import vello_amd
    from oracle.oracle import Oracle
    from tests import instance_parity as ip
    from vello_amd import AaConfig

    lib = vello_amd.FragmentLibrary(ip.symbol_fragments())
    inst = ip.symbol_instances(0x5EED0003)
    poses = np.ascontiguousarray(ip.symbol_instances(0x5EED0003, phase=0.35)["transform"], dtype=np.float32)
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    rp.compare_retained_frame(eng, lib, ip.instance_list(inst), poses, 1600, 1600, rp.WHITE, AaConfig.Msaa16, "gpu_ret_symbol_map", source="device",
                              device=_device, oracle=Oracle(capacity_scale=8, auto_grow=True))
