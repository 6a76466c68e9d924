"""Retained instance lists (vello_hip_retain_instances / vello_hip_render_retained / vello_hip_release_retained) on the SIMT-emulated
build of the kernel sources: k_instance_transforms' frames against the CPU oracle through compare_frame and, bit for bit, against
vello_hip_render_instances_painted; kernel shapes, pose sources, life cycle and refusals (tests/retained_parity.py).  Device memory is
host memory here: a numpy array passed with transforms_is_device stands for device poses.  The symbol map is the GPU suite's."""
import numpy as np
import pytest

from tests import retained_parity as rp


def _target(w, h):
    return np.zeros((h, w, 4), dtype=np.uint8)  # (stands for device memory in the emulated build)


def _same(t):
    return t


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_emu_retained_polygons_polylines(emu_engine, stroke_kernel):
    rp.check_frame(emu_engine, f"emu_ret_lines_{int(stroke_kernel)}", ["polygons", "polylines"], flags={"stroke_kernel": stroke_kernel}, n=5, base=rp.WHITE)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
def test_emu_retained_curves(emu_engine, which):
    rp.check_frame(emu_engine, f"emu_ret_curves_{which}", ["cardioid", "stroke_styles", "funky"], flags={which: True}, n=5, base=rp.WHITE, source="device")


def test_emu_retained_brushes(emu_engine):
    rp.check_frame(emu_engine, "emu_ret_brushes", ["solid", "linear", "radial", "sweep", "image", "blur"], n=13, paints=rp.some_paints, source="device")


def test_emu_retained_layers(emu_engine):
    rp.check_frame(emu_engine, "emu_ret_layers", ["clip", "blend", "clip_blend", "solid"], n=9)


def test_emu_retained_msaa8_painted(emu_engine):
    from vello_amd import AaConfig

    rp.check_frame(emu_engine, "emu_ret_msaa8", ["solid", "blur", "clip"], n=9, aas=(AaConfig.Msaa8,), paints=rp.some_paints, w=128, h=96)


@pytest.mark.parametrize("view,cull", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("source", ["host", "device"])
def test_emu_retained_equals_instance_frame(emu_engine, view, cull, source):
    from vello_amd import Affine

    v = Affine.translate(20.0, -9.0) * Affine.rotate(0.25) * Affine.scale(1.3) if view else None
    rp.check_bitwise(emu_engine, f"emu_ret_bits_{int(view)}{int(cull)}_{source}", view=v, cull=cull, source=source, painted=source == "host")


def test_emu_retained_kernel_shapes(emu_engine):
    rp.check_shapes(emu_engine, "emu_ret_shapes")


def test_emu_retained_pose_sources(emu_engine):
    rp.check_sources(emu_engine, "emu_ret_sources")


def test_emu_retained_source_stream(emu_engine):
    """Device poses with a src_stream, overwritten right after the call: the frame shows the first contents (the emulator runs a
    launch when it is enqueued; the GPU twin has a torch op on another stream write the poses)."""
    import vello_amd
    from tests import instance_parity as ip
    from vello_amd import AaConfig

    e = emu_engine
    w, h, aa = 96, 64, AaConfig.Msaa8
    lib = vello_amd.FragmentLibrary([ip.polygon(5), ip.polygon(8)])
    lib.upload(e)
    inst = ip.scatter(np.random.default_rng(2), 6, 2, w, h, scale=(0.8, 2.0))
    first, second = rp.turned(inst, w, h, 1), rp.turned(inst, w, h, 2)
    e.retain_instances(inst)
    d = first.copy()
    e.render_retained(w, h, rp.BLACK, aa, transforms=d, src_stream=e.stream() or 1, transforms_is_device=True)
    d[...] = second
    assert e.sync() == 0
    got = e.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)
    assert np.array_equal(got, rp.want(lib, rp.posed(inst, first), w, h, rp.BLACK, aa))


def test_emu_retained_life_cycle(emu_engine):
    rp.check_life_cycle(emu_engine, "emu_ret_life", _target, _same)


def test_emu_retained_pool_overflow(emu_engine):
    import vello_amd

    rp.check_overflow(lambda caps: vello_amd.Engine(capacities=caps), "emu_ret_overflow")


def test_emu_retained_errors(emu_engine):
    rp.check_errors(emu_engine, "emu_ret_errors", _target, _same)


def test_emu_retained_device_nan(emu_engine):
    rp.check_device_nan(emu_engine, "emu_ret_nan", _target, _same)
