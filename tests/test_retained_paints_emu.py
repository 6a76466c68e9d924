"""Per-frame paints of retained instance lists (vello_hip_render_retained_painted) on the SIMT-emulated build of the kernel sources:
k_instance_paints' frames against the CPU oracle through compare_frame and, bit for bit, against vello_hip_render_instances_painted;
kernel shapes, life cycle, refusals and pool overflow (tests/repaint_parity.py).  Device memory is host memory here: a numpy array
passed with paints_is_device / transforms_is_device stands for device paints / poses."""
import numpy as np
import pytest

from tests import repaint_parity as rq


def _target(w, h):
    return np.zeros((h, w, 4), dtype=np.uint8)  # (stands for device memory in the emulated build)


def _same(t):
    return t


@pytest.mark.parametrize("pose_source", ["host", "device"])
@pytest.mark.parametrize("paint_source", ["host", "device"])
def test_emu_repaint_oracle(emu_engine, pose_source, paint_source):
    rq.check_oracle(emu_engine, f"emu_repaint_{pose_source}_{paint_source}", pose_source, paint_source)


@pytest.mark.parametrize("view,cull", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("paint_source", ["host", "device"])
def test_emu_repaint_equals_painted_instance_frame(emu_engine, view, cull, paint_source):
    from vello_amd import Affine

    v = Affine.translate(20.0, -9.0) * Affine.rotate(0.25) * Affine.scale(1.3) if view else None
    rq.check_bitwise(emu_engine, f"emu_repaint_bits_{int(view)}{int(cull)}_{paint_source}", view=v, cull=cull,
                     pose_source="device" if paint_source == "host" else "host", paint_source=paint_source)


def test_emu_repaint_occlusion_follows_frame_colours(emu_engine):
    rq.check_occlusion(emu_engine, "emu_repaint_occlusion")


def test_emu_repaint_all_keep_is_unpainted_frame(emu_engine):
    rq.check_all_keep(emu_engine, "emu_repaint_keep")


def test_emu_repaint_kernel_shapes(emu_engine):
    rq.check_shapes(emu_engine, "emu_repaint_shapes")


def test_emu_repaint_life_cycle(emu_engine):
    rq.check_life_cycle(emu_engine, "emu_repaint_life", _target, _same)


def test_emu_repaint_source_stream(emu_engine):
    rq.check_source_stream_emu(emu_engine, "emu_repaint_stream")


def test_emu_repaint_errors(emu_engine):
    rq.check_errors(emu_engine, "emu_repaint_errors", _target, _same)


def test_emu_repaint_no_masks(emu_engine):
    rq.check_no_masks(emu_engine, "emu_repaint_no_masks", _target, _same)


def test_emu_repaint_device_flags(emu_engine):
    rq.check_device_flags(emu_engine, "emu_repaint_flags", _target, _same)


def test_emu_repaint_pool_overflow(emu_engine):
    import vello_amd

    rq.check_overflow(lambda caps: vello_amd.Engine(capacities=caps), "emu_repaint_overflow")
