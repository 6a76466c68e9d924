"""Marquee selection (vello_hip_pick_rect) on the MI355X: the checks of test_pick_rect_emu.py on the real kernels, with device outputs
in torch tensors, and a selection turned into the next retained frame's paints without leaving the device."""
import numpy as np
import pytest

from tests import pick_parity as pk
from tests import region_parity as rg
from tests.test_pick_gpu import _Dev as _PickDev

pytestmark = pytest.mark.gpu


class _Dev(_PickDev):
    @staticmethod
    def words(n, fill=0):
        import torch

        t = torch.full((n,), int(np.int32(np.uint32(fill))), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return t

    @staticmethod
    def words_numpy(r):
        return r.cpu().numpy().view(np.uint32)


def _host_memory(n):
    """Host memory handed in as device memory, which the GPU build must refuse: pageable memory and pinned memory."""
    import torch

    pageable = np.zeros(n, dtype=np.uint32)
    pinned = torch.from_numpy(np.zeros(n, dtype=np.int32)).pin_memory()
    assert pinned.is_pinned() and not pinned.is_cuda
    return {"pageable": pageable, "pinned": pinned}


def _make_engine(caps):
    import vello_amd

    return vello_amd.Engine(device=0, capacities=caps)


def test_gpu_pick_rect_square(gpu_engine):
    rg.check_hand_square(gpu_engine, "gpu_rect_square")


def test_gpu_pick_rect_hand_shapes(gpu_engine):
    rg.check_hand_shapes(gpu_engine, "gpu_rect_shapes")


def test_gpu_pick_rect_brush_fragments(gpu_engine):
    rg.check_brush_fragments(gpu_engine, "gpu_rect_brushes")


def test_gpu_pick_rect_clip_scene(gpu_engine):
    rg.check_clip_scene(gpu_engine, "gpu_rect_clips")


def test_gpu_pick_rect_clip_fragments(gpu_engine):
    rg.check_clip_fragments(gpu_engine, "gpu_rect_clip_fragments")


def test_gpu_pick_rect_image(gpu_engine):
    rg.check_image(gpu_engine, "gpu_rect_image")


def test_gpu_pick_rect_soup_shapes(gpu_engine):
    rg.check_soup_shapes(gpu_engine, "gpu_rect_soup")


def test_gpu_pick_rect_draw_shapes(gpu_engine):
    rg.check_draw_shapes(gpu_engine, "gpu_rect_draws")


def test_gpu_pick_rect_three_draws(gpu_engine):
    rg.check_three_draws(gpu_engine, "gpu_rect_three")


def test_gpu_pick_rect_instances(gpu_engine):
    rg.check_instances(gpu_engine, "gpu_rect_instances", _Dev)


def test_gpu_pick_rect_retained_painted(gpu_engine):
    rg.check_retained_painted(gpu_engine, "gpu_rect_painted", _Dev)


def test_gpu_pick_rect_culling(gpu_engine):
    rg.check_culling(gpu_engine, "gpu_rect_cull")


def test_gpu_pick_rect_which_frame(gpu_engine):
    rg.check_which_frame(gpu_engine, "gpu_rect_which", _Dev)


def test_gpu_pick_rect_sinks(gpu_engine):
    rg.check_sinks(gpu_engine, "gpu_rect_sinks", _Dev)


def test_gpu_pick_rect_refusals(gpu_engine):
    rg.check_refusals(_make_engine, "gpu_rect_refusals", _Dev, host_memory=_host_memory)


def test_gpu_pick_rect_failed_frame(gpu_engine):
    rg.check_failed_frame(_make_engine, "gpu_rect_failed", _Dev)


def test_gpu_pick_rect_selection_paints_the_next_frame(gpu_engine):
    """The instance words, left in device memory, become the paints of the next retained frame by a torch op: the selected instances
    turn white, the others keep their colours, and the host never reads the selection."""
    import torch

    import vello_amd
    from tests import retained_parity as rp
    from vello_amd import AaConfig

    e = gpu_engine
    lib = pk.instance_library()
    lib.upload(e)
    w, h, aa = 128, 96, AaConfig.Area
    inst = pk.instance_list(lib, w, h, 3)
    off = pk.draw_offsets(lib, inst)
    e.retain_instances(inst)
    rp.frame(e, w, h, pk.BLACK, aa, None, "rest")
    rect = (20.0, 10.0, 100.0, 80.0)
    words = _Dev.words(len(inst), 0x5A5A5A5A)
    _, got, counts = e.pick_rect(rect, instances_out=words, draws=False)
    assert got is words
    o = pk.run_oracle(*rp.compose(lib, inst), w, h, pk.BLACK, aa, lib)
    want = rg.reference(o, rect, off)
    assert np.array_equal(_Dev.words_numpy(words), want[1]) and counts == want[2] and 0 < counts["instances_touched"] < len(inst)
    paints = torch.stack([(words & 1), torch.full_like(words, -1)], dim=1).contiguous()  # (PAINT_SOLID where TOUCHED, white)
    torch.cuda.synchronize()
    target = _Dev.target(w, h)
    e.render_retained(w, h, pk.BLACK, aa, paints=paints, out=target)
    assert e.sync() == 0
    host_paints = [0xFFFFFFFF if v & 1 else None for v in want[1]]
    o_p = pk.run_oracle(*rp.compose(lib, inst, host_paints), w, h, pk.BLACK, aa, lib)
    assert np.array_equal(_Dev.to_numpy(target), o_p.image)
