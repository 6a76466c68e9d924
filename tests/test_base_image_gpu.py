"""Base images (vello_hip_set_base_image) on the MI355X: the cases of test_base_image_emu.py on the real kernels -- k_fine_base's
16-byte and dword global loads in start_list and blend_pass, in place, the allocation test of the enqueue -- and what only a GPU has:
a base image written, and then overwritten, by a torch op on a side stream."""
import numpy as np
import pytest

from tests import base_image_parity as bp
from tests import placement_parity as plp

pytestmark = pytest.mark.gpu
MEM = plp.TorchMemory()


def _gpu_engine_factory():
    import vello_amd

    return lambda caps: vello_amd.Engine(device=0, capacities=caps)


@pytest.mark.parametrize("config", sorted(bp.CONFIGS))
def test_gpu_base_image_matrix(gpu_engine, config):
    bp.check_matrix(gpu_engine, MEM, "gpu_base", config)


@pytest.mark.parametrize("aa", [0, 1, 2])
def test_gpu_base_image_brushes(gpu_engine, aa):
    bp.check_brushes(gpu_engine, MEM, "gpu_base_brushes", aa)


@pytest.mark.parametrize("aa", [1, 2])
def test_gpu_base_image_slices(gpu_engine, aa):
    bp.check_slices(gpu_engine, MEM, "gpu_base_slices", aa)


def test_gpu_base_image_blend_spill(gpu_engine):
    bp.check_blend_spill(gpu_engine, MEM, "gpu_base_blend")


@pytest.mark.parametrize("aa", [0, 1, 2])
def test_gpu_base_image_in_place(gpu_engine, aa):
    bp.check_in_place(gpu_engine, MEM, "gpu_base_in_place", aa)


@pytest.mark.parametrize("aa", [0, 2])
def test_gpu_base_image_damage_separate(gpu_engine, aa):
    bp.check_damage_separate(gpu_engine, MEM, "gpu_base_damage", aa)


def test_gpu_base_image_uniform_is_base_color(gpu_engine):
    bp.check_uniform(gpu_engine, MEM, "gpu_base_uniform")


def test_gpu_base_image_no_instances(gpu_engine):
    bp.check_no_instances(gpu_engine, MEM, "gpu_base_n0")


@pytest.mark.parametrize("aa", [0, 2])
def test_gpu_base_image_in_flight(gpu_engine, aa):
    bp.check_in_flight(bp.dp.in_flight_engine(_gpu_engine_factory()), MEM, "gpu_base_in_flight", aa)


def test_gpu_base_image_render_frame(gpu_engine):
    bp.check_render_frame(gpu_engine, MEM, "gpu_base_render_frame")


def test_gpu_base_image_out_none(gpu_engine):
    bp.check_out_none(gpu_engine, MEM, "gpu_base_out_none")


def test_gpu_base_image_host_target(gpu_engine):
    bp.check_host_target(gpu_engine, MEM, "gpu_base_host_target")


def test_gpu_base_image_morphed(gpu_engine):
    bp.check_morphed(gpu_engine, MEM, "gpu_base_morphed")


def test_gpu_base_image_retained_painted(gpu_engine):
    bp.check_retained_painted(gpu_engine, MEM, "gpu_base_retained")


def test_gpu_base_image_with_view(gpu_engine):
    bp.check_with_view(gpu_engine, MEM, "gpu_base_view")


def test_gpu_base_image_with_stroke_scale(gpu_engine):
    bp.check_with_stroke_scale(gpu_engine, MEM, "gpu_base_stroke")


def test_gpu_base_image_run_stages(gpu_engine):
    bp.check_run_stages(gpu_engine, MEM, "gpu_base_run_stages")


def test_gpu_base_image_failed_frame(gpu_engine):
    bp.check_failed_frame(_gpu_engine_factory(), MEM, "gpu_base_failed")


def test_gpu_base_image_refusals(gpu_engine):
    host = np.zeros(37 * 19 * 4 + 64, dtype=np.uint8)
    bp.check_refusals(gpu_engine, MEM, "gpu_base_refusals", host_address=host.ctypes.data + (-host.ctypes.data) % 16)


def test_gpu_base_image_engine_binding(gpu_engine):
    bp.check_engine_binding(gpu_engine, MEM, "gpu_base_binding")


def test_gpu_base_image_renderer(gpu_engine):
    bp.check_renderer(MEM, "gpu_base_renderer")


def test_gpu_base_image_ordering(gpu_engine):
    """The image is written by torch ops on a side stream passed as src_stream -- behind enough work that a frame which did not wait
    would read the bytes from before -- and overwritten on that stream once the frame is enqueued: the frame shows the first
    contents, whichever lane it runs on, with nothing waiting on the host in between."""
    import torch

    ex = bp.main_expect("clipped", 2)
    w, h = ex.w, ex.h
    pal = torch.from_numpy(np.ascontiguousarray(bp.palette_bytes(w, h))).to("cuda")
    image = torch.full((h, w, 4), 0x5A, dtype=torch.uint8, device="cuda")
    targets = [bp.Placed(MEM, w, h, w * 4, bp.LEAD, 190 + k) for k in range(2)]
    ballast = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    gpu_engine.upload_scene(ex.packed, ex.layout)
    gpu_engine.set_frames_in_flight(2)
    try:
        with torch.cuda.stream(side):
            for _ in range(8):
                ballast.add_(1.0)
            image.copy_(pal)
        gpu_engine.set_base_image(image, src_stream=side)
        for t in targets:
            gpu_engine.render_resident(w, h, bp.IGNORED_BASE, ex.aa, out=t.view)
        with torch.cuda.stream(side):
            image.fill_(0xC3)
        gpu_engine.set_base_image(None)
        assert gpu_engine.sync() == 0
        side.synchronize()
        for k, t in enumerate(targets):
            t.check(f"gpu_base_ordering_frame{k}", ex.image(), None, 0)
        assert (image.cpu().numpy() == 0xC3).all(), "the side stream's later write is not the image's last"
    finally:
        gpu_engine.set_base_image(None)
        gpu_engine.set_frames_in_flight(1)
