"""Target strides, offsets and non-square atlases on the MI355X (tests/placement_parity.py): the surfaces are torch tensors, filled on
torch's stream; torch.cuda.synchronize() runs before the engine renders into them."""
import pytest

from tests import placement_parity as pp

pytestmark = pytest.mark.gpu

MEM = pp.TorchMemory()


def _to_device(array):
    import torch

    t = torch.from_numpy(array).to("cuda")
    torch.cuda.synchronize()
    return t


def test_gpu_placement_matrix_reaches_every_store_path():
    pp.check_matrix_inputs()


@pytest.mark.parametrize("ti", range(len(pp.TARGETS)), ids=[f"{w}x{h}" for w, h in pp.TARGETS])
def test_gpu_placement_matrix(gpu_engine, ti):
    pp.check_matrix_target(gpu_engine, MEM, "gpu_place", ti)


def test_gpu_placement_render_host_odd_stride(gpu_engine):
    pp.check_render_host(gpu_engine, "gpu_place_render_host")


def test_gpu_placement_render_device(gpu_engine):
    pp.check_render_device(gpu_engine, MEM, "gpu_place_render_device")


def test_gpu_placement_render_frame(gpu_engine):
    pp.check_render_frame(gpu_engine, MEM, "gpu_place_render_frame")


def test_gpu_placement_render_instances(gpu_engine):
    pp.check_render_instances(gpu_engine, MEM, "gpu_place_render_instances")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_gpu_placement_renderer(gpu_engine, device):
    pp.check_renderer(MEM, f"gpu_place_renderer_{int(device)}", device=device)


@pytest.mark.parametrize("aa", [0, 1, 2])
def test_gpu_placement_brushes(gpu_engine, aa):
    from vello_amd import AaConfig

    pp.check_brushes(gpu_engine, MEM, f"gpu_place_brushes_aa{aa}", AaConfig(aa))


def test_gpu_placement_fine_slices(gpu_engine):
    pp.check_fine_slices(gpu_engine, MEM, "gpu_place_slices")


def test_gpu_placement_contact_sheet_in_flight(gpu_engine):
    pp.check_contact_sheet(gpu_engine, MEM, "gpu_place_sheet")


def test_gpu_placement_refusals(gpu_engine):
    pp.check_refusals(gpu_engine, MEM, "gpu_place_refused")


@pytest.mark.parametrize("which", range(len(pp.ATLASES)), ids=[f"{a[0]}x{a[1]}" for a in pp.ATLASES])
def test_gpu_atlas_not_square_write_image(gpu_engine, which):
    pp.check_atlas(gpu_engine, "gpu_atlas_write", which)


@pytest.mark.parametrize("which", range(len(pp.ATLASES)), ids=[f"{a[0]}x{a[1]}" for a in pp.ATLASES])
def test_gpu_atlas_not_square_copy_images(gpu_engine, which):
    pp.check_atlas(gpu_engine, "gpu_atlas_copy", which, device_source=_to_device)
