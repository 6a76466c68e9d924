"""Scene instances on the MI355X: the cases of test_scene_instances_emu.py on the real kernels, and the symbol map that only fits here
-- 64 fragments drawn from the road map's distributions, 30 000 instances, 1600 x 1600, MSAA16, every intermediate against the oracle."""
import pytest

from tests import instance_parity as ip

pytestmark = pytest.mark.gpu


def _target(w, h):
    import torch

    return torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")


def _numpy(t):
    return t.cpu().numpy()


def test_gpu_instances_tag_shapes(gpu_engine):
    ip.check_tag_shapes(gpu_engine, "gpu_inst_tags")


def test_gpu_instances_many(gpu_engine):
    ip.check_many(gpu_engine, "gpu_inst_many")


def test_gpu_instances_one_tag_chunks(gpu_engine):
    ip.check_one_tag_chunks(gpu_engine, "gpu_inst_one_tag")


def test_gpu_instances_long_chunks(gpu_engine):
    ip.check_long_chunks(gpu_engine, "gpu_inst_long", 2)


def test_gpu_instances_host_agreement(gpu_engine):
    ip.check_host_agreement(gpu_engine, "gpu_inst_host")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_gpu_instances_polygons_polylines(gpu_engine, stroke_kernel):
    ip.check_frame(gpu_engine, f"gpu_inst_lines_{int(stroke_kernel)}", ["polygons", "polylines"], flags={"stroke_kernel": stroke_kernel}, n=5, base=ip.WHITE)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
def test_gpu_instances_curves(gpu_engine, which):
    ip.check_frame(gpu_engine, f"gpu_inst_curves_{which}", ["cardioid", "stroke_styles", "funky"], flags={which: True}, n=5, base=ip.WHITE,
                   in_flight=2 if which == "flatten_alone" else 1)


def test_gpu_instances_brushes(gpu_engine):
    ip.check_frame(gpu_engine, "gpu_inst_brushes", ["solid", "linear", "radial", "sweep", "image", "blur"], n=13)


def test_gpu_instances_layers(gpu_engine):
    ip.check_frame(gpu_engine, "gpu_inst_layers", ["clip", "blend", "clip_blend", "solid"], n=9)


def test_gpu_instances_front_fusion(gpu_engine):
    ip.check_front_fusion(gpu_engine, "gpu_inst_front")


def test_gpu_instances_life_cycle(gpu_engine):
    ip.check_life_cycle(gpu_engine, "gpu_inst_life", _target, _numpy)


def test_gpu_instances_errors(gpu_engine):
    ip.check_errors(gpu_engine, "gpu_inst_errors", _target, _numpy)


def test_gpu_instances_symbol_map(gpu_engine):
    import bench
    import vello_amd
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    lib = vello_amd.FragmentLibrary(ip.symbol_fragments())
    inst = ip.symbol_instances(0x5EED0003)
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    ip.compare_instance_frame(eng, lib, ip.instance_list(inst), 1600, 1600, ip.WHITE, AaConfig.Msaa16, "gpu_inst_symbol_map",
                              oracle=Oracle(capacity_scale=8, auto_grow=True))
