"""Per-instance paints on the MI355X: the checks of tests/paint_parity.py on the real kernels, and a cut of the symbol map -- 2 000
instances over 400 x 400, MSAA16, every instance painted from a palette -- bytes and image against the oracle."""
import numpy as np
import pytest

from tests import paint_parity as pp

pytestmark = pytest.mark.gpu


def _target(w, h):
    import torch

    return torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")


def _numpy(t):
    return t.cpu().numpy()


def test_gpu_paints_mask_bits(gpu_engine):
    pp.check_mask_bits(gpu_engine, "gpu_paint_mask")


def test_gpu_paints_chunk_boundaries(gpu_engine):
    pp.check_chunk_boundaries(gpu_engine, "gpu_paint_chunks")


def test_gpu_paints_long_chunks(gpu_engine):
    pp.check_long_chunks(gpu_engine, "gpu_paint_long", 2)


def test_gpu_paints_unstaged(gpu_engine):
    pp.check_unstaged(gpu_engine, "gpu_paint_unstaged")


def test_gpu_paints_no_colour_words(gpu_engine):
    pp.check_no_colour_words(gpu_engine, "gpu_paint_words")


def test_gpu_paints_colour_values(gpu_engine):
    pp.check_colour_values(gpu_engine, "gpu_paint_values")


def test_gpu_paints_occlusion(gpu_engine):
    pp.check_occlusion(gpu_engine, "gpu_paint_occlusion")


def test_gpu_paints_host_agreement(gpu_engine):
    pp.check_host_agreement(gpu_engine, "gpu_paint_host")


def test_gpu_paints_null_and_empty(gpu_engine):
    pp.check_null_and_empty(gpu_engine, "gpu_paint_null")


def test_gpu_paints_life_cycle(gpu_engine):
    pp.check_life_cycle(gpu_engine, "gpu_paint_life", _target, _numpy)


def test_gpu_paints_errors(gpu_engine):
    pp.check_errors(gpu_engine, "gpu_paint_errors", _target, _numpy)


def test_gpu_paints_symbol_map_cut(gpu_engine):
    import vello_amd
    from tests import instance_parity as ip
    from vello_amd import AaConfig, PAINT_DTYPE

    lib = vello_amd.FragmentLibrary(ip.symbol_fragments())
    n, size = 2000, 400
    inst = ip.symbol_instances(0x5EED0004, n=n, size=float(size))
    palette = np.array([0xFF0000FF, 0xFF00FF00, 0xFFFF0000, 0x80404000, 0xFF20C0F0, 0xC0303060, 0xFFFFFFFF], dtype=np.uint32)
    paints = np.zeros(n, dtype=PAINT_DTYPE)
    paints["flags"] = 1
    paints["rgba"] = palette[np.arange(n) % len(palette)]
    gpu_engine.set_auto_grow(True)
    packed, plain, layout = pp.check_bytes(gpu_engine, "gpu_paint_symbol_map", lib, ip.instance_list(inst), paints, size, size, aa=AaConfig.Msaa16)
    dd = packed.view(np.uint32)[layout.draw_data_base: layout.transform_base]
    assert len(dd) == n and np.array_equal(dd, paints["rgba"])
