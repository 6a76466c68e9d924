"""Per-frame path data (vello_hip_render_resident_morphed) on the MI355X: the cases of test_path_morph_emu.py on the real kernels, the
tiger at 512 x 512, and what only a GPU shows -- a device source written and overwritten on a caller's stream."""
import pytest

from tests import morph_parity as mp

pytestmark = pytest.mark.gpu

MEM = mp.GpuMemory()


@pytest.mark.parametrize("n_words", mp.SIZES)
def test_gpu_morph_sizes_and_alignment(gpu_engine, n_words):
    mp.check_size(gpu_engine, MEM, "gpu_morph_size", n_words)


def test_gpu_morph_odd_sizes(gpu_engine):
    mp.check_odd_sizes(gpu_engine, MEM, "gpu_morph_odd")


def test_gpu_morph_unaligned_scene_stream(gpu_engine):
    mp.check_unaligned_scene_stream(gpu_engine, MEM, "gpu_morph_unaligned")


def test_gpu_morph_arithmetic(gpu_engine):
    mp.check_arithmetic(gpu_engine, MEM, "gpu_morph_arith")


def test_gpu_morph_verbatim_bits(gpu_engine):
    mp.check_verbatim_bits(gpu_engine, MEM, "gpu_morph_bits")


def test_gpu_morph_front_fusion(gpu_engine):
    mp.check_front_fusion(gpu_engine, MEM, "gpu_morph_front")


def test_gpu_morph_indexed(gpu_engine):
    mp.check_indexed(gpu_engine, MEM, "gpu_morph_indexed")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_gpu_morph_strokes(gpu_engine, stroke_kernel):
    mp.check_strokes(gpu_engine, MEM, "gpu_morph_strokes", stroke_kernel)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
@pytest.mark.parametrize("case", range(3))
def test_gpu_morph_curves(gpu_engine, case, which):
    mp.check_curves(gpu_engine, MEM, "gpu_morph_curves", which, case)


def test_gpu_morph_tiger(gpu_engine):
    mp.check_tiger(gpu_engine, MEM, "gpu_morph_tiger")


def test_gpu_morph_view(gpu_engine):
    mp.check_view(gpu_engine, MEM, "gpu_morph_view")


def test_gpu_morph_culled(gpu_engine):
    mp.check_culled(gpu_engine, MEM, "gpu_morph_culled")


def test_gpu_morph_in_flight(gpu_engine):
    mp.check_in_flight(gpu_engine, MEM, "gpu_morph_in_flight")


def test_gpu_morph_device_source_ordering(gpu_engine):
    mp.check_ordering(gpu_engine, "gpu_morph_ordering")


def test_gpu_morph_run_stages_and_queries(gpu_engine):
    mp.check_run_stages_and_queries(gpu_engine, MEM, "gpu_morph_stages")


def test_gpu_morph_refusals(gpu_engine):
    mp.check_refusals(gpu_engine, MEM, "gpu_morph_refusals")


def test_gpu_morph_bindings(gpu_engine):
    mp.check_bindings(gpu_engine, MEM, "gpu_morph_bindings")
