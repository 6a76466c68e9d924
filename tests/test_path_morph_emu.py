"""Per-frame path data (vello_hip_render_resident_morphed) on the SIMT-emulated build of the kernel sources: the blend kernel's sizes,
alignments and arithmetic, every path a frame can take, the other per-frame options, frames in flight, queries, run_stages and the
refusals, against the CPU oracle on the substituted scene (tests/morph_parity.py)."""
import pytest

from tests import morph_parity as mp

MEM = mp.EmuMemory()


@pytest.mark.parametrize("n_words", mp.SIZES)
def test_emu_morph_sizes_and_alignment(emu_engine, n_words):
    mp.check_size(emu_engine, MEM, "emu_morph_size", n_words)


def test_emu_morph_odd_sizes(emu_engine):
    mp.check_odd_sizes(emu_engine, MEM, "emu_morph_odd")


def test_emu_morph_unaligned_scene_stream(emu_engine):
    mp.check_unaligned_scene_stream(emu_engine, MEM, "emu_morph_unaligned")


def test_emu_morph_arithmetic(emu_engine):
    mp.check_arithmetic(emu_engine, MEM, "emu_morph_arith")


def test_emu_morph_verbatim_bits(emu_engine):
    mp.check_verbatim_bits(emu_engine, MEM, "emu_morph_bits")


def test_emu_morph_front_fusion(emu_engine):
    mp.check_front_fusion(emu_engine, MEM, "emu_morph_front")


def test_emu_morph_indexed(emu_engine):
    mp.check_indexed(emu_engine, MEM, "emu_morph_indexed")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_emu_morph_strokes(emu_engine, stroke_kernel):
    mp.check_strokes(emu_engine, MEM, "emu_morph_strokes", stroke_kernel)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
@pytest.mark.parametrize("case", range(3))
def test_emu_morph_curves(emu_engine, case, which):
    mp.check_curves(emu_engine, MEM, "emu_morph_curves", which, case)


def test_emu_morph_tiger(emu_engine):
    mp.check_tiger(emu_engine, MEM, "emu_morph_tiger")


def test_emu_morph_view(emu_engine):
    mp.check_view(emu_engine, MEM, "emu_morph_view")


def test_emu_morph_culled(emu_engine):
    mp.check_culled(emu_engine, MEM, "emu_morph_culled")


def test_emu_morph_in_flight(emu_engine):
    mp.check_in_flight(emu_engine, MEM, "emu_morph_in_flight")


def test_emu_morph_run_stages_and_queries(emu_engine):
    mp.check_run_stages_and_queries(emu_engine, MEM, "emu_morph_stages")


def test_emu_morph_refusals(emu_engine):
    mp.check_refusals(emu_engine, MEM, "emu_morph_refusals")


def test_emu_morph_bindings(emu_engine):
    mp.check_bindings(emu_engine, MEM, "emu_morph_bindings")
