"""The core pipeline's kernels at their partition boundaries on the SIMT-emulated build of the kernel sources: the checks of
tests/shape_parity.py (shared with tests/test_stage_shapes_gpu.py).  Unmarked is a thinned set -- per probe the offsets that put its
first, a middle and its last tag on the edge, the draw counts around one partition and one coarse batch, the backdrop rectangles of
exactly four blocks of rows; the whole slides, the second partition edge, the frames-in-flight runs, the 255 to 257 bins and the
FRONT_MAX_* pairs take the emulator more than about five seconds a case and are marked slow."""
import pytest

from tests import shape_parity as sp

slow = pytest.mark.slow


def _slow_if(cond, *values):
    return pytest.param(*values, marks=slow) if cond else pytest.param(*values)


@pytest.mark.parametrize("which", ("first", "middle", "last"))
@pytest.mark.parametrize("boundary", [_slow_if(b == "pathtag_part_2", b) for b in sp.TAG_BOUNDARIES])
@pytest.mark.parametrize("probe", list(sp.PROBES))
def test_emu_tags_at_boundary(emu_engine, probe, boundary, which):
    """first: the probe's first tag is the first tag above the boundary; last: its last tag is the last tag below it"""
    n = sp.probe_length(probe)
    below = {"first": 0, "middle": n // 2, "last": n}[which]
    sp.check_tags_at_boundary(emu_engine, probe, boundary, below, f"emu_tags_{probe}_{boundary}_{below}")


@slow
@pytest.mark.parametrize("boundary", list(sp.TAG_BOUNDARIES))
@pytest.mark.parametrize("probe", list(sp.PROBES))
def test_emu_tags_slide(emu_engine, probe, boundary):
    sp.check_probe_slide(emu_engine, probe, boundary, f"emu_slide_{probe}_{boundary}")


@slow
@pytest.mark.parametrize("in_flight", (1, 2))
@pytest.mark.parametrize("probe", list(sp.PROBES))
def test_emu_tags_slide_stroke_kernel(emu_engine, probe, in_flight):
    """(the stroked-line kernel forced: beside the heavy list's workgroups, and with two frames in flight as a launch of its own)"""
    sp.check_probe_slide(emu_engine, probe, "flatten_block", f"emu_slide_sk{in_flight}_{probe}", in_flight=in_flight, stroke_kernel=True)


@pytest.mark.parametrize("in_flight", (1, pytest.param(2, marks=slow)))
@pytest.mark.parametrize("extra", (0, 1))
@pytest.mark.parametrize("blocks", (1, 4))
def test_emu_unpadded_tag_stream(emu_engine, blocks, extra, in_flight):
    sp.check_unpadded_stream(emu_engine, blocks, extra, f"emu_unpadded_{blocks}_{extra}", in_flight=in_flight)


def _draw_case(case):
    key, mult, _ = case
    quick = key is None or (key, mult) in (("draw_part", 1), ("coarse_batch", 1))
    return pytest.param(case, marks=() if quick else slow, id=sp.case_id(case))


@pytest.mark.parametrize("stacked", (False, True), ids=("grid", "stacked"))
@pytest.mark.parametrize("case", [_draw_case(c) for c in sp.DRAW_COUNT_CASES])
def test_emu_draw_count(emu_engine, case, stacked):
    sp.check_draw_count(emu_engine, case, stacked, f"emu_draws_{sp.case_id(case)}_{int(stacked)}")


@pytest.mark.parametrize("stacked", (False, True), ids=("grid", "stacked"))
@pytest.mark.parametrize("straddle", (False, True), ids=("adjacent", "straddle"))
def test_emu_clip_across_draw_partition(emu_engine, straddle, stacked):
    sp.check_clip_across_draw_partition(emu_engine, straddle, stacked, f"emu_draw_clip_{int(straddle)}_{int(stacked)}")


@slow
@pytest.mark.parametrize("stacked", (False, True), ids=("grid", "stacked"))
def test_emu_front_max_draw_objects(emu_engine, stacked):
    sp.check_front_max_draw_objects(emu_engine, stacked, f"emu_front_draws_{int(stacked)}")


@slow
def test_emu_front_max_tags(emu_engine):
    sp.check_front_max_tags(emu_engine, "emu_front_tags")


def test_emu_front_tiny_segments(emu_engine):
    sp.check_front_tiny_segments(emu_engine, "emu_front_tiny")


@pytest.mark.parametrize("case", range(5))
def test_emu_clip_partition(emu_engine, case):
    sp.check_clip_partition(emu_engine, case, "emu_clip_part")


@pytest.mark.parametrize("case", sp.LINE_COUNT_CASES, ids=sp.case_id)
def test_emu_lines(emu_engine, case):
    sp.check_lines(emu_engine, case, f"emu_lines_{sp.case_id(case)}")


@pytest.mark.parametrize("in_flight", (1, pytest.param(2, marks=slow)))
@pytest.mark.parametrize("case", [pytest.param(c, marks=() if c[1] == 0 else slow, id=sp.case_id(c)) for c in sp.BACKDROP_CASES])
def test_emu_backdrop(emu_engine, case, in_flight):
    sp.check_backdrop(emu_engine, case, f"emu_backdrop_{sp.case_id(case)}", in_flight=in_flight)


def test_emu_backdrop_cases_cover_every_group_remainder(emu_engine):
    """(host only) the backdrop cases leave every n_draw_objects % 4, the unmarked ones among them"""
    assert {(before + 2) % 4 for _, _, before in sp.BACKDROP_CASES} == {0, 1, 2, 3}
    assert {(before + 2) % 4 for _, rel, before in sp.BACKDROP_CASES if rel == 0} == {0, 1, 2, 3}


@pytest.mark.parametrize("case", [pytest.param(c, marks=() if c[0] == "coarse_grid_bins" else slow, id=sp.case_id(c)) for c in sp.BIN_COUNT_CASES])
def test_emu_bins(emu_engine, case):
    sp.check_bins(emu_engine, case, f"emu_bins_{sp.case_id(case)}")


def test_emu_stage_constants_are_the_engine_s(emu_engine):
    """Every name of the seam answers, nothing beyond it does, and the sizes that are one fact keep their relation."""
    import vello_amd

    c = emu_engine.stage_constants()
    assert list(c) == list(vello_amd.Engine.STAGE_CONSTANTS) and all(v > 0 for v in c.values())
    assert emu_engine._lib.vello_hip_stage_constant(len(c)) == 0 and emu_engine._lib.vello_hip_stage_constant(-1) == 0
    assert c["pathtag_part_tags"] % c["flatten_block_tags"] == 0 and c["front_max_tags"] % c["flatten_block_tags"] == 0
    assert c["path_count_chunk_small"] < c["path_count_chunk_in_flight"] < c["path_count_chunk"]
