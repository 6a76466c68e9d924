"""The core pipeline's kernels at their partition boundaries on the MI355X: the checks of tests/shape_parity.py on the real kernels --
every tag, draw object, clip, line and tile row placed by the sizes of Engine.stage_constants(), every frame against the oracle
through compare_frame.  Each test is one family at one boundary; the families whose kernels differ with frames in flight (flatten's
own-launch stroke kernel, path_count's in-flight form, the grid caps of backdrop and path_tiling) run once more with two."""
import pytest

from tests import shape_parity as sp

pytestmark = pytest.mark.gpu


# (frames in flight, stroked-line kernel forced): with two frames in flight flatten's heavy list has a kernel of its own, and with
# the debug flag the stroked lines go to the stroked-line kernel -- beside the heavy list's workgroups, or as a launch of its own
TAG_VARIANTS = {"alone": (1, False), "in_flight": (2, False), "stroke_kernel": (1, True), "stroke_kernel_in_flight": (2, True)}


@pytest.mark.parametrize("variant", list(TAG_VARIANTS))
@pytest.mark.parametrize("boundary", list(sp.TAG_BOUNDARIES))
@pytest.mark.parametrize("probe", list(sp.PROBES))
def test_gpu_tags_at_boundary(gpu_engine, probe, boundary, variant):
    in_flight, stroke_kernel = TAG_VARIANTS[variant]
    sp.check_probe_slide(gpu_engine, probe, boundary, f"gpu_tags_{probe}_{boundary}_{variant}", in_flight=in_flight, stroke_kernel=stroke_kernel)


@pytest.mark.parametrize("in_flight", (1, 2))
@pytest.mark.parametrize("extra", (0, 1))
@pytest.mark.parametrize("blocks", (1, 4))
def test_gpu_unpadded_tag_stream(gpu_engine, blocks, extra, in_flight):
    sp.check_unpadded_stream(gpu_engine, blocks, extra, f"gpu_unpadded_{blocks}_{extra}", in_flight=in_flight)


@pytest.mark.parametrize("stacked", (False, True), ids=("grid", "stacked"))
@pytest.mark.parametrize("case", sp.DRAW_COUNT_CASES, ids=sp.case_id)
def test_gpu_draw_count(gpu_engine, case, stacked):
    sp.check_draw_count(gpu_engine, case, stacked, f"gpu_draws_{sp.case_id(case)}_{int(stacked)}")


@pytest.mark.parametrize("stacked", (False, True), ids=("grid", "stacked"))
@pytest.mark.parametrize("straddle", (False, True), ids=("adjacent", "straddle"))
def test_gpu_clip_across_draw_partition(gpu_engine, straddle, stacked):
    sp.check_clip_across_draw_partition(gpu_engine, straddle, stacked, f"gpu_draw_clip_{int(straddle)}_{int(stacked)}")


@pytest.mark.parametrize("stacked", (False, True), ids=("grid", "stacked"))
def test_gpu_front_max_draw_objects(gpu_engine, stacked):
    sp.check_front_max_draw_objects(gpu_engine, stacked, f"gpu_front_draws_{int(stacked)}")


def test_gpu_front_max_tags(gpu_engine):
    sp.check_front_max_tags(gpu_engine, "gpu_front_tags")


def test_gpu_front_tiny_segments(gpu_engine):
    sp.check_front_tiny_segments(gpu_engine, "gpu_front_tiny")


@pytest.mark.parametrize("case", range(5))
def test_gpu_clip_partition(gpu_engine, case):
    sp.check_clip_partition(gpu_engine, case, "gpu_clip_part")


@pytest.mark.parametrize("case", sp.LINE_COUNT_CASES, ids=sp.case_id)
def test_gpu_lines(gpu_engine, case):
    sp.check_lines(gpu_engine, case, f"gpu_lines_{sp.case_id(case)}")


@pytest.mark.parametrize("in_flight", (1, 2))
@pytest.mark.parametrize("case", sp.BACKDROP_CASES, ids=sp.case_id)
def test_gpu_backdrop(gpu_engine, case, in_flight):
    sp.check_backdrop(gpu_engine, case, f"gpu_backdrop_{sp.case_id(case)}", in_flight=in_flight)


def test_gpu_backdrop_cases_cover_every_group_remainder(gpu_engine):
    """(host only) the backdrop cases leave every n_draw_objects % 4, and every width has its three heights"""
    c = gpu_engine.stage_constants()
    assert {(before + 2) % 4 for _, _, before in sp.BACKDROP_CASES} == {0, 1, 2, 3}
    assert all(sp.backdrop_height(c, w, rel) >= 1 for w, rel, _ in sp.BACKDROP_CASES)


@pytest.mark.parametrize("case", sp.BIN_COUNT_CASES, ids=sp.case_id)
def test_gpu_bins(gpu_engine, case):
    sp.check_bins(gpu_engine, case, f"gpu_bins_{sp.case_id(case)}")
