"""k_fine's batch planner, command windows and slice cuts at their edges on the MI355X: the checks of tests/fine_parity.py on the real
kernel.  Every case asserts through the planner model -- from the PTCL words and segments the engine wrote for the frame -- that the
edge it is named after was hit, then holds every AA mode's frame to the oracle through compare_frame."""
import pytest

from tests import fine_parity as fp

pytestmark = pytest.mark.gpu


# (a) fills a batch
@pytest.mark.parametrize("n", fp.REGULAR_COUNTS)
def test_gpu_fine_regular_list(gpu_engine, n):
    fp.check_regular(gpu_engine, n, f"gpu_fine_regular_{n}")


@pytest.mark.parametrize("depth", fp.NEST_DEPTHS)
def test_gpu_fine_nested_clips(gpu_engine, depth):
    fp.check_nested_clips(gpu_engine, depth, f"gpu_fine_nest_{depth}")


def test_gpu_fine_densest_window(gpu_engine):
    fp.check_densest_window(gpu_engine, "gpu_fine_densest")


@pytest.mark.parametrize("case", list(fp.MIXED_CASES))
def test_gpu_fine_mixed_prefix(gpu_engine, case):
    fp.check_mixed(gpu_engine, case, f"gpu_fine_mixed_{case}")


# (b) segments a batch
@pytest.mark.parametrize("delta", (-1, 0, 1))
@pytest.mark.parametrize("where", list(fp.SEGMENT_SPLITS))
def test_gpu_fine_segment_sum(gpu_engine, where, delta):
    fp.check_segment_sum(gpu_engine, where, delta, f"gpu_fine_segsum_{where}_{delta}")


@pytest.mark.parametrize("second", (False, True), ids=("first", "second"))
@pytest.mark.parametrize("n", fp.SINGLE_SEGMENTS)
def test_gpu_fine_single_fill_segments(gpu_engine, n, second):
    fp.check_single_fill_segments(gpu_engine, n, second, f"gpu_fine_single_{n}_{int(second)}")


# (c) records a batch
@pytest.mark.parametrize("delta", (-1, 0, 1))
@pytest.mark.parametrize("where", ("last", "middle", "first"))
def test_gpu_fine_record_cap(gpu_engine, where, delta):
    fp.check_record_cap(gpu_engine, where, delta, f"gpu_fine_cap_{where}_{delta}")


# (d) the simple-fill edge
@pytest.mark.parametrize("records", fp.SIMPLE_RECORDS)
def test_gpu_fine_simple_records(gpu_engine, records):
    fp.check_simple_records(gpu_engine, records, f"gpu_fine_simple_{records}")


@pytest.mark.parametrize("kind", ("even_odd", "long"))
def test_gpu_fine_simple_handoff(gpu_engine, kind):
    fp.check_simple_handoff(gpu_engine, kind, f"gpu_fine_handoff_{kind}")


# (e) windows
@pytest.mark.parametrize("off", fp.WINDOW_OFFSETS)
def test_gpu_fine_window_offset(gpu_engine, off):
    fp.check_window_offset(gpu_engine, off, f"gpu_fine_window_{off}")


@pytest.mark.parametrize("delta", fp.REACH_DELTAS)
def test_gpu_fine_prefetch_reach(gpu_engine, delta):
    fp.check_prefetch_reach(gpu_engine, delta, f"gpu_fine_reach_{delta}")


@pytest.mark.parametrize("case", list(fp.JUMP_CASES))
def test_gpu_fine_jump(gpu_engine, case):
    fp.check_jump(gpu_engine, case, f"gpu_fine_jump_{case}")


@pytest.mark.parametrize("first", (1, 9, 10))
def test_gpu_fine_jump_behind_batch(gpu_engine, first):
    fp.check_jump_behind_batch(gpu_engine, first, f"gpu_fine_jump_behind_{first}")


# (f) slices
@pytest.mark.parametrize("in_flight", (1, 2))
@pytest.mark.parametrize("n", fp.FORCED_FILLS)
def test_gpu_fine_slices_forced(gpu_engine, n, in_flight):
    fp.check_slices_forced(gpu_engine, n, in_flight, f"gpu_fine_forced_{n}")


@pytest.mark.parametrize("in_flight", (1, 2))
@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_gpu_fine_slices_natural(gpu_engine, delta, in_flight):
    fp.check_slices_natural(gpu_engine, delta, in_flight, f"gpu_fine_natural_{delta}")


@pytest.mark.parametrize("case", fp.SLICE_END_CASES)
def test_gpu_fine_slice_end(gpu_engine, case):
    fp.check_slice_end(gpu_engine, case, f"gpu_fine_slice_end_{case}")


@pytest.mark.parametrize("in_flight", (1, 2))
def test_gpu_fine_slices_mixed_tiles(gpu_engine, in_flight):
    fp.check_slices_mixed_tiles(gpu_engine, in_flight, "gpu_fine_slices_mixed")


# (g) dispatch order
@pytest.mark.parametrize("which", ("bucket_1", "last_bucket", "heavy"))
def test_gpu_fine_dispatch(gpu_engine, which):
    fp.check_dispatch(gpu_engine, which, f"gpu_fine_dispatch_{which}")


# (h) winding at the byte's edge
@pytest.mark.parametrize("reverse", (False, True), ids=("cw", "ccw"))
@pytest.mark.parametrize("turns", fp.WINDINGS)
@pytest.mark.parametrize("kind", fp.WINDING_KINDS)
def test_gpu_fine_winding(gpu_engine, kind, turns, reverse):
    fp.check_winding(gpu_engine, turns, kind, reverse, f"gpu_fine_winding_{kind}_{turns}_{int(reverse)}")


# (i) area AA
@pytest.mark.parametrize("n", fp.AREA_SEGMENTS)
def test_gpu_fine_area_segments(gpu_engine, n):
    fp.check_area_segments(gpu_engine, n, f"gpu_fine_area_{n}")


@pytest.mark.parametrize("off", fp.AREA_LOOKAHEAD)
def test_gpu_fine_area_lookahead(gpu_engine, off):
    fp.check_area_lookahead(gpu_engine, off, f"gpu_fine_area_ahead_{off}")
