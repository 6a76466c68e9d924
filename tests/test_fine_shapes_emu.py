"""k_fine's batch planner, command windows and slice cuts at their edges on the SIMT-emulated build of the kernel sources: the checks
of tests/fine_parity.py (shared with tests/test_fine_shapes_gpu.py).  Every case takes the emulator about a second; the families
with many offsets are thinned to their edges (the GPU file runs them all), the rest of each family is marked slow."""
import pytest

from tests import fine_parity as fp

slow = pytest.mark.slow


def _thin(values, keep):
    return [pytest.param(v, marks=() if v in keep else slow) for v in values]


# (a) fills a batch
@pytest.mark.parametrize("n", _thin(fp.REGULAR_COUNTS, (1, 11, 12, 23)))
def test_emu_fine_regular_list(emu_engine, n):
    fp.check_regular(emu_engine, n, f"emu_fine_regular_{n}")


@pytest.mark.parametrize("depth", _thin(fp.NEST_DEPTHS, (11, 14)))
def test_emu_fine_nested_clips(emu_engine, depth):
    fp.check_nested_clips(emu_engine, depth, f"emu_fine_nest_{depth}")


def test_emu_fine_densest_window(emu_engine):
    fp.check_densest_window(emu_engine, "emu_fine_densest")


@pytest.mark.parametrize("case", list(fp.MIXED_CASES))
def test_emu_fine_mixed_prefix(emu_engine, case):
    fp.check_mixed(emu_engine, case, f"emu_fine_mixed_{case}")


# (b) segments a batch
@pytest.mark.parametrize("delta", (-1, 0, 1))
@pytest.mark.parametrize("where", list(fp.SEGMENT_SPLITS))
def test_emu_fine_segment_sum(emu_engine, where, delta):
    fp.check_segment_sum(emu_engine, where, delta, f"emu_fine_segsum_{where}_{delta}")


@pytest.mark.parametrize("second", (False, True), ids=("first", "second"))
@pytest.mark.parametrize("n", _thin(fp.SINGLE_SEGMENTS, (64, 65, 129)))
def test_emu_fine_single_fill_segments(emu_engine, n, second):
    fp.check_single_fill_segments(emu_engine, n, second, f"emu_fine_single_{n}_{int(second)}")


# (c) records a batch
@pytest.mark.parametrize("delta", (-1, 0, 1))
@pytest.mark.parametrize("where", ("last", "middle", "first"))
def test_emu_fine_record_cap(emu_engine, where, delta):
    fp.check_record_cap(emu_engine, where, delta, f"emu_fine_cap_{where}_{delta}")


# (d) the simple-fill edge
@pytest.mark.parametrize("records", fp.SIMPLE_RECORDS)
def test_emu_fine_simple_records(emu_engine, records):
    fp.check_simple_records(emu_engine, records, f"emu_fine_simple_{records}")


@pytest.mark.parametrize("kind", ("even_odd", "long"))
def test_emu_fine_simple_handoff(emu_engine, kind):
    fp.check_simple_handoff(emu_engine, kind, f"emu_fine_handoff_{kind}")


# (e) windows
@pytest.mark.parametrize("off", fp.WINDOW_OFFSETS)
def test_emu_fine_window_offset(emu_engine, off):
    fp.check_window_offset(emu_engine, off, f"emu_fine_window_{off}")


@pytest.mark.parametrize("delta", fp.REACH_DELTAS)
def test_emu_fine_prefetch_reach(emu_engine, delta):
    fp.check_prefetch_reach(emu_engine, delta, f"emu_fine_reach_{delta}")


@pytest.mark.parametrize("case", list(fp.JUMP_CASES))
def test_emu_fine_jump(emu_engine, case):
    fp.check_jump(emu_engine, case, f"emu_fine_jump_{case}")


@pytest.mark.parametrize("first", _thin((1, 9, 10), (10,)))
def test_emu_fine_jump_behind_batch(emu_engine, first):
    fp.check_jump_behind_batch(emu_engine, first, f"emu_fine_jump_behind_{first}")


# (f) slices
@pytest.mark.parametrize("in_flight", _thin((1, 2), (1,)))
@pytest.mark.parametrize("n", fp.FORCED_FILLS)
def test_emu_fine_slices_forced(emu_engine, n, in_flight):
    fp.check_slices_forced(emu_engine, n, in_flight, f"emu_fine_forced_{n}")


@pytest.mark.parametrize("in_flight", (1, 2))
@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_emu_fine_slices_natural(emu_engine, delta, in_flight):
    fp.check_slices_natural(emu_engine, delta, in_flight, f"emu_fine_natural_{delta}")


@pytest.mark.parametrize("case", fp.SLICE_END_CASES)
def test_emu_fine_slice_end(emu_engine, case):
    fp.check_slice_end(emu_engine, case, f"emu_fine_slice_end_{case}")


@pytest.mark.parametrize("in_flight", (1, 2))
def test_emu_fine_slices_mixed_tiles(emu_engine, in_flight):
    fp.check_slices_mixed_tiles(emu_engine, in_flight, "emu_fine_slices_mixed")


# (g) dispatch order
@pytest.mark.parametrize("which", ("bucket_1", "last_bucket", "heavy"))
def test_emu_fine_dispatch(emu_engine, which):
    fp.check_dispatch(emu_engine, which, f"emu_fine_dispatch_{which}")


# (h) winding at the byte's edge
@pytest.mark.parametrize("reverse", (False, True), ids=("cw", "ccw"))
@pytest.mark.parametrize("turns", _thin(fp.WINDINGS, (127, 128)))
@pytest.mark.parametrize("kind", fp.WINDING_KINDS)
def test_emu_fine_winding(emu_engine, kind, turns, reverse):
    fp.check_winding(emu_engine, turns, kind, reverse, f"emu_fine_winding_{kind}_{turns}_{int(reverse)}")


# (i) area AA
@pytest.mark.parametrize("n", fp.AREA_SEGMENTS)
def test_emu_fine_area_segments(emu_engine, n):
    fp.check_area_segments(emu_engine, n, f"emu_fine_area_{n}")


@pytest.mark.parametrize("off", fp.AREA_LOOKAHEAD)
def test_emu_fine_area_lookahead(emu_engine, off):
    fp.check_area_lookahead(emu_engine, off, f"emu_fine_area_ahead_{off}")
