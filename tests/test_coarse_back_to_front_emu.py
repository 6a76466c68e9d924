"""k_coarse's back-to-front form on the SIMT-emulated build of the kernel sources, against the CPU oracle's lists from each tile's
last opaque full cover onwards (tests/coarse_back_to_front_parity.py): covers at the batch boundaries, the jump chain of a list
that is never covered, the covered mask, the early exit, what must not cull, the scenes that keep the forward form and a PTCL
pool that is one word short."""
import pytest

from tests import coarse_back_to_front_parity as bp


@pytest.mark.parametrize("n_above", [0, 10])
@pytest.mark.parametrize("which", ["nb-1", "nb", "nb+1", "2nb+1"])
def test_emu_b2f_cover_at_batch_boundaries(emu_engine, which, n_above):
    bp.check_cover_boundaries(emu_engine, "emu_b2f_cover", which, n_above)


@pytest.mark.parametrize("first", [True, False])
def test_emu_b2f_cover_first_and_last_of_its_batch(emu_engine, first):
    bp.check_cover_slot(emu_engine, "emu_b2f_slot", first)


@pytest.mark.parametrize("tail", [5, 40])
def test_emu_b2f_uncovered_list_over_three_batches(emu_engine, tail):
    bp.check_uncovered_three_batches(emu_engine, "emu_b2f_chain", tail)


def test_emu_b2f_covered_and_uncovered_tile_of_one_quadrant(emu_engine):
    bp.check_covered_and_uncovered(emu_engine, "emu_b2f_mask")


def test_emu_b2f_all_tiles_covered_early(emu_engine):
    bp.check_all_covered(emu_engine, "emu_b2f_exit")


def test_emu_b2f_must_not_cull(emu_engine):
    bp.check_must_not_cull(emu_engine, "emu_b2f_keep")


def test_emu_b2f_clip_pair_keeps_forward_form(emu_engine):
    bp.check_clip_pair(emu_engine, "emu_b2f_clip")


def test_emu_b2f_no_opaque_fill_keeps_forward_form(emu_engine):
    bp.check_no_opaque(emu_engine, "emu_b2f_none")


def test_emu_b2f_ptcl_pool_one_region_short(emu_engine):
    import vello_amd

    bp.check_ptcl_pool_short(lambda caps: vello_amd.Engine(capacities=caps) if caps else vello_amd.Engine(), "emu_b2f_pool")


def test_emu_b2f_in_flight_and_front_ends(emu_engine):
    bp.check_in_flight(emu_engine, "emu_b2f_inflight3", 3)
    bp.check_front_ends(emu_engine, "emu_b2f_front")


def test_emu_b2f_counter_random_scene(emu_engine):
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    s, w, h = bp.random_cover_scene(3000, 256)
    packed, layout = s.resolve()
    emu_engine.set_auto_grow(True)
    try:
        bp.check_counter_large(emu_engine, packed, layout, w, h, AaConfig.Msaa16, "emu_b2f_random3k", Oracle(capacity_scale=8))
    finally:
        emu_engine.set_auto_grow(False)
