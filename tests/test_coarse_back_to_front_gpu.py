"""k_coarse's back-to-front form on the MI355X: the cases of test_coarse_back_to_front_emu.py on the real kernel -- eight waves, the
ballots behind the covered mask, the LDS exchange of the batch tables, bump allocation against other workgroups -- with one and three
frames in flight, through the indexed and the unindexed front end, and bench.py's d2 scene."""
import pytest

from tests import coarse_back_to_front_parity as bp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_above", [0, 10])
@pytest.mark.parametrize("which", ["nb-1", "nb", "nb+1", "2nb+1"])
def test_gpu_b2f_cover_at_batch_boundaries(gpu_engine, which, n_above):
    bp.check_cover_boundaries(gpu_engine, "gpu_b2f_cover", which, n_above)


@pytest.mark.parametrize("first", [True, False])
def test_gpu_b2f_cover_first_and_last_of_its_batch(gpu_engine, first):
    bp.check_cover_slot(gpu_engine, "gpu_b2f_slot", first)


@pytest.mark.parametrize("tail", [5, 40])
def test_gpu_b2f_uncovered_list_over_three_batches(gpu_engine, tail):
    bp.check_uncovered_three_batches(gpu_engine, "gpu_b2f_chain", tail)


def test_gpu_b2f_covered_and_uncovered_tile_of_one_quadrant(gpu_engine):
    bp.check_covered_and_uncovered(gpu_engine, "gpu_b2f_mask")


def test_gpu_b2f_all_tiles_covered_early(gpu_engine):
    bp.check_all_covered(gpu_engine, "gpu_b2f_exit")


def test_gpu_b2f_must_not_cull(gpu_engine):
    bp.check_must_not_cull(gpu_engine, "gpu_b2f_keep")


def test_gpu_b2f_clip_pair_keeps_forward_form(gpu_engine):
    bp.check_clip_pair(gpu_engine, "gpu_b2f_clip")


def test_gpu_b2f_no_opaque_fill_keeps_forward_form(gpu_engine):
    bp.check_no_opaque(gpu_engine, "gpu_b2f_none")


def test_gpu_b2f_ptcl_pool_one_region_short(gpu_engine):
    import vello_amd

    bp.check_ptcl_pool_short(lambda caps: vello_amd.Engine(device=0, capacities=caps) if caps else vello_amd.Engine(device=0), "gpu_b2f_pool")


@pytest.mark.parametrize("n", [1, 3])
def test_gpu_b2f_frames_in_flight(gpu_engine, n):
    bp.check_in_flight(gpu_engine, f"gpu_b2f_inflight{n}", n)


def test_gpu_b2f_indexed_and_unindexed_front_end(gpu_engine):
    bp.check_front_ends(gpu_engine, "gpu_b2f_front")


def test_gpu_b2f_counter_random_scene(gpu_engine):
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    s, w, h = bp.random_cover_scene(30000, 512)
    packed, layout = s.resolve()
    gpu_engine.set_auto_grow(True)
    try:
        bp.check_counter_large(gpu_engine, packed, layout, w, h, AaConfig.Msaa16, "gpu_b2f_random30k", Oracle(capacity_scale=8))
    finally:
        gpu_engine.set_auto_grow(False)


def test_gpu_b2f_d2(gpu_engine):
    # bench.py's headline scene on its pools: what coarse leaves of it is what the oracle's lists hold from each tile's last cover onwards
    import bench
    import vello_amd
    import workloads
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    packed, layout = workloads.paris_like_scene_d2().resolve()
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    bp.check_counter_large(eng, packed, layout, 1600, 1600, AaConfig.Msaa16, "gpu_b2f_d2", Oracle(capacity_scale=8))
