"""The unitigs by list ranking on the CPU: the host twin of pg_kindex_unitigs_ranked (csrc/kunitig_rank_host.cpp, which runs the rounds of
csrc/krank.hpp that the kernels run, one after the other) on a device = -1 index against the independent model (tests/kunitig_model.py)
at its default guard and against what each construction dictates (tests/kunitig_ranked_cases.py), and under
-fsanitize=address,undefined in a stand-alone program.  tests/test_gpu_kunitig_ranked.py runs the same through the kernels.  All
comparisons are of integers and exact."""

import pytest

import kunitig_ranked_cases as R
from host_program import build_and_run


@pytest.mark.parametrize("flavour", R.FLAVOURS, ids=R.flavour_id)
def test_existing_designs_with_nothing_cut(flavour):
    """Every design of kunitig_cases.cases(): the model's unitigs and the design's; "cut" returns the whole genome once with cut == 0 and
    the ring of "circular-too-long" is emitted."""
    R.check_designs(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", R.FLAVOURS, ids=R.flavour_id)
def test_ladder_of_chain_lengths(flavour):
    """Chains of 1 .. 257 k-mers, every power of two and its neighbours, in one index, and from reads reverse complemented: the closed
    form and the model."""
    R.check_ladder(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("n", R.ALONE)
@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_chain_alone_in_its_index(flavour, n):
    """keys == n: the rounds launched, ceil(log2(n + 1)), are the rounds needed."""
    R.check_alone(flavour[0], flavour[1], -1, n)


@pytest.mark.parametrize("flavour", R.FLAVOURS, ids=R.flavour_id)
def test_rings_beside_a_chain(flavour):
    R.check_rings(flavour[0], flavour[1], -1, R.rings_beside(flavour[0]), chain=True)


@pytest.mark.parametrize("n", R.RINGS_ALONE)
@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_ring_alone_in_its_index(flavour, n):
    R.check_rings(flavour[0], flavour[1], -1, (n,), chain=False)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_two_rings_and_isolated_kmers(flavour):
    """The start list: 128 chain starts, the rings' two behind them."""
    R.check_rings(flavour[0], flavour[1], -1, (flavour[0] + 2, 300), chain=False, lone=64)


def test_isolated_kmers_fill_the_start_list():
    """32 769 isolated 31-mers: the start list at its capacity 2 * keys, 257 scan blocks, and no round with anything to do."""
    R.check_isolated(-1)


def test_one_chain_of_65537_kmers():
    R.check_fast_records()
    R.check_long_chain(-1)


@pytest.mark.parametrize("flavour", [(13, False), (31, False), (65, True)], ids=R.flavour_id)
def test_random_counter_words(flavour):
    R.check_fuzz(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", R.FLAVOURS, ids=R.flavour_id)
def test_noisy_reads_of_a_genome_with_a_repeat(flavour):
    R.check_noisy(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_capacities_and_null_outputs(flavour):
    R.check_capacities(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_refusals(flavour):
    R.check_refusals(flavour[0], flavour[1], -1, (-1, -1))


@pytest.mark.parametrize("flavour", [(31, False), (127, True)], ids=R.flavour_id)
def test_api_engines_and_round_trip(flavour):
    R.check_api(flavour[0], flavour[1], -1)


def test_walk_rank_edit_round_rank_on_one_index():
    R.check_shared_scratch(-1)


# ---- the host twin under the sanitizers, in a program of its own ----
def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/kunitig_ranked_asan.cpp: both flavours, a chain, a ring and isolated k-mers in one index, heap outputs at exactly the counted
    sizes -- compiled with the host twin's sources and -fsanitize=address,undefined, and run.  Nothing loaded into Python is sanitised."""
    build_and_run(tmp_path, "kunitig_ranked_asan", ["kindex_host.cpp", "kunitig_rank_host.cpp"], ["kunitig ranked host twin: ok"])
