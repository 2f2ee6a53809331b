"""The unitigs on the CPU: the host twin (pg_kindex_unitigs on a device = -1 index: csrc/kunitig_host.cpp, the rule the kernels share in
csrc/kunitig.hpp) against the independent model (tests/kunitig_model.py) on the designed cases of tests/kunitig_cases.py -- each also
against the unitigs its construction dictates --, on tables of random counter words, on a noisy read set, at the capacities' edges, every
refusal, the api's methods with the round trip into the query and the walk, and under -fsanitize=address,undefined in a stand-alone
program.  tests/test_gpu_kunitig.py runs the same through the kernels.  All comparisons are of integers and exact."""

import pytest

import kunitig_cases as G
from host_program import build_and_run


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_host_twin_matches_model_and_design(flavour):
    """Every designed case: a linear genome and its reads reverse complemented; a shared prefix (BRANCH_OUT, BRANCH_IN); a branch of one
    read beside one of five at min_arc 1 and 2; one weak k-mer in the middle by coverage and by the deleted bit; a ring, alone, beside
    a chain, longer than max_kmers and exactly that long; a hairpin; a homopolymer; an isolated k-mer; texts that end 31, 32, 33, 64
    and 65 bases behind a word edge; max_kmers below and at a chain's length; counters at 63; an empty index; start lists of 129 and
    513 entries -- the model's unitigs, the design's, the layout word for word, count mode's totals, and every solid k-mer in exactly
    one unitig."""
    G.check_flavour(flavour[0], flavour[1], device=-1)


@pytest.mark.parametrize("flavour", [(13, False), (31, False), (65, True)], ids=G.flavour_id)
def test_random_counter_words(flavour):
    G.check_fuzz("n513", flavour[0], flavour[1], -1, [(1, 1), (100, 50), (200, 20)])
    G.check_fuzz("colliding", flavour[0], flavour[1], -1, [(100, 50)])


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_noisy_reads_of_a_genome_with_a_repeat(flavour):
    G.check_noisy(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=G.flavour_id)
def test_capacities_and_null_outputs(flavour):
    G.check_capacities(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], -1, (-1, -1))


@pytest.mark.parametrize("flavour", [(31, False), (127, True)], ids=G.flavour_id)
def test_api_and_round_trip(flavour):
    G.check_api(flavour[0], flavour[1], -1)


def test_isolated_kmers_fill_the_start_list():
    """32 769 isolated solid 31-mers (distinct random keys, every arc counter zero): 65 538 starts, which is the start list's capacity
    2 * keys exactly -- 257 blocks of 256, one more than a round of the device's scan over the blocks' sums.  The count call and the
    full call give 32 769 unitigs of K bases, both reasons DEAD_END, no ring, nothing cut: the model's, as sorted lists."""
    G.check_isolated(-1)


# ---- the host twin under the sanitizers, in a program of its own ----
def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/kunitig_asan.cpp: both flavours, a linear genome, a ring and isolated k-mers in one index, the output buffers on the heap at
    exactly the sizes the count call states -- compiled with the host twin's sources and -fsanitize=address,undefined, and run.  Nothing
    loaded into Python is sanitised."""
    build_and_run(tmp_path, "kunitig_asan", ["kindex_host.cpp", "kunitig_host.cpp"], ["kunitig host twin: ok"])
