"""Bubble popping on the CPU: the host twin (pg_kindex_pop_bubbles on a device = -1 index: csrc/kedit_host.cpp, the rule the kernels
share in csrc/kbubble.hpp) against the independent model (tests/kbubble_model.py) on the designs of tests/kbubble_cases.py -- each also
against what its construction dictates: the totals and the word of every key of the original set after every round --, every refusal,
KmerIndex.pop_bubbles and KmerIndex.simplify.  The stand-alone program under -fsanitize=address,undefined is the tips' and the bubbles'
in one (tests/kedit_asan.cpp, built and run by tests/test_ktip_host.py).  tests/test_gpu_kbubble.py runs the same through the kernels.
All comparisons are of integers and exact."""
import pytest

import kbubble_cases as G


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
@pytest.mark.parametrize("design", G.DESIGNS, ids=lambda d: d.__name__[6:])
def test_host_twin_matches_model_and_design(design, flavour):
    """A 1-read copy of a 5-read path with another base, at max_len K - 1 and K, each junction canonical and not, the reads reverse
    complemented, and the popped index beside one built without the copy; arms read 1:1, 2:1 and 300:260 times; three arms of one
    bubble; arms of K and K - 1 k-mers whose means and sums order them differently, at max_diff 0 and 1; two bubbles at one k-mer; a
    bubble on an arm, by rounds, by two calls back to back and by pop_bubbles; a tip on an arm, by pop_bubbles and by simplify; two
    loops from one k-mer, a sibling with a fork inside, an arm longer than max_len, tips, an island, a ring and a hairpin, all kept;
    tombstones in the middle of probe runs; an empty index; 257 and 513 bubbles on one path; noisy reads of a genome with a repeat
    through simplify to the fixed point."""
    design(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], -1, (-1, -1))

