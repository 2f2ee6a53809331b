"""Bubble popping on strongest paths on the CPU: the host twin (pg_kindex_pop_bulges on a device = -1 index: csrc/kedit_ops_host.cpp, the
rule the kernels share in csrc/kbulge.hpp) against the independent model (tests/kbulge_model.py) on the designs of
tests/kbulge_cases.py -- each also against what its construction dictates: the totals and the word of every key of the original set
after every round --, every refusal, KmerIndex.pop_bulges and KmerIndex.simplify(ops=...).  The stand-alone program under
-fsanitize=address,undefined is the arcs' and the bulges' in one (tests/kedit_ops_asan.cpp, built and run by tests/test_karc_host.py).
tests/test_gpu_kbulge.py runs the same through the kernels.  All comparisons are of integers and exact."""
import pytest

import kbulge_cases as G


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
@pytest.mark.parametrize("design", G.DESIGNS, ids=lambda d: d.__name__[6:])
def test_host_twin_matches_model_and_design(design, flavour):
    """A plain substitution bubble beside pop_bubbles on a second index; two errors less than K apart on different reads; fork ties of
    5 : 5 and 63 : 63, 2 : 1, and the strongest arc on the arm with the lower mean; three arms of one bubble; a bubble on an arm gone
    in one round; an arm of K - 1 k-mers at max_diff 0 and 1; two bulges at one k-mer; 257 and 513 arms on one path; records whose
    counters disagree at their two ends; noisy reads of a genome with a repeat to the fixed point; an empty index."""
    design(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], -1, (-1, -1))
