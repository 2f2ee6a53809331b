"""Bubble popping on the GPU: the kbubble kernels (csrc/kindex_kernels.hip, csrc/kbubble.hpp) against the independent model
(tests/kbubble_model.py) on every design of tests/kbubble_cases.py, with the host twin popped in step: after every round the totals and
the word of every key of the original set are compared with the model's and, word for word, with the twin's -- a round's result is a
function of the index alone, so the two agree exactly.  Four junction counters cleared by two lanes, one word that loses a counter of each
half to two bubbles, two rounds queued back to back on one stream, start lists that cross wave and workgroup edges and tombstones inside
probe runs are among the designs.  Then KmerCounter -> index() -> simplify() -> unitigs() on the simulated read set of the corrector's
tests.  All comparisons are of integers and exact; no test asserts a time or a rate."""
import numpy as np
import pytest

import kbubble_cases as G
import kcorrect_cases as C
import kindex_model as M
import kunitig_model as U
from soapdenovo2_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every test makes and destroys indexes, so the module pins the device arena (tests/test_gpu_kindex_sharded.py)."""
    with api.arena_pinned(0):
        yield


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
@pytest.mark.parametrize("design", G.DESIGNS, ids=lambda d: d.__name__[6:])
def test_device_matches_model_design_and_host_twin(design, flavour):
    design(flavour[0], flavour[1], 0, twin=-1)


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], 0, (0, 0))


def test_counter_to_index_to_simplified_unitigs():
    """KmerCounter counts the simulated reads (a circular genome of 3 000 bases, 900 reads of 100 bases with substitutions, K = 31) ->
    finalize -> index() -> simplify() -> unitigs() at min_cov 1 and min_arc 1, where every error k-mer is solid and the graph is full
    of tips and bubbles: simplify's calls, their order and totals, and then the unitigs are the model's over the counter's own records,
    driven the same way; a bubble was popped, and the unitigs are fewer than after clip_tips alone."""
    import torch
    reads, _ = C.simulated()
    K, n, L = C.SIM_K, reads.shape[0], reads.shape[1]
    packed = torch.from_numpy(api.pack_reads_uniform(reads).view(np.int64)).cuda()
    kc = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    ix = kc.index()
    records = kc.export()
    kc.close()
    model = M.Model.from_records(records, K, 2)
    MIN_COV, MIN_ARC = 1, 1
    only_tips = api.KmerIndex.from_records(records, K, False, 0)
    only_tips.clip_tips(MIN_COV, MIN_ARC)
    clipped = int(only_tips.unitigs(MIN_COV, MIN_ARC).totals[0])
    only_tips.close()
    calls = G.plain(ix.simplify(MIN_COV, MIN_ARC))
    seqs, f, totals = api.unitig_seqs(ix, MIN_COV, MIN_ARC)
    ix.close()
    assert calls == G.model_simplify(model, MIN_COV, MIN_ARC, 2 * K, 2 * K)
    got = sorted((tuple(int(x) for x in s), int(l), int(r), int(c)) for s, l, r, c in zip(seqs, f["left_code"], f["right_code"], f["coverage_sum"]))
    assert got == sorted(U.unitigs(model, MIN_COV, MIN_ARC)[0])
    popped = sum(t[0] for name, t in calls if name == "bubbles")
    assert popped > 0 and totals["unitigs"] < clipped and totals["solid"] == totals["covered"] == calls[-1][1][2]
    print("simplify: %d calls %s, unitigs %d after the tips alone, %d simplified" % (len(calls), calls, clipped, totals["unitigs"]))
