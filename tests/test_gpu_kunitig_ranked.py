"""The unitigs by list ranking on the GPU: the krank kernels (csrc/kindex_kernels.hip, csrc/krank.hpp) against the independent model
(tests/kunitig_model.py) at its default guard, against what each construction dictates and, as sorted lists, against the host twin, on
the cases of tests/kunitig_ranked_cases.py; calls queued back to back on one stream; the walking engine, an edit round and the ranked
engine on one index's scratch; and KmerCounter -> index() -> simplify() -> unitigs(engine="rank") on the corrector's simulated read set,
whose circular genome is a ring of about 3 000 k-mers.  All comparisons are of integers and exact; no test asserts a time or a rate."""
import numpy as np
import pytest

import karc_cases as A
import kcorrect_cases as C
import kindex_model as M
import kunitig_cases as G
import kunitig_model as U
import kunitig_ranked_cases as R
from soapdenovo2_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every test makes and destroys indexes, so the module pins the device arena (tests/test_gpu_kunitig.py)."""
    with api.arena_pinned(0):
        yield


@pytest.mark.parametrize("flavour", R.FLAVOURS, ids=R.flavour_id)
def test_existing_designs_with_nothing_cut(flavour):
    R.check_designs(flavour[0], flavour[1], 0, twin=-1)


@pytest.mark.parametrize("flavour", R.FLAVOURS, ids=R.flavour_id)
def test_ladder_of_chain_lengths(flavour):
    R.check_ladder(flavour[0], flavour[1], 0, twin=-1)


@pytest.mark.parametrize("n", R.ALONE)
@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_chain_alone_in_its_index(flavour, n):
    R.check_alone(flavour[0], flavour[1], 0, n, twin=-1)


@pytest.mark.parametrize("flavour", R.FLAVOURS, ids=R.flavour_id)
def test_rings_beside_a_chain(flavour):
    R.check_rings(flavour[0], flavour[1], 0, R.rings_beside(flavour[0]), chain=True, twin=-1)


@pytest.mark.parametrize("n", R.RINGS_ALONE)
@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_ring_alone_in_its_index(flavour, n):
    R.check_rings(flavour[0], flavour[1], 0, (n,), chain=False, twin=-1)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_two_rings_and_isolated_kmers(flavour):
    R.check_rings(flavour[0], flavour[1], 0, (flavour[0] + 2, 300), chain=False, lone=64, twin=-1)


def test_isolated_kmers_fill_the_start_list():
    """32 769 isolated 31-mers: the start list at its capacity, 257 scan blocks, and every round ends at once."""
    R.check_isolated(0, twin=-1)


def test_one_chain_of_65537_kmers():
    """17 rounds, more nodes than one workgroup: the closed form."""
    R.check_fast_records()
    R.check_long_chain(0)


@pytest.mark.parametrize("flavour", [(13, False), (31, False), (65, True)], ids=R.flavour_id)
def test_random_counter_words(flavour):
    R.check_fuzz(flavour[0], flavour[1], 0)


@pytest.mark.parametrize("flavour", R.FLAVOURS, ids=R.flavour_id)
def test_noisy_reads_of_a_genome_with_a_repeat(flavour):
    R.check_noisy(flavour[0], flavour[1], 0, twin=-1)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_capacities_and_null_outputs(flavour):
    R.check_capacities(flavour[0], flavour[1], 0)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=R.flavour_id)
def test_refusals(flavour):
    R.check_refusals(flavour[0], flavour[1], 0, (0, 0))


@pytest.mark.parametrize("flavour", [(31, False), (127, True)], ids=R.flavour_id)
def test_api_engines_and_round_trip(flavour):
    R.check_api(flavour[0], flavour[1], 0)


def unitigs_of(w, outs, n):
    packed, word_off, _, report, _ = (w.down(x) for x in outs)
    f = api.unitig_fields(report)
    return sorted((tuple(int(x) for x in api.unpack_seq(packed[int(word_off[u]):], int(f["len"][u]))), int(f["left_code"][u]),
                   int(f["right_code"][u]), int(f["coverage_sum"][u])) for u in range(n))


def test_two_ranked_calls_back_to_back_on_one_stream():
    """Two full calls with different thresholds queued with no host wait in between -- the second reuses the index's scratch behind the
    first's end --, their outputs read afterwards: each is its own model's."""
    import torch
    K = 31
    P, SA, SB = G.forked(K)
    records = G.records_of(*G.count([(G.tile(np.concatenate([P, SA]), K), 5), ([np.concatenate([P, SB])[len(P) - K - 3:len(P) + K + 3]], 1)], K), 2)
    w = R.Compactor(records, K, False, 0)
    try:
        params = [(1, 1), (2, 2)]
        sizes = [w.count(a, b, G.MAXK) for a, b in params]
        assert [s[0] for s in sizes] == [3, 1]
        outs = [w.outputs(s[0], s[1]) for s in sizes]
        torch.cuda.synchronize()
        for (a, b), s, o in zip(params, sizes, outs):
            assert w.call(a, b, G.MAXK, s[0], s[1], *o) == 0
        for (a, b), s, o in zip(params, sizes, outs):
            assert [int(v) for v in w.down(o[4])] == s
            assert unitigs_of(w, o, s[0]) == sorted(U.unitigs(w.model, a, b)[0])
    finally:
        w.close()


def test_walk_rank_edit_round_rank_share_the_scratch():
    R.check_shared_scratch(0)


def test_counter_to_index_to_simplify_to_ranked_unitigs():
    """KmerCounter counts the corrector's simulated reads (a circular genome of 3 000 bases, K = 31) -> index() ->
    simplify(ops=api.SIMPLIFY_OPS) at 2 / 1 -> unitigs(engine="rank"): the model's unitigs over the edited index's records at the default
    guard, the walking engine's with the same totals, every solid k-mer in exactly one unitig, and the batch back through query_ragged."""
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
    try:
        calls = A.plain(ix.simplify(2, 1, ops=api.SIMPLIFY_OPS))
        listed = lambda out: (sorted((tuple(int(x) for x in s), int(l), int(r), int(c)) for s, l, r, c in
                                     zip(out[0], out[1]["left_code"], out[1]["right_code"], out[1]["coverage_sum"])), out[2])
        got, totals = listed(api.unitig_seqs(ix, 2, 1, engine="rank"))
        walked, w_totals = listed(api.unitig_seqs(ix, 2, 1, engine="walk"))
        u = ix.unitigs(2, 1, engine="rank")
        cnt = ix.query_ragged(u.packed, u.word_off, u.kmer_base, int(u.totals[0]), int(u.totals[3])).cpu().numpy().view(np.uint64)
    finally:
        ix.close()
    model = M.Model.from_records(records, K, 2)
    assert calls == A.model_simplify(model, api.SIMPLIFY_OPS, 2, 1, 2 * K, 2 * K), "the model was not edited as the index was"
    want, n_cut = U.unitigs(model, 2, 1)
    assert n_cut == 0 and got == sorted(want)
    assert got == walked and totals == w_totals and totals["cut"] == 0
    solid = U.solid_keys(model, 2)
    assert totals["solid"] == totals["covered"] == len(solid) == cnt.size
    assert sorted(k for t, _, _, _ in got for k in U.kmers_of(t, K)) == solid
    assert (((cnt >> np.uint64(24)) & np.uint64(0xff)) >= 2).all()
    print("ranked unitigs after simplify: %d, cyclic %d, longest %d bases" % (totals["unitigs"], totals["cyclic"], max(len(t) for t, _, _, _ in got)))
    assert max(len(t) for t, _, _, _ in got) > 1000
