"""The unitigs on the GPU: the kunitig kernels (csrc/kindex_kernels.hip, csrc/kunitig.hpp) against the independent model
(tests/kunitig_model.py) and, as sorted lists, against the host twin on every case of tests/kunitig_cases.py -- start lists of 129 and 513
entries in a table of more slots than a workgroup has lanes among them --, two compactions queued back to back on one stream, and
KmerCounter -> index() -> unitigs() on the simulated read set of the corrector's tests.  All comparisons are of integers and exact; no
test asserts a time or a rate."""
import numpy as np
import pytest

import kcorrect_cases as C
import kindex_model as M
import kunitig_cases as G
import kunitig_model as U
from soapdenovo2_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every test makes and destroys indexes, so the module pins the device arena (tests/test_gpu_kindex_sharded.py)."""
    with api.arena_pinned(0):
        yield


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_device_matches_model_design_and_host_twin(flavour):
    G.check_flavour(flavour[0], flavour[1], device=0, twin=-1)


@pytest.mark.parametrize("flavour", [(13, False), (31, False), (65, True)], ids=G.flavour_id)
def test_random_counter_words(flavour):
    G.check_fuzz("n513", flavour[0], flavour[1], 0, [(1, 1), (100, 50), (200, 20)])
    G.check_fuzz("colliding", flavour[0], flavour[1], 0, [(100, 50)])


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_noisy_reads_of_a_genome_with_a_repeat(flavour):
    G.check_noisy(flavour[0], flavour[1], 0, twin=-1)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=G.flavour_id)
def test_capacities_and_null_outputs(flavour):
    G.check_capacities(flavour[0], flavour[1], 0)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], 0, (0, 0))


@pytest.mark.parametrize("flavour", [(31, False), (127, True)], ids=G.flavour_id)
def test_api_and_round_trip(flavour):
    G.check_api(flavour[0], flavour[1], 0)


def test_isolated_kmers_fill_the_start_list():
    """32 769 isolated solid 31-mers: 65 538 starts, the start list's capacity 2 * keys exactly, in 257 blocks of 256 -- the 257th is
    scanned in the second round of kunitig_scan_sums_kernel, with the first round's carry.  The count call and the full call against
    the closed form, the model and the host twin (tests/kunitig_cases.py: check_isolated)."""
    G.check_isolated(0, twin=-1)


def test_two_compactions_back_to_back_on_one_stream():
    """Two full calls with different thresholds queued one after the other with no host wait in between -- the second reuses the index's
    scratch behind the first's end --, their outputs read afterwards: each is its own model's."""
    import torch
    K = 31
    P, SA, SB = G.forked(K)
    records = G.records_of(*G.count([(G.tile(np.concatenate([P, SA]), K), 5), ([np.concatenate([P, SB])[len(P) - K - 3:len(P) + K + 3]], 1)], K), 2)
    w = G.Compactor(records, K, False, 0)
    try:
        params = [(1, 1), (2, 2)]
        sizes = [w.count(a, b, G.MAXK) for a, b in params]
        assert [s[0] for s in sizes] == [3, 1]
        outs = [w.outputs(s[0], s[1]) for s in sizes]
        torch.cuda.synchronize()
        for (a, b), s, o in zip(params, sizes, outs):
            assert w.call(a, b, G.MAXK, s[0], s[1], *o) == 0
        for (a, b), s, o in zip(params, sizes, outs):
            packed, word_off, _, report, totals = (w.down(x) for x in o)
            assert [int(v) for v in totals] == s
            f = api.unitig_fields(report)
            got = sorted((tuple(int(x) for x in api.unpack_seq(packed[int(word_off[u]):], int(f["len"][u]))), int(f["left_code"][u]),
                          int(f["right_code"][u]), int(f["coverage_sum"][u])) for u in range(s[0]))
            assert got == sorted(U.unitigs(w.model, a, b)[0])
    finally:
        w.close()


def test_counter_to_index_to_unitigs():
    """KmerCounter counts the simulated reads (a circular genome of 3 000 bases, 900 reads of 100 bases with substitutions, K = 31) ->
    finalize -> index() -> unitigs() at min_cov 3 and min_arc 2: the model's unitigs over the counter's own records, the host twin's,
    every solid k-mer in exactly one of them, and the batch back through query_ragged."""
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
    seqs, f, totals = api.unitig_seqs(ix, C.SIM_MIN_COV, 2)
    u = ix.unitigs(C.SIM_MIN_COV, 2)
    cnt = ix.query_ragged(u.packed, u.word_off, u.kmer_base, int(u.totals[0]), int(u.totals[3])).cpu().numpy().view(np.uint64)
    ix.close()
    got = sorted((tuple(int(x) for x in s), int(l), int(r), int(c)) for s, l, r, c in zip(seqs, f["left_code"], f["right_code"], f["coverage_sum"]))
    want, n_cut = U.unitigs(model, C.SIM_MIN_COV, 2)
    assert got == sorted(want) and n_cut == 0 and totals["cut"] == 0
    solid = U.solid_keys(model, C.SIM_MIN_COV)
    assert totals["solid"] == totals["covered"] == len(solid) == cnt.size
    assert sorted(k for t, _, _, _ in got for k in U.kmers_of(t, K)) == solid
    assert (((cnt >> np.uint64(24)) & np.uint64(0xff)) >= C.SIM_MIN_COV).all()
    host = api.KmerIndex.from_records(records, K, False, -1)
    h_seqs, h_f, h_totals = api.unitig_seqs(host, C.SIM_MIN_COV, 2)
    host.close()
    assert sorted(tuple(int(x) for x in s) for s in h_seqs) == [t for t, _, _, _ in got] and h_totals == totals
    print("unitigs: %d of %d solid k-mers, longest %d bases, reasons %s" % (totals["unitigs"], totals["solid"], max(len(s) for s in seqs),
                                                                           {r: (f["left"] + f["right"]).count(r) for r in set(f["left"] + f["right"])}))
    assert totals["unitigs"] > 1 and max(len(s) for s in seqs) > 4 * K
