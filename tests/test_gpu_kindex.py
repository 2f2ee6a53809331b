"""The k-mer index on the GPU: the build kernel with the lane-per-sequence and the wavefront-per-sequence query kernels
(csrc/kindex_kernels.hip) against the independent model (tests/kindex_model.py) on every case of tests/test_kindex_host.py -- but the
duplicate key, which stays on the host twin: no test here is built around making a kernel fail -- and on the wave kernel's own edges.
All comparisons are of integers and exact; no test asserts a time or a rate."""
import numpy as np
import pytest

import kindex_cases as E
import kindex_model as M
from soapdenovo2_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", E.TABLES)
@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_device_matches_model(flavour, name):
    E.check_table(name, flavour[0], flavour[1], device=0, waves=(False, True))


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_wave_kernel_edges(flavour):
    """Sequences of 1, 63, 64, 65, 128, 129 and 4 097 k-mers, each also with its last k-mer alone absent (the last lane's stretch), in
    batches of 0 to 5 sequences (workgroups of four waves with empty ones) and with a k-mer-less sequence between two real ones of
    one workgroup; the lane kernel on the same batches gives the same words, and a second run too."""
    K, mer127 = flavour
    ix = E.Index(E.table("genome", K, mer127)[0], K, mer127, 0)
    seqs, tags = E.wave_sequences(K)
    cnt, summ = ix.check_ragged(seqs, wave=True, what="wave")
    for t, s, row in zip(tags, seqs, summ):
        nk = len(s) - K + 1
        assert list(row[[0, 3]]) == ([nk - 1, nk - 1] if t.endswith("last-absent") else [nk, nk]), t
    lane_cnt, lane_summ = ix.check_ragged(seqs, wave=False, what="lane")
    again_cnt, again_summ = ix.check_ragged(seqs, wave=True, what="wave again")
    assert (lane_cnt == cnt).all() and (lane_summ == summ).all() and (again_cnt == cnt).all() and (again_summ == summ).all()
    short = seqs[:8]                                           # (up to 65 k-mers: the batches' shapes matter here, not their lengths)
    for n in range(6):
        ix.check_ragged(short[:n], wave=True, what="wave, %d sequences" % n)
    none = np.zeros(K - 1, dtype=np.uint8)
    ix.check_ragged([short[2], none, short[4], short[5], none, short[6]], wave=True, what="wave, k-mer-less between")
    ix.check_ragged([short[2], none, short[4], short[5], none, short[6]], wave=False, what="lane, k-mer-less between")
    ix.close()


@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=E.flavour_id)
def test_counts_or_summary_alone(flavour, wave):
    K, mer127 = flavour
    ix = E.Index(E.table("n513", K, mer127)[0], K, mer127, 0)
    seqs = E.sequences(K)[0] + E.wave_sequences(K)[0][:6]
    cnt, summ, _ = ix.ragged(seqs, wave)
    only_cnt, none, _ = ix.ragged(seqs, wave, summary=False)
    none2, only_summ, _ = ix.ragged(seqs, wave, counts=False)
    assert none is None and none2 is None and (only_cnt == cnt).all() and (only_summ == summ).all()
    ix.close()


@pytest.mark.parametrize("flavour", [(31, False), (127, True)], ids=E.flavour_id)
def test_table_is_a_function_of_the_records(flavour):
    """The records as they lie, reversed and shuffled three times: the slot image may differ, the answers may not."""
    K, mer127 = flavour
    records = E.table("colliding", K, mer127)[0]
    seqs = E.sequences(K)[0]
    rng = np.random.default_rng(3)
    orders = [np.arange(len(records)), np.arange(len(records))[::-1]] + [rng.permutation(len(records)) for _ in range(3)]
    want = None
    for o in orders:
        ix = E.Index(np.ascontiguousarray(records[o]), K, mer127, 0)
        got = ix.check_ragged(seqs, wave=False, what="order") + ix.check_ragged(seqs, wave=True, what="order, wave")
        ix.close()
        want = want or got
        assert all((a == b).all() for a, b in zip(got, want))


@pytest.fixture(scope="module", params=[(31, False), (65, True)], ids=E.flavour_id)
def counted(request):
    K, mer127 = request.param
    codes = synth.reads_codes(3000, 3000, 100, 0.01, 7)
    return (K, mer127, codes) + M.count_reads(codes, K)


@pytest.mark.parametrize("delow", [0, 1])
def test_round_trip_through_the_counter(counted, delow):
    """KmerCounter -> finalize -> index() -> query_uniform of the same device batch, with both kernels: what
    test_kindex_host.py::test_round_trip_through_the_oracle asks of the oracle's records, and conservation: with nothing saturated the
    checksum's coverage sum is the k-mer occurrences that went in, and with delow = 0 that many query positions have an answer."""
    import torch
    K, mer127, codes, occ, arcs = counted
    kc = api.KmerCounter(K, n_sets=8, mer127=mer127, log2_slots=18)
    packed = torch.from_numpy(api.pack_reads_uniform(codes).view(np.int64)).cuda()
    n_kmers = kc.count_uniform(packed, codes.shape[0], codes.shape[1], 0)
    kc.finalize(delow)
    digest = kc.checksum()
    ix = kc.index()
    info = ix.info()
    assert info["keys"] == kc.distinct() == len(occ) and info["slots"] == M.table_slots(len(occ)) and info["device"] == 0
    assert info["bytes"] == api.host_kindex_bytes(len(occ), mer127)
    kc.close()                                                 # (the index owns its table: the counter and its records may go)
    for wave in (False, True):
        cnt, summ = ix.query_uniform(packed, codes.shape[0], codes.shape[1], wave=wave, counts=True, summary=True)
        cnt, summ = cnt.cpu().numpy().view(np.uint64), summ.cpu().numpy().view(np.uint64)
        E.check_round_trip(codes, K, occ, M.filtered(arcs, delow), delow, cnt, summ)
        assert int(digest[7]) == 0 and int(digest[6]) == n_kmers
        if delow == 0:
            assert int((cnt != 0).sum()) == int(digest[6]) == int(summ[:, 0].sum())
    ix.close()


def test_index_needs_a_finalized_counter():
    kc = api.KmerCounter(31, n_sets=8, log2_slots=16)
    with pytest.raises(api.PgError, match=r"\(PG_ESTATE\)"):
        kc.index()
    kc.close()


def test_kmer_coverage_on_the_device():
    K = 31
    ix = E.Index(E.table("genome", K, False)[0], K, False, 0)
    seqs, _ = E.sequences(K)
    for wave in (False, True):
        cov = api.kmer_coverage(seqs, ix.ix, wave=wave)
        for s, c in zip(seqs, cov):
            assert list(c) == [M.coverage(a) for a in ix.model.query(s)]
    ix.close()
