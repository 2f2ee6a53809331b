"""The trim on the GPU: ktrim_span_kernel, the scan's three kernels, ktrim_pack_kernel and, for an index cut over ranks (every rank on
GPU 0), ktrim_span_rows_kernel (csrc/kindex_kernels.hip, csrc/ktrim.hpp) against the independent model (tests/ktrim_model.py) on every
case and batch of tests/ktrim_cases.py, against the host twin on the simulated read set, two trims back to back on one stream, and the
round trip count -> index -> trim -> count again.  All comparisons are of integers and exact; no test asserts a time or a rate."""
import numpy as np
import pytest

import kcorrect_cases as C
import kindex_model as M
import ktrim_cases as E
from conftest import oracle_records
from soapdenovo2_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every test makes and destroys indexes, some of several tables each, so the module pins the device arena (tests/test_gpu_kindex_sharded.py)."""
    with api.arena_pinned(0):
        yield


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_device_matches_model(flavour):
    E.check_flavour(flavour[0], flavour[1], device=0)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=E.flavour_id)
def test_cut_over_ranks_gives_the_single_tables_words(flavour):
    """1, 2, 3 and 8 ranks on GPU 0: the spans come from the merged rows, scan and pack are the single table's."""
    E.check_ranks(flavour[0], flavour[1], lambda n: (0,) * n)


def test_batches_of_one_scan_round_and_one_block_more():
    """65 536 reads are exactly one round of ktrim_scan_sums_kernel (256 blocks of 256), 65 537 put one block into its second round,
    which takes the first round's carry: the kernels against the cumulative sums of the keep / drop bit vector and against the host
    twin (tests/ktrim_cases.py: check_rounds)."""
    E.check_rounds(0, twin=-1)


@pytest.fixture(scope="module")
def simulated_records(tmp_path_factory):
    return oracle_records(C.simulated()[0], C.SIM_K, 8, prefix=str(tmp_path_factory.mktemp("ktrim") / "o"))[0]


def test_device_matches_host_twin_on_the_simulated_set(simulated_records):
    """The oracle's records of the simulated reads, indexed on the device and by the host twin: the same output arrays, uniform and
    ragged -- and the model's (test_ktrim_host.py checks what those are worth)."""
    reads = list(C.simulated()[0])
    K = C.SIM_K
    host = E.Trimmer(K, False, -1, records=simulated_records)
    dev = E.Trimmer(K, False, 0, records=simulated_records, model=host.model)
    try:
        for uniform in (True, False):
            h = host.run(reads, K + 1, uniform=uniform, min_cov=C.SIM_MIN_COV)
            d = dev.run(reads, K + 1, uniform=uniform, min_cov=C.SIM_MIN_COV)
            assert all(a.shape == b.shape and (a == b).all() for a, b in zip(h, d))
            dev.check(reads, "simulated, uniform=%s" % uniform, min_len=K + 1, uniform=uniform, min_cov=C.SIM_MIN_COV)
            assert 850 < int(d[5][0]) <= len(reads) and int(d[5][3]) > 0
    finally:
        host.close()
        dev.close()


def test_two_trims_back_to_back_on_one_stream():
    """Two batches trimmed one after the other with no host wait in between (the second is the smaller one: the index's scratch does not
    grow), their outputs read afterwards: each is its own model's."""
    import torch
    K = 31
    t = E.Trimmer(K, False, 0)
    try:
        L = C.read_len(K)
        first, second = E.batch_of(K, 257, 21), E.batch_of(K, 65, 22)
        a_words, b_words = E.pack(first, K, 2, True)[0], E.pack(second, K, 2, True)[0]
        d_a, d_b = t.up(a_words), t.up(b_words)
        torch.cuda.synchronize()
        got_a = t.ix.trim_uniform(d_a, len(first), L, E.MIN_COV, E.min_len_of(K))
        got_b = t.ix.trim_uniform(d_b, len(second), L, E.MIN_COV, E.min_len_of(K))
        for got, reads in ((got_a, first), (got_b, second)):
            w = E.want(t.model, reads, E.min_len_of(K))
            spans, packed, word_off, kmer_base, src, totals = [t.down(o) for o in got]
            n_kept, n_words = int(w.totals[0]), int(w.totals[1])
            assert (spans == w.spans).all() and (totals == w.totals).all() and (src[:n_kept] == w.src).all()
            assert (word_off[:n_kept] == w.word_off).all() and (kmer_base[:n_kept + 1] == w.kmer_base).all()
            assert (packed[:n_words + 3] == w.words).all()
        times = t.ix.trim_times()
        assert set(times) == {"span", "scan", "pack", "total"}
    finally:
        t.close()


def test_round_trip_through_the_counter():
    """KmerCounter counts the simulated reads -> finalize -> index() -> trim_uniform -> a fresh KmerCounter counts the trimmed batch where
    it lies, as the ragged batch it is, with the kept reads and their k-mers from `totals`: as many distinct k-mers as the model's
    trimmed reads hold, and fewer than before."""
    import torch
    reads, _ = C.simulated()
    K, n, L = C.SIM_K, reads.shape[0], reads.shape[1]
    before = len(M.count_reads(reads, K)[0])
    packed = torch.from_numpy(api.pack_reads_uniform(reads).view(np.int64)).cuda()
    kc = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    assert kc.distinct() == before
    ix = kc.index()
    records = kc.export()
    kc.close()
    model = M.Model.from_records(records, K, 2)
    w = E.want(model, list(reads), K + 1, C.SIM_MIN_COV)
    after = E.check_recount(model, w.reads, C.SIM_MIN_COV)
    spans, out, word_off, kmer_base, src, totals = ix.trim_uniform(packed, n, L, C.SIM_MIN_COV)
    ix.close()
    totals = totals.cpu().numpy().view(np.uint64)
    assert (totals == w.totals).all()
    kc2 = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc2.count_ragged(out, word_off, kmer_base, int(totals[0]), int(totals[2]), 0)
    kc2.finalize(0)
    distinct = kc2.distinct()
    kc2.close()
    print("distinct k-mers before %d, after %d (model %d)" % (before, distinct, after))
    assert distinct == after and after < before
