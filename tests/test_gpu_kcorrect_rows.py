"""The corrector on an index cut over ranks, on the GPU: kcor_rows_begin_kernel, kcor_rows_plan_kernel and kcor_rows_decide_kernel
(csrc/kindex_kernels.hip, csrc/kcorrect_rows.hpp) around the sharded query, every rank on GPU 0, against the independent model
(tests/kcorrect_model.py), the host twin, the single device table's kcor_kernel and itself at other round capacities; then the hand-over
of scratch and events to the calls that follow, and the round trip count -> index over ranks -> correct -> trim -> count again.  All
comparisons are of integers and exact; no test asserts a time or a rate."""
import numpy as np
import pytest

import kcorrect_cases as E
import kcorrect_rows_cases as R
import kindex_model as M
import ktrim_cases as T
from conftest import oracle_records
from soapdenovo2_amd import api

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_device_matches_model_over_3_ranks(flavour):
    R.check_flavour(flavour[0], flavour[1], (0, 0, 0))


@pytest.mark.parametrize("flavour", R.RANK_FLAVOURS, ids=E.flavour_id)
def test_1_2_and_8_ranks(flavour):
    R.check_ranks(flavour[0], flavour[1], lambda n: (0,) * n)


@pytest.mark.parametrize("flavour", R.RANK_FLAVOURS, ids=E.flavour_id)
def test_round_capacity_changes_nothing_but_the_rounds(flavour):
    cor = R.RowsCorrector(flavour[0], flavour[1], (0, 0, 0))
    try:
        R.check_capacities(cor, (1, 5))
    finally:
        cor.close()


@pytest.fixture(scope="module")
def simulated_records(tmp_path_factory):
    return oracle_records(E.simulated()[0], E.SIM_K, 8, prefix=str(tmp_path_factory.mktemp("kcorrect_rows") / "o"))[0]


def _sim_params():
    return dict(min_cov=E.SIM_MIN_COV, max_fixes=api.CORRECT_MAX_FIXES, min_run=api.CORRECT_MIN_RUN)


def test_device_matches_host_twin_on_the_simulated_set(simulated_records):
    """The oracle's records of the simulated reads cut over 3 ranks of GPU 0 and over 3 ranks of the host twin: the same output words,
    reports and trials, uniform and ragged -- and the model's."""
    reads = list(E.simulated()[0])
    host = R.RowsCorrector(E.SIM_K, False, (-1, -1, -1), records=simulated_records)
    dev = R.RowsCorrector(E.SIM_K, False, (0, 0, 0), records=simulated_records, model=host.model)
    try:
        for uniform in (True, False):
            h_got, h_rep = host.run(reads, uniform=uniform, **_sim_params())
            d_got, d_rep = dev.check(reads, "simulated, uniform=%s" % uniform, uniform=uniform, **_sim_params())
            assert (h_got == d_got).all() and (h_rep == d_rep).all()
            h, d = host.ix.correct_rows_stats(), dev.ix.correct_rows_stats()
            assert h == d and d["trials"] == R.trials_of(d_rep) > 300
    finally:
        host.close()
        dev.close()


def test_in_place_two_buffers_and_the_single_table(simulated_records):
    import torch
    reads = list(E.simulated()[0])
    dev = R.RowsCorrector(E.SIM_K, False, (0, 0, 0), records=simulated_records)
    one = E.Corrector(E.SIM_K, False, 0, records=simulated_records, model=dev.model)
    try:
        words, _, _, L = E.pack(reads, E.SIM_K, 2, True)
        d_in = dev.up(words.copy())
        out, rep = dev.ix.correct_rows_uniform(d_in, len(reads), L, **_sim_params())
        assert out.data_ptr() != d_in.data_ptr() and (dev.down(d_in) == words).all()
        ref, ref_rep = one.ix.correct_uniform(d_in, len(reads), L, **_sim_params())
        assert torch.equal(out, ref) and torch.equal(rep, ref_rep)
        same, rep2 = dev.ix.correct_rows_uniform(d_in, len(reads), L, out=d_in, **_sim_params())
        assert same.data_ptr() == d_in.data_ptr()
        assert torch.equal(out, d_in) and torch.equal(rep, rep2) and not (dev.down(out) == words).all()
    finally:
        dev.close()
        one.close()


def test_calls_that_follow_a_correction():
    """Two corrections one after the other on one stream with nothing between the calls (the second batch is the smaller one: no
    scratch grows), read afterwards; then a correction, a trim and a query on the same cut index, each against its model: the scratch,
    the row buffers and the events are handed from one call to the next."""
    import torch
    K = 31
    cor = R.RowsCorrector(K, False, (0, 0, 0))
    try:
        L = E.read_len(K)
        pool = [c.read for c in E.cases(K) if len(c.read) == L]
        first, second = [pool[i % len(pool)] for i in range(257)], [pool[(3 * i + 1) % len(pool)] for i in range(65)]
        d_a, d_b = cor.up(E.pack(first, K, 2, True)[0]), cor.up(E.pack(second, K, 2, True)[0])
        torch.cuda.synchronize()
        got_a = cor.ix.correct_rows_uniform(d_a, len(first), L, **E.PARAMS)
        got_b = cor.ix.correct_rows_uniform(d_b, len(second), L, **E.PARAMS)
        for (got, rep), reads in ((got_a, first), (got_b, second)):
            w, w_rep = cor.want(reads, uniform=True, **E.PARAMS)
            assert (cor.down(got) == w).all() and (cor.down(rep) == w_rep).all()
        # correct, then trim what came out, then ask for the counts of what went in: nothing waits in between
        out, rep = cor.ix.correct_rows_uniform(d_a, len(first), L, **E.PARAMS)
        trimmed = cor.ix.trim_uniform(out, len(first), L, E.MIN_COV, T.min_len_of(K))
        counts = cor.ix.query_uniform(d_b, len(second), L)
        w, w_rep = cor.want(first, uniform=True, **E.PARAMS)
        assert (cor.down(out) == w).all() and (cor.down(rep) == w_rep).all()
        fixed = [E.model_correct(cor.model, r, E.PARAMS)[0] for r in first]
        t = T.want(cor.model, fixed, T.min_len_of(K))
        spans, packed, word_off, kmer_base, src, totals = [cor.down(o) for o in trimmed]
        n_kept, n_words = int(t.totals[0]), int(t.totals[1])
        assert (spans == t.spans).all() and (totals == t.totals).all() and (src[:n_kept] == t.src).all()
        assert (word_off[:n_kept] == t.word_off).all() and (kmer_base[:n_kept + 1] == t.kmer_base).all() and (packed[:n_words + 3] == t.words).all()
        want_counts = np.array([c for r in second for c in cor.model.query(r)], dtype=np.uint64)
        assert (cor.down(counts) == want_counts).all()
        # and once more on another stream than the calls before
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            again, again_rep = cor.ix.correct_rows_uniform(d_a, len(first), L, **E.PARAMS)
        side.synchronize()
        assert (cor.down(again) == w).all() and (cor.down(again_rep) == w_rep).all()
    finally:
        cor.close()


def test_round_trip_through_the_counter():
    """KmerCounter counts the simulated reads -> finalize -> index(devices=(0, 0)) -> correct_rows_uniform -> trim_uniform -> a fresh
    KmerCounter counts the trimmed batch where it lies: as many distinct k-mers as the model's corrected, then trimmed reads hold."""
    import torch
    reads, _ = E.simulated()
    K, n, L = E.SIM_K, reads.shape[0], reads.shape[1]
    before = len(M.count_reads(reads, K)[0])
    packed = torch.from_numpy(api.pack_reads_uniform(reads).view(np.int64)).cuda()
    kc = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    assert kc.distinct() == before
    ix = kc.index(devices=(0, 0))
    assert ix.sharded
    records = kc.export()
    kc.close()
    model = M.Model.from_records(records, K, 2)
    fixed, report = E.simulated_model_output(model)
    w = T.want(model, list(fixed), K + 1, E.SIM_MIN_COV)
    after = T.check_recount(model, w.reads, E.SIM_MIN_COV)
    out, rep = ix.correct_rows_uniform(packed, n, L, **_sim_params())
    assert (rep.cpu().numpy().view(np.uint64) == report).all()
    spans, kept, word_off, kmer_base, src, totals = ix.trim_uniform(out, n, L, E.SIM_MIN_COV)
    ix.close()
    totals = totals.cpu().numpy().view(np.uint64)
    assert (totals == w.totals).all()
    kc2 = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc2.count_ragged(kept, word_off, kmer_base, int(totals[0]), int(totals[2]), 0)
    kc2.finalize(0)
    distinct = kc2.distinct()
    kc2.close()
    print("distinct k-mers before %d, after correct and trim %d (model %d)" % (before, distinct, after))
    assert distinct == after and after < before
