"""The read corrector on the CPU: the host twin (pg_kindex_correct on a device = -1 index: the per-read procedure the kernel shares,
csrc/kcorrect.hpp) against the independent model (tests/kcorrect_model.py) on the designed cases of tests/kcorrect_cases.py and on one
simulated read set counted by the oracle.  tests/test_gpu_kcorrect.py runs the same through kcor_kernel.  All comparisons are of
integers and exact."""
import numpy as np
import pytest

import kcorrect_cases as E
import kcorrect_model as C
import kindex_model as M
from conftest import oracle_records
from soapdenovo2_amd import api


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_host_twin_matches_model(flavour):
    """Every designed case does what its name says in the model, and the twin gives the model's words and reports: alone, in one
    ragged batch, with reads without k-mers between others, in batches of 1, 63, 64, 65 and 257, uniform and ragged, in place and not."""
    E.check_flavour(flavour[0], flavour[1], device=-1)


def test_argument_errors():
    K = 31
    cor = E.Corrector(K, False, -1)
    words, off, base, _ = E.pack([c.read for c in E.cases(K)[:6]], K, 2, False)
    out, rep = np.zeros_like(words), np.zeros(6, dtype=np.uint64)
    L = api.lib()

    def call(min_cov=3, max_fixes=3, min_run=5, n=6, packed_out=out.ctypes.data, report=rep.ctypes.data, n_words=len(words), ulen=0):
        return L.pg_kindex_correct(cor.ix.h, words.ctypes.data, off.ctypes.data, base.ctypes.data, n, ulen, n_words, min_cov, max_fixes, min_run,
                                   packed_out, report, None)

    einval = -1                                                 # PG_EINVAL (include/soapdenovo2_amd.h)
    assert call(min_cov=0) == einval and b"min_cov" in L.pg_last_error()
    assert call(min_run=0) == einval and call(max_fixes=256) == einval and call(packed_out=None) == einval
    assert call(ulen=101, n_words=6 * 4 + 2) == einval          # (a uniform batch needs its nw + 1 words of tail in n_words)
    assert not out.any() and not rep.any()
    assert call(n=0, packed_out=out.ctypes.data) == 0 and not out.any()       # no reads: PG_OK, nothing touched
    assert call(max_fixes=255, report=None) == 0 and out.any() and not rep.any()
    for bad in (dict(min_cov=0), dict(min_run=0), dict(max_fixes=256)):
        with pytest.raises(api.PgError, match=r"failed \(-1\)"):
            cor.ix.correct_ragged(words, off, base, 6, **dict(E.PARAMS, **bad))
    cor.close()


def test_correct_reads_and_report_fields():
    """api.correct_reads takes and returns base codes; report_fields splits the words as the header lays them out."""
    K = 31
    cor = E.Corrector(K, False, -1)
    cs = E.cases(K)
    reads = [c.read for c in cs]
    fixed, rep = api.correct_reads(reads, cor.ix, **E.PARAMS)
    want = [E.model_correct(cor.model, r, E.PARAMS) for r in reads]
    assert all(len(f) == len(r) and (f == w[0]).all() for f, r, w in zip(fixed, reads, want))
    assert [int(x) for x in rep] == [w[1] for w in want]
    f = api.report_fields(rep)
    for name, bit in (("no_kmers", C.NO_KMERS), ("no_anchor", C.NO_ANCHOR), ("stop_right", C.STOP_RIGHT), ("stop_left", C.STOP_LEFT),
                      ("limit", C.LIMIT)):
        assert [bool(x) for x in f[name]] == [bool(w[1] & bit) for w in want] and (any(f[name]) or name == "stop_left")
    assert list(f["fixes"]) == [w[1] & 0xFF for w in want] and list(f["weak"]) == [w[1] >> 32 for w in want]
    # the defaults are arguments like the others
    again, _ = api.correct_reads(reads, cor.ix, E.MIN_COV)
    want = [E.model_correct(cor.model, r, dict(min_cov=E.MIN_COV, max_fixes=api.CORRECT_MAX_FIXES, min_run=api.CORRECT_MIN_RUN)) for r in reads]
    assert all((f == w[0]).all() for f, w in zip(again, want))
    cor.close()


def test_left_sweep_stops_too():
    """STOP_LEFT: two errors next to each other in front of the anchor."""
    K = 31
    cor = E.Corrector(K, False, -1)
    read = E.cases(K)[10].truth.copy()
    read[[3, 4]] ^= 2
    got, rep = E.model_correct(cor.model, read, E.PARAMS)
    assert (got == read).all() and rep & E.FLAGS == C.STOP_LEFT and rep & 0xFF == 0
    cor.check([read], "stop left", **E.PARAMS)
    cor.close()


@pytest.fixture(scope="module")
def simulated_index(tmp_path_factory):
    reads, truth = E.simulated()
    records, _, _ = oracle_records(reads, E.SIM_K, 8, prefix=str(tmp_path_factory.mktemp("kcorrect") / "o"))
    cor = E.Corrector(E.SIM_K, False, -1, records=records)
    yield cor
    cor.close()


def test_simulated_set(simulated_index):
    """A circular genome of 3 000 bases, 900 reads of 100 bases from both strands (30x), every base substituted with probability 0.005,
    K = 31, the records the oracle counts from these reads, min_cov = 3, api's default max_fixes and min_run.  The twin equals the model
    read for read; and, by the model: no read without an error is changed, no base that was right is changed, and at least 90 % of the
    reads with errors come back equal to the error-free read (the model restores 340 of this set's 347: 98.0 %)."""
    cor = simulated_index
    reads, truth = E.simulated()
    K, model = E.SIM_K, cor.model
    # every k-mer of the genome is solid and no k-mer that only an error made is
    genome_kmers = {k for r in truth for k in M.canonical_kmers(r, K)}
    error_kmers = {k for r in reads for k in M.canonical_kmers(r, K)} - genome_kmers
    assert len(genome_kmers) == E.SIM_GENOME and error_kmers
    assert min(M.coverage(model.cnt.get(k, 0)) for k in genome_kmers) >= E.SIM_MIN_COV
    assert max(M.coverage(model.cnt[k]) for k in error_kmers) < E.SIM_MIN_COV
    fixed, report = E.simulated_model_output(model)
    had = (reads != truth).any(axis=1)
    assert 300 < had.sum() < 600
    assert (fixed[~had] == reads[~had]).all() and not report[~had].any()
    assert not ((fixed != truth) & (reads == truth)).any()
    restored = (fixed[had] == truth[had]).all(axis=1)
    print("restored %d of %d reads with errors" % (restored.sum(), had.sum()))
    assert restored.mean() >= 0.9
    params = dict(min_cov=E.SIM_MIN_COV, max_fixes=api.CORRECT_MAX_FIXES, min_run=api.CORRECT_MIN_RUN)
    got, rep = cor.check(list(reads), "simulated, uniform", uniform=True, **params)
    got_r, rep_r = cor.check(list(reads), "simulated, ragged, in place", in_place=True, **params)
    assert (got == got_r).all() and (rep == report).all() and (rep_r == report).all()
