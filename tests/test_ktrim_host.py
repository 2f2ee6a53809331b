"""The trim on the CPU: the host twin (pg_kindex_trim on a device = -1 index, one table or cut over a list of -1s: csrc/ktrim_host.cpp,
the rule the kernels share in csrc/ktrim.hpp) against the independent model (tests/ktrim_model.py) on the designed cases of
tests/ktrim_cases.py, on the simulated read set of the corrector's tests counted by the oracle, and under -fsanitize=address,undefined
in a stand-alone program.  tests/test_gpu_ktrim.py runs the same through the kernels.  All comparisons are of integers and exact."""

import numpy as np
import pytest

import kcorrect_cases as C
import kindex_model as M
import ktrim_cases as E
from conftest import oracle_records
from host_program import build_and_run
from soapdenovo2_amd import api


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_host_twin_matches_model(flavour):
    """Every designed case gives the span it is named for in the model, and the twin gives the model's spans, words, offsets, source
    indices and totals: alone (ragged and uniform), in one ragged batch with min_len = K, K + 1 and K + 5, with reads without k-mers
    between others, in batches of 1, 63, 64, 65, 257 and 4 097 reads with a seeded keep / drop pattern, all kept and all dropped, and
    with spans only."""
    E.check_flavour(flavour[0], flavour[1], device=-1)


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=E.flavour_id)
def test_cut_over_ranks_gives_the_single_tables_words(flavour):
    E.check_ranks(flavour[0], flavour[1], lambda n: (-1,) * n)


def test_batches_of_one_scan_round_and_one_block_more():
    """65 536 reads (256 blocks of 256: exactly one round of the device's scan over the blocks' sums) and 65 537 (one block in the
    second round), K = 13, each read kept whole or dropped by a seeded random bit: totals, src_out, word_off_out and kmer_base_out are
    cumulative sums of the bit vector and packed_out is the kept template's word repeated (tests/ktrim_cases.py: check_rounds)."""
    E.check_rounds(-1)


def test_argument_errors():
    K = 31
    t = E.Trimmer(K, False, -1)
    reads = [c.read for c in E.cases(K)[:6]]
    words, off, base, _ = E.pack(reads, K, 2, False)
    n = len(reads)
    out, w_off, k_base, src, tot, span = (np.zeros_like(words), np.zeros(n, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64),
                                          np.zeros(n, dtype=np.uint64), np.full(4, 7, dtype=np.uint64), np.zeros(n, dtype=np.uint64))
    L = api.lib()

    def call(min_cov=3, min_len=K + 1, n=n, packed_out=out.ctypes.data, word_off_out=w_off.ctypes.data, kmer_base_out=k_base.ctypes.data,
             src_out=src.ctypes.data, totals=tot.ctypes.data, out_span=span.ctypes.data, n_words=len(words), ulen=0, n_kmers=int(base[-1])):
        return L.pg_kindex_trim(t.ix.h, words.ctypes.data, n_words, off.ctypes.data, base.ctypes.data, n, ulen, n_kmers, min_cov, min_len,
                                out_span, packed_out, word_off_out, kmer_base_out, src_out, totals, None)

    einval = -1                                                 # PG_EINVAL (include/soapdenovo2_amd.h)
    assert call(min_cov=0) == einval and b"min_cov" in L.pg_last_error()
    assert call(min_len=K - 1) == einval and call(packed_out=words.ctypes.data) == einval
    assert call(word_off_out=None) == einval and call(kmer_base_out=None) == einval and call(totals=None) == einval
    assert call(packed_out=None, out_span=None) == einval
    assert call(ulen=101, n_kmers=n * 71, n_words=n * 4 + 2) == einval     # (a uniform batch needs its nw + 1 words of tail in n_words)
    assert call(ulen=101, n_kmers=n * 71 + 1, n_words=n * 4 + 3) == einval
    assert not out.any() and not span.any() and (tot == 7).all()
    assert call(n=0) == 0 and not tot.any() and not out.any()                # no reads: PG_OK, the totals zeroed
    assert call(min_len=K, src_out=None, out_span=None) == 0 and int(tot[0]) > 0 and out.any() and not src.any() and not span.any()
    assert call(packed_out=None) == 0 and span.any()
    for bad in (dict(min_cov=0), dict(min_cov=3, min_len=K - 1)):
        with pytest.raises(api.PgError, match=r"failed \(-1\)"):
            t.ix.trim_ragged(words, off, base, n, int(base[-1]), **bad)
    t.close()


def test_trim_reads_and_span_fields():
    """api.trim_reads takes and returns base codes; span_fields splits the words as the header lays them out; min_len defaults to K + 1."""
    K = 31
    t = E.Trimmer(K, False, -1)
    reads = [c.read for c in E.cases(K)]
    w = E.want(t.model, reads, K + 1)
    kept, src, spans = api.trim_reads(reads, t.ix, E.MIN_COV)
    assert len(kept) == len(w.reads) and all(len(a) == len(b) and (a == b).all() for a, b in zip(kept, w.reads))
    assert (src == w.src.astype(np.int64)).all() and (spans == w.spans).all()
    f = api.span_fields(spans)
    assert [(int(s), int(n)) for s, n in zip(f["start"], f["len"])] == [E.model_span(t.model, r) for r in reads]
    fewer, _, _ = api.trim_reads(reads, t.ix, E.MIN_COV, E.min_len_of(K))
    assert len(fewer) == int(E.want(t.model, reads, E.min_len_of(K)).totals[0]) < len(kept)
    t.close()


@pytest.fixture(scope="module")
def simulated_index(tmp_path_factory):
    reads, _ = C.simulated()
    records, _, _ = oracle_records(reads, C.SIM_K, 8, prefix=str(tmp_path_factory.mktemp("ktrim") / "o"))
    t = E.Trimmer(C.SIM_K, False, -1, records=records)
    yield t
    t.close()


def test_simulated_set(simulated_index):
    """The corrector's simulated set (a circular genome of 3 000 bases, 900 reads of 100 bases, every base substituted with probability
    0.005, K = 31, the oracle's records, min_cov = 3): after the trim every k-mer of every kept read is solid, and a recount of the kept
    reads holds exactly the distinct k-mers of the model's trimmed reads, none of them weak -- and so after correct, then trim."""
    t = simulated_index
    reads, truth = C.simulated()
    K, model = C.SIM_K, t.model
    before = len(M.count_reads(reads, K)[0])
    corrected, _ = api.correct_reads(list(reads), t.ix, C.SIM_MIN_COV)
    for what, batch in (("trim", list(reads)), ("correct then trim", corrected)):
        packed, word_off, kmer_base, src, totals = t.check(batch, "simulated, " + what, min_len=K + 1, uniform=True, min_cov=C.SIM_MIN_COV)
        kept = E.unpack(packed, word_off, kmer_base, K)
        w = E.want(model, batch, K + 1, C.SIM_MIN_COV)
        assert len(kept) == len(w.reads) and all((a == b).all() for a, b in zip(kept, w.reads))
        distinct = E.check_recount(model, kept, C.SIM_MIN_COV)
        assert distinct == len(M.count_reads(w.reads, K)[0]) <= C.SIM_GENOME < before
        print("%s: %d of %d reads kept, %d bases removed, %d distinct k-mers (%d before)" % (what, totals[0], len(batch), totals[3], distinct, before))
        assert 0 < int(totals[3]) and int(totals[0]) > 850


# ---- the host twin under the sanitizers, in a program of its own ----
def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/ktrim_asan.cpp: both flavours, one table and 3 ranks, a ragged and a uniform batch with exactly nw + 1 words of tail, every
    output buffer on the heap at exactly the capacity the header states -- compiled with the host twin's sources and
    -fsanitize=address,undefined, and run.  Nothing loaded into Python is sanitised."""
    build_and_run(tmp_path, "ktrim_asan", ["kindex_host.cpp", "ktrim_host.cpp"], ["ktrim host twin: ok"])
