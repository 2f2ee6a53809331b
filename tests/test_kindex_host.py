"""The k-mer index on the CPU: the host twin (pg_kindex_build with device = -1: the table, lookups and summary code the kernels share,
csrc/kindex.hpp) against the independent model (tests/kindex_model.py), on hand-made tables at the layout's edges and on the records
the oracle counts from synthetic reads.  tests/test_gpu_kindex.py runs the same cases through the build kernel and the two query
kernels.  All comparisons are of integers and exact."""
import numpy as np
import pytest

import kindex_cases as E
import kindex_model as M
from conftest import oracle_records
from soapdenovo2_amd import api, synth


def test_model_restates_the_hash():
    """The model's key_hash is the library's: bits 40 and up, which is what pg_host_map_owner shows of it (owner = (hash >> 40) % n, so
    n = 2^24 gives them all).  Bits 39:0 -- the ones a home slot is made of -- are the same multiply chain's and have no public view."""
    for K, mer127 in E.FLAVOURS:
        nw = 4 if mer127 else 2
        keys = E.table("n513", K, mer127)[1]
        words = np.array([M.words_of_key(k, nw) for k in keys], dtype=np.uint64)
        assert (api.map_owner(words, 1 << 24, mer127) == np.array([M.key_hash(k, nw) >> 40 for k in keys], dtype=np.uint32)).all()


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_colliding_table_has_long_probe_runs(flavour):
    K, mer127 = flavour
    nw = 4 if mer127 else 2
    _, keys = E.table("colliding", K, mer127)
    homes = [M.home_slot(k, nw, len(keys)) for k in keys]
    assert max(np.bincount(homes)) >= 3
    assert M.longest_probe_run(keys, nw) >= 3


@pytest.mark.parametrize("name", E.TABLES)
@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_host_twin_matches_model(flavour, name):
    E.check_table(name, flavour[0], flavour[1], device=-1)


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_host_twin_long_sequences(flavour):
    """The sequences of the wave kernel's edges through the host twin: the last base changed makes the last k-mer alone absent."""
    K, mer127 = flavour
    ix = E.Index(E.table("genome", K, mer127)[0], K, mer127, -1)
    seqs, tags = E.wave_sequences(K)
    cnt, summ = ix.check_ragged(seqs, what="long sequences")
    for t, s, row in zip(tags, seqs, summ):
        nk = len(s) - K + 1
        assert list(row[[0, 3]]) == ([nk - 1, nk - 1] if t.endswith("last-absent") else [nk, nk]), t
    ix.close()


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_counts_or_summary_alone(flavour):
    K, mer127 = flavour
    ix = E.Index(E.table("n513", K, mer127)[0], K, mer127, -1)
    seqs, _ = E.sequences(K)
    cnt, summ, _ = ix.ragged(seqs)
    only_cnt, none, _ = ix.ragged(seqs, summary=False)
    none2, only_summ, _ = ix.ragged(seqs, counts=False)
    assert none is None and none2 is None and (only_cnt == cnt).all() and (only_summ == summ).all()
    with pytest.raises(api.PgError):
        ix.ix.query_ragged(*api.pack_seqs_ragged(seqs, K)[:3], len(seqs), 0, counts=False, summary=False)
    ix.close()


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_duplicate_key_fails_the_build(flavour):
    K, mer127 = flavour
    records = E.table("n513", K, mer127)[0]
    twice = np.concatenate([records, records[0:1]])             # (the first record is never a deleted one)
    with pytest.raises(api.PgError, match=r"duplicate key in records \(PG_EINVAL\)"):
        api.KmerIndex.from_records(twice, K, mer127, device=-1)


def test_bad_k_fails_the_build():
    rec2, rec4 = np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 6), dtype=np.uint64)
    for K, mer127, rec in [(30, False, rec2), (11, False, rec2), (65, False, rec2), (64, True, rec4), (129, True, rec4)]:
        with pytest.raises(api.PgError, match=r"\(PG_EINVAL\)"):
            api.KmerIndex.from_records(rec, K, mer127, device=-1)


def test_kmer_coverage_takes_short_sequences():
    K = 31
    ix = E.Index(E.table("genome", K, False)[0], K, False, -1)
    seqs, _ = E.sequences(K)
    cov = api.kmer_coverage(seqs, ix.ix)
    assert [len(c) for c in cov] == [max(0, len(s) - K + 1) for s in seqs]
    for s, c in zip(seqs, cov):
        assert list(c) == [M.coverage(a) for a in ix.model.query(s)]
    ix.close()


# ---- round trip: count reads, index the records, ask with the same reads ----
@pytest.fixture(scope="module", params=[(31, False), (65, True)], ids=E.flavour_id)
def counted(request):
    K, mer127 = request.param
    codes = synth.reads_codes(3000, 3000, 100, 0.01, 7)
    return (K, mer127, codes) + M.count_reads(codes, K)


@pytest.mark.parametrize("delow", [0, 1])
def test_round_trip_through_the_oracle(counted, delow, tmp_path):
    """delow = 0: every k-mer of the reads is present, and a k-mer of coverage c < 255 is returned by exactly c query positions.
    delow = 1: exactly the k-mers the model says the filter removed (M.filtered) read as 0."""
    K, mer127, codes, occ, arcs = counted
    records, _, _ = oracle_records(codes, K, 8, D=delow, mer127=mer127, prefix=str(tmp_path / "o"))   # (the oracle writes <prefix>.kmerFreq)
    ix = E.Index(records, K, mer127, -1)
    cnt, summ = ix.uniform(codes)
    ix.close()
    E.check_round_trip(codes, K, occ, M.filtered(arcs, delow), delow, cnt, summ)
