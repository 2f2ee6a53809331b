"""The k-mer index cut over ranks on the CPU: the host twin of pg_kindex_build_sharded / pg_kindex_query_words (a device list of -1s: n
serial tables, csrc/kindex_host.cpp) against the independent model (tests/kindex_model.py) and against the index in one table, on the
cases of tests/kindex_cases.py; the cut against its Python statement (tests/kindex_sharded_cases.py: owner); parts; refusals;
pg_host_kindex_plan against a restatement of its arithmetic; and the twin under -fsanitize=address,undefined in a stand-alone program.
tests/test_gpu_kindex_sharded.py runs the same cases through the kernels.  All comparisons are of integers and exact."""

import numpy as np
import pytest

import kindex_cases as E
import kindex_model as M
import kindex_sharded_cases as S
from host_program import build_and_run
from soapdenovo2_amd import api


def host(n):
    return (-1,) * n


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_map_owner_is_the_stated_cut(flavour):
    """api.map_owner on every key of every table, for every rank count used here and two that are no power of two."""
    K, mer127 = flavour
    nw = 4 if mer127 else 2
    for name in E.TABLES:
        keys = E.table(name, K, mer127)[1]
        words = np.array([M.words_of_key(k, nw) for k in keys], dtype=np.uint64).reshape(-1, nw)
        for n in S.RANKS + [7, 255, 256]:
            assert list(api.map_owner(words, n, mer127)) == [S.owner(k, nw, n) for k in keys], (name, n)


@pytest.mark.parametrize("name", E.TABLES)
@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_three_ranks_match_model(flavour, name):
    S.check_table(name, flavour[0], flavour[1], host(3))


@pytest.mark.parametrize("n", S.RANKS)
@pytest.mark.parametrize("name", E.TABLES)
@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_every_rank_count_matches_model(flavour, name, n):
    S.check_table(name, flavour[0], flavour[1], host(n))


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_designed_cuts(flavour):
    """`one` over 8 ranks: seven ranks own nothing and keep a zeroed table of the smallest size; the genome over 2, 3 and 8: every rank
    owns keys (both asserted of the keys in the case file, here of the index)."""
    K, mer127 = flavour
    ix = S.Index(E.table("one", K, mer127)[0], K, mer127, host(8))
    ranks = ix.ix.info()["ranks"]
    assert sorted(r["keys"] for r in ranks) == [0] * 7 + [1] and all(r["slots"] == 1024 for r in ranks)
    ix.check_ragged(E.sequences(K)[0], what="one over 8")
    ix.close()
    for n in (2, 3, 8):
        ix = S.Index(E.table("genome", K, mer127)[0], K, mer127, host(n))
        assert min(r["keys"] for r in ix.ix.info()["ranks"]) >= 1
        ix.close()


@pytest.mark.parametrize("name", E.TABLES)
@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_same_words_as_one_table(flavour, name):
    """Every answer and summary word of the short and the long sequences: the index in one table and the cut over every n."""
    K, mer127 = flavour
    records, keys = E.table(name, K, mer127)
    seqs = E.sequences(K)[0] + E.wave_sequences(K)[0]
    one = E.Index(records, K, mer127, -1)
    cnt, summ, _ = one.ragged(seqs)
    want = np.concatenate([cnt, summ.reshape(-1)])
    total = one.ix.info()["keys"]
    one.close()
    for n in S.RANKS:
        ix = S.Index(records, K, mer127, host(n))
        assert ix.ix.info()["keys"] == total == len(keys)
        got = ix.words(seqs)
        ix.close()
        assert got.shape == want.shape and (got == want).all(), n


@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_parts(flavour):
    """The same records as one part, as three parts of which one is empty, as parts of 255, 256 and 257 records, and permuted: the same
    per-rank counts and the same words.  A key in two different parts fails the build."""
    K, mer127 = flavour
    records, keys = E.table("genome", K, mer127)
    seqs = E.sequences(K)[0] + E.wave_sequences(K)[0][:6]
    n = len(records)
    assert n > 255 + 256 + 257
    perm = np.random.default_rng(9).permutation(n)
    splits = {"one part": [records],
              "three parts, one empty": [records[:1000], records[:0], records[1000:]],
              "255, 256, 257 and the rest": [records[:255], records[255:511], records[511:768], records[768:]],
              "permuted": [np.ascontiguousarray(records[perm][:n // 2]), np.ascontiguousarray(records[perm][n // 2:])],
              "no parts but empty ones": None}
    want = None
    for what, parts in splits.items():
        if parts is None:
            ix = S.Index(records[:0], K, mer127, host(3), parts=[records[:0], records[:0]])
            assert ix.ix.info()["keys"] == 0 and not ix.words(seqs)[:-4 * len(seqs)].any()
            ix.close()
            continue
        ix = S.Index(records, K, mer127, host(3), parts=parts)
        S.check_info(ix.ix, keys, ix.nw, host(3))
        got = ix.words(seqs)
        ix.check_ragged(seqs, what=what)
        ix.close()
        want = got if want is None else want
        assert (got == want).all(), what
    with pytest.raises(api.PgError, match=r"duplicate key in records \(PG_EINVAL\)"):
        api.KmerIndex.from_parts([records[:1000], np.concatenate([records[1000:], records[0:1]])], K, mer127, host(3))


def test_refusals():
    K, mer127 = 31, False
    records = E.table("n513", K, mer127)[0]
    seqs = E.sequences(K)[0]
    words, off, base = api.pack_seqs_ragged(seqs, K)
    ix = api.KmerIndex.from_records(records, K, mer127, host(2))
    out = np.zeros(int(base[-1]), dtype=np.uint64)
    L = api.lib()
    # pg_kindex_query does not carry the batch's extent: it names the entry that does
    rc = L.pg_kindex_query(ix.h, words.ctypes.data, off.ctypes.data, base.ctypes.data, len(seqs), 0, int(base[-1]), 0, out.ctypes.data, None, None)
    assert rc != 0 and b"pg_kindex_query_words" in L.pg_last_error() and not out.any()
    rc = L.pg_kindex_query_words(ix.h, words.ctypes.data, len(words), off.ctypes.data, base.ctypes.data, len(seqs), 0, int(base[-1]), 0,
                                 out.ctypes.data, None, None)
    assert rc == 0 and out.any()
    with pytest.raises(api.PgError, match="cut over ranks"):
        ix.correct_ragged(words, off, base, len(seqs), 3)
    codes = np.stack([s for s in seqs if len(s) == 2 * K + 1])
    with pytest.raises(api.PgError, match="cut over ranks"):
        ix.correct_uniform(api.pack_reads_uniform(codes), len(codes), codes.shape[1], 3)
    with pytest.raises(api.PgError, match="n_words"):                         # a uniform batch's words are checked against n_words
        ix._query(api.pack_reads_uniform(codes)[:len(codes) * api.packed_words(codes.shape[1])], None, None, len(codes), codes.shape[1],
                  len(codes) * (K + 2), False, True, False)
    ix.close()
    for devices in [(-1, 0), (0, -1), (), host(257), (-2,)]:
        with pytest.raises(api.PgError, match=r"\(PG_EINVAL\)"):
            api.KmerIndex.from_records(records, K, mer127, devices)
    # a null part with records; a device part given to the host twin
    devs, n_rec, where = np.array(host(2), dtype=np.int32), np.array([5], dtype=np.uint64), np.array([-1], dtype=np.int32)
    null = np.zeros(1, dtype=np.uint64)
    assert not L.pg_kindex_build_sharded(devs.ctypes.data, 2, K, 0, null.ctypes.data, n_rec.ctypes.data, where.ctypes.data, 1, None)
    assert b"null and has records (PG_EINVAL)" in L.pg_last_error()
    ptr, where = np.array([records.ctypes.data], dtype=np.uint64), np.array([0], dtype=np.int32)
    assert not L.pg_kindex_build_sharded(devs.ctypes.data, 2, K, 0, ptr.ctypes.data, n_rec.ctypes.data, where.ctypes.data, 1, None)
    assert b"host parts only (PG_EINVAL)" in L.pg_last_error()
    # an index in one table: no ranks, its own four words as rank 0, and pg_kindex_query_words is pg_kindex_query
    one = api.KmerIndex.from_records(records, K, mer127, -1)
    assert L.pg_kindex_ranks(one.h) == 0 and not one.sharded and one.info()["ranks"] == [{k: one.info()[k] for k in ("keys", "slots", "bytes", "device")}]
    out2 = np.zeros_like(out)
    assert L.pg_kindex_query_words(one.h, words.ctypes.data, len(words), off.ctypes.data, base.ctypes.data, len(seqs), 0, int(base[-1]), 0,
                                   out2.ctypes.data, None, None) == 0 and (out2 == out).all()
    one.close()


# ---- the plan ----
CHUNK_RECORDS = 1 << 22


def plan_restated(n_records, mer127, n, batch_kmers, batch_words, device_bytes):
    slot = ((4 if mer127 else 2) + 2) * 8
    share = (n_records + n - 1) // n
    keys = share + share // 16 + 1024 if n > 1 else n_records
    table = M.table_slots(keys) * slot
    chunk = min(CHUNK_RECORDS, n_records) * slot
    rows = batch_kmers * 8
    staging = rows if n > 1 else 0
    batch = 3 * batch_words * 8 if n > 1 else 0
    peak = table + max(chunk, rows + max(staging, batch))
    budget = int(float(device_bytes) * 0.85)
    return {"table": table, "slots": M.table_slots(keys), "keys": keys, "chunk": chunk, "rows": rows, "staging": staging, "batch_copy": batch,
            "peak": peak, "budget": budget, "fits": peak <= budget, "one_table": M.table_slots(n_records) * slot}


def test_plan():
    GB288 = 288 * 10**9
    for n_records in (0, 1, 513, 143_000_000, 1_100_000_000, 5_000_000_000):
        for mer127 in (False, True):
            for n in (1, 2, 3, 8, 256):
                for bk, bw, dev in ((10**8, 10**7, GB288), (0, 0, GB288), (10**6, 10**5, 10**9)):
                    got = api.kindex_plan(n_records, mer127, n, bk, bw, dev)
                    want = plan_restated(n_records, mer127, n, bk, bw, dev)
                    fewest = next((m for m in range(1, 257) if plan_restated(n_records, mer127, m, bk, bw, dev)["fits"]), 0)
                    assert got == dict(want, fewest_ranks=fewest), (n_records, mer127, n, bk, dev)
    # the issue's two sizes, 63-mer build on a 288 GB card: 1.1e9 keys are one table of 137 GB and fit; 5e9 are 550 GB and do not, and the
    # fewest ranks are the first n whose own plan fits
    small, big = api.kindex_plan(1_100_000_000), api.kindex_plan(5_000_000_000)
    assert small["fits"] and small["fewest_ranks"] == 1 and small["table"] == small["one_table"] == (1 << 32) * 32
    assert not big["fits"] and big["one_table"] == (1 << 34) * 32
    fits = [api.kindex_plan(5_000_000_000, n_ranks=n)["fits"] for n in range(1, big["fewest_ranks"] + 1)]
    assert big["fewest_ranks"] == 3 and fits == [False, False, True]
    for bad in (0, 257):
        with pytest.raises(api.PgError):
            api.kindex_plan(1000, n_ranks=bad)


# ---- the host twin under the sanitizers, in a program of its own ----
def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/kindex_sharded_asan.cpp: 3 ranks, 3 parts, both flavours, batches with exactly NW + 1 words of tail on the heap, against the
    index in one table -- compiled with the host twin's sources and -fsanitize=address,undefined, and run.  Nothing loaded into Python
    is sanitised."""
    build_and_run(tmp_path, "kindex_sharded_asan", ["kindex_host.cpp"], ["kindex sharded host twin: ok"])
