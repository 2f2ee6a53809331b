"""The k-mer index cut over ranks on the GPU, every rank on GPU 0 (an ordinal may repeat: a rank is a table, a stream and its buffers):
kidx_count_owners_kernel, kidx_build_kernel for an owner, kidx_probe_owned_kernel, the rows' merge and kidx_summary_rows_kernel
(csrc/kindex_kernels.hip) against the independent model (tests/kindex_model.py), against the index in one table on the device and
against the host twin, on the cases of tests/test_kindex_sharded_host.py -- but the duplicate key, which stays on the host twin: no test
here is built around making a kernel fail.  Ranks on different physical GPUs are not run here.  All comparisons are of integers and
exact; no test asserts a time or a rate."""
import re

import numpy as np
import pytest

import kindex_cases as E
import kindex_model as M
import kindex_sharded_cases as S
from soapdenovo2_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every test makes and destroys indexes of several tables each, so the module pins the device arena (tests/test_gpu_map_sharded.py)."""
    with api.arena_pinned(0):
        yield


def gpu(n):
    return (0,) * n


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


@pytest.mark.parametrize("name", E.TABLES)
@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_three_ranks_match_model(flavour, name):
    S.check_table(name, flavour[0], flavour[1], gpu(3), waves=(False, True))


@pytest.mark.parametrize("n", [n for n in S.RANKS if n != 3])
@pytest.mark.parametrize("name", E.TABLES)
@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_every_rank_count_matches_model(flavour, name, n):
    """(`one` over 8 ranks -- seven ranks launch no insert and keep a zeroed table -- and `empty` over every n are among these.)"""
    S.check_table(name, flavour[0], flavour[1], gpu(n), waves=(False, True))


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_wave_probe_edges(flavour):
    """Sequences of 1, 63, 64, 65, 128, 129 and 4 097 k-mers, each also with its last k-mer alone absent, through the wave probe over 3
    ranks; the lane probe gives the same words."""
    K, mer127 = flavour
    ix = S.Index(E.table("genome", K, mer127)[0], K, mer127, gpu(3))
    seqs, tags = E.wave_sequences(K)
    cnt, summ = ix.check_ragged(seqs, wave=True, what="wave")
    for t, s, row in zip(tags, seqs, summ):
        nk = len(s) - K + 1
        assert list(row[[0, 3]]) == ([nk - 1, nk - 1] if t.endswith("last-absent") else [nk, nk]), t
    lane_cnt, lane_summ = ix.check_ragged(seqs, wave=False, what="lane")
    assert (lane_cnt == cnt).all() and (lane_summ == summ).all()
    ix.close()


@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_counts_or_summary_alone(flavour, wave):
    """Counts alone: the lead's rows are the caller's and no summary runs; summary alone: the rows are the index's own."""
    K, mer127 = flavour
    ix = S.Index(E.table("n513", K, mer127)[0], K, mer127, gpu(3))
    seqs = E.sequences(K)[0] + E.wave_sequences(K)[0][:6]
    cnt, summ, _ = ix.ragged(seqs, wave)
    only_cnt, none, _ = ix.ragged(seqs, wave, summary=False)
    none2, only_summ, _ = ix.ragged(seqs, wave, counts=False)
    assert none is None and none2 is None and (only_cnt == cnt).all() and (only_summ == summ).all()
    w_cnt, w_summ = ix.want(seqs)
    assert (cnt == w_cnt).all() and (summ == w_summ).all()
    ix.close()


@pytest.mark.parametrize("name", E.TABLES)
@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_same_words_as_one_table_and_as_the_host_twin(flavour, name):
    K, mer127 = flavour
    records = E.table(name, K, mer127)[0]
    seqs = E.sequences(K)[0] + E.wave_sequences(K)[0]
    one = E.Index(records, K, mer127, 0)
    cnt, summ, _ = one.ragged(seqs)
    want = np.concatenate([cnt, summ.reshape(-1)])
    one.close()
    for n in S.RANKS:
        twin = S.Index(records, K, mer127, (-1,) * n)
        assert (twin.words(seqs) == want).all(), n
        info = twin.ix.info()
        twin.close()
        ix = S.Index(records, K, mer127, gpu(n))
        got = ix.ix.info()
        assert [dict(r, device=-1) for r in got["ranks"]] == info["ranks"] and (got["keys"], got["slots"], got["bytes"]) == (info["keys"], info["slots"], info["bytes"])
        for wave in (False, True):
            assert (ix.words(seqs, wave) == want).all(), (n, wave)
        ix.close()


@pytest.mark.parametrize("name", ["one", "n513"])
@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_one_table_is_a_one_rank_cut(flavour, name):
    """pg_kindex_build's table is rank 0 of a cut over one rank: the build kernel with n == 1 works no owner out, whichever entry made
    the index.  The same records -- a deleted one among them: `one` gets a deleted record of `n513` behind its own -- as an index in one
    table, as a one-rank cut and as the host twin: the same keys, slots and bytes, and with the lane and the wave query the same
    answers and summaries, which are the model's."""
    K, mer127 = flavour
    records = E.table(name, K, mer127)[0]
    nw = records.shape[1] - 2
    if name == "one":
        more = E.table("n513", K, mer127)[0][1:]                               # (n513's first key is `one`'s)
        records = np.concatenate([records, more[(more[:, nw] >> np.uint64(32 + 25)) & np.uint64(1) == 1][:1]])
        assert len(records) == 2
    assert ((records[:, nw] >> np.uint64(32 + 25)) & np.uint64(1)).any() and not ((records[:, nw] >> np.uint64(32 + 25)) & np.uint64(1)).all()
    seqs = E.sequences(K)[0] + E.wave_sequences(K)[0][:8]
    made = [E.Index(records, K, mer127, 0), S.Index(records, K, mer127, gpu(1)), E.Index(records, K, mer127, -1)]
    assert [x.ix.sharded for x in made] == [False, True, False]
    infos = [x.ix.info() for x in made]
    assert all((i["keys"], i["slots"], i["bytes"]) == (len(records), M.table_slots(len(records)), api.host_kindex_bytes(len(records), mer127)) for i in infos)
    assert all(len(i["ranks"]) == 1 and {k: i["ranks"][0][k] for k in ("keys", "slots", "bytes")} == {k: i[k] for k in ("keys", "slots", "bytes")} for i in infos)
    want = made[2].check_ragged(seqs, what="host twin")
    assert want[0].any() and not want[0].all()                               # (some k-mers present, some absent)
    for x, what in zip(made[:2], ("one table", "one-rank cut")):
        for wave in (False, True):
            cnt, summ = x.check_ragged(seqs, wave, "%s wave=%s" % (what, wave))
            assert (cnt == want[0]).all() and (summ == want[1]).all(), (what, wave)
    for x in made:
        x.close()


@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_summary_kernel_edges(flavour):
    """Batches of 1, 3, 4, 5 and 257 sequences (a workgroup of the summary kernel takes four), with sequences without k-mers between
    others, ragged and uniform, with both probes."""
    K, mer127 = flavour
    ix = S.Index(E.table("genome", K, mer127)[0], K, mer127, gpu(3))
    g = E.genome(K)
    none = np.zeros(K - 1, dtype=np.uint8)
    pool = [g[7 * i:7 * i + K + i % 70].copy() if i % 5 != 2 else none for i in range(257)]
    pool[100] = g[3:3 + 300 + K - 1].copy()
    pool[100][150] ^= 1                                                         # some absent k-mers in the middle of a long row
    for n in (1, 3, 4, 5, 257):
        for wave in (False, True):
            ix.check_ragged(pool[:n] if n > 1 else pool[3:4], wave, "summary, %d sequences wave=%s" % (n, wave))
    ix.check_ragged([none, pool[0], none, none, pool[1], none], True, "summary, k-mer-less between")
    for n in (1, 3, 4, 5, 257):
        codes = np.stack([g[11 * i:11 * i + K + 40] for i in range(n)])
        codes[n // 2, 50] ^= 2
        cnt, summ = ix.uniform(codes, wave=n % 2 == 1)
        w_cnt, w_summ = ix.want(list(codes))
        assert (cnt == w_cnt).all() and (summ == w_summ).all(), "uniform %d" % n
    ix.close()


@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_parts(flavour, monkeypatch):
    """One tensor; three tensors (read where they lie); a numpy host part beside a tensor (the host part through the chunk buffer); and
    with chunks of 256 records a host part of 513 (chunks of 256, 256 and 1) and one of 256 (exactly one chunk) over (0, 0)."""
    K, mer127 = flavour
    records, keys = E.table("genome", K, mer127)
    seqs = E.sequences(K)[0] + E.wave_sequences(K)[0][:6]
    want = None
    splits = {"one tensor": [up(records)],
              "three tensors": [up(records[:1000]), up(records[1000:1001]), up(records[1001:])],
              "a host part and a tensor": [np.ascontiguousarray(records[:1500]), up(records[1500:])]}
    for what, parts in splits.items():
        ix = S.Index(records, K, mer127, gpu(3), parts=parts)
        S.check_info(ix.ix, keys, ix.nw, gpu(3))
        got = ix.check_ragged(seqs, what=what) + ix.check_ragged(seqs, wave=True, what=what)
        ix.close()
        want = want or got
        assert all((a == b).all() for a, b in zip(got, want)), what
    monkeypatch.setenv("SOAPDENOVO2_AMD_KINDEX_CHUNK_RECORDS", "256")
    for n in (513, 256):
        part = np.ascontiguousarray(records[:n])
        for parts in ([part], [part[:1], up(part[1:2]), part[2:]]):
            ix = S.Index(part, K, mer127, gpu(2), parts=parts)
            S.check_info(ix.ix, keys[:n], ix.nw, gpu(2))
            ix.check_ragged(seqs, what="chunks of 256, %d records" % n)
            ix.close()


@pytest.fixture(scope="module", params=S.WIDE, ids=E.flavour_id)
def counted(request):
    K, mer127 = request.param
    codes = synth.reads_codes(3000, 3000, 100, 0.01, 7)
    return (K, mer127, codes) + M.count_reads(codes, K)


def test_round_trip_through_the_counter(counted):
    """tests/test_gpu_kindex.py's round trip with the index cut over 3 ranks: KmerCounter -> finalize(delow = 1) -> index(devices) ->
    query_uniform of the same device batch, with both probes."""
    import torch
    K, mer127, codes, occ, arcs = counted
    delow = 1
    kc = api.KmerCounter(K, n_sets=8, mer127=mer127, log2_slots=18)
    packed = torch.from_numpy(api.pack_reads_uniform(codes).view(np.int64)).cuda()
    kc.count_uniform(packed, codes.shape[0], codes.shape[1], 0)
    kc.finalize(delow)
    ix = kc.index(devices=gpu(3))
    info = ix.info()
    assert ix.sharded and info["keys"] == kc.distinct() == len(occ) and len(info["ranks"]) == 3 and info["device"] == 0
    assert sorted(r["keys"] for r in info["ranks"]) == sorted(S.owner_counts(list(occ), 4 if mer127 else 2, 3))
    kc.close()                                                 # (the index owns its tables: the counter and its records may go)
    for wave in (False, True):
        cnt, summ = ix.query_uniform(packed, codes.shape[0], codes.shape[1], wave=wave, counts=True, summary=True)
        cnt, summ = cnt.cpu().numpy().view(np.uint64), summ.cpu().numpy().view(np.uint64)
        E.check_round_trip(codes, K, occ, M.filtered(arcs, delow), delow, cnt, summ)
    ix.close()


@pytest.mark.parametrize("flavour", S.WIDE, ids=E.flavour_id)
def test_back_to_back_queries(flavour):
    """Two queries on one index with no host wait between them, a larger batch and then a smaller one, the second one with the other
    probe: the ranks' row buffers and the staging buffer are reused, and both answers are right -- with the caller's rows and with
    the index's own (summary alone)."""
    K, mer127 = flavour
    ix = S.Index(E.table("genome", K, mer127)[0], K, mer127, gpu(3))
    big, small = E.wave_sequences(K)[0], E.sequences(K)[0]
    batches = []
    for seqs in (big, small):
        words, off, base = api.pack_seqs_ragged(seqs, K)
        batches.append((up(words), up(off), up(base), len(seqs), int(base[-1])))
    for counts in (True, False):
        got = [ix.ix.query_ragged(*b, wave=i == 0, counts=counts, summary=True) for i, b in enumerate(batches)]     # (nothing waited for yet)
        for seqs, g in zip((big, small), got):
            w_cnt, w_summ = ix.want(seqs)
            cnt, summ = g if counts else (None, g)
            assert (summ.cpu().numpy().view(np.uint64) == w_summ).all()
            assert cnt is None or (cnt.cpu().numpy().view(np.uint64) == w_cnt).all()
    ix.close()


def test_budget_hook(monkeypatch):
    """With a rank's table capped at 1 MB the 20 000-key table (3 MB as one table in the 127-mer build) is refused over one rank, the
    message names the ranks that hold it, nothing stays allocated, and over that many ranks the same build succeeds."""
    K, mer127 = 65, True
    records, keys, codes = S.budget_table(K, mer127)
    monkeypatch.setenv("SOAPDENOVO2_AMD_KINDEX_BUDGET_MB", "1")
    before = api.arena_stats(0)["in_use"]
    with pytest.raises(api.PgError, match=r"rank 0's table is 3145728 bytes.* ranks would hold it \(PG_ENOMEM\)") as e:
        api.KmerIndex.from_records(records, K, mer127, gpu(1))
    assert api.arena_stats(0)["in_use"] == before
    n = int(re.search(r"(\d+) ranks would hold it", str(e.value)).group(1))
    assert n == 3                                                             # 16 384 slots of 48 B are the most 1 MB holds: 8 192 keys a rank
    with pytest.raises(api.PgError, match=r"\(PG_ENOMEM\)"):
        api.KmerIndex.from_records(records, K, mer127, gpu(n - 1))
    assert api.arena_stats(0)["in_use"] == before
    ix = S.Index(records, K, mer127, gpu(n))
    S.check_info(ix.ix, keys, ix.nw, gpu(n))
    assert max(r["bytes"] for r in ix.ix.info()["ranks"]) <= 1 << 20
    ix.check_ragged([codes[:300], codes[5000:5200], E.rc(codes[900:1100]), E.genome(K)[:200]], what="budget")
    ix.close()
    assert api.arena_stats(0)["in_use"] == before


def test_bad_ordinals():
    records = E.table("n513", 31, False)[0]
    before = api.arena_stats(0)["in_use"]
    with pytest.raises(api.PgError, match=r"mixes.*\(PG_EINVAL\)"):
        api.KmerIndex.from_records(records, 31, False, (0, -1))
    with pytest.raises(api.PgError, match=r"does not exist \(PG_ENODEV\)"):
        api.KmerIndex.from_records(records, 31, False, (0, 1 << 20))
    with pytest.raises(api.PgError, match=r"does not exist"):
        api.KmerIndex.from_records(up(records), 31, False, (1 << 20, 0))
    assert api.arena_stats(0)["in_use"] == before
    ix = S.Index(records, 31, False, gpu(2))                                   # and the device is as good as before
    ix.check_ragged(E.sequences(31)[0], what="after the refusals")
    ix.close()


def test_kmer_coverage_and_corrector_refusal():
    K = 31
    ix = S.Index(E.table("genome", K, False)[0], K, False, gpu(3))
    seqs, _ = E.sequences(K)
    for wave in (False, True):
        cov = api.kmer_coverage(seqs, ix.ix, wave=wave)
        for s, c in zip(seqs, cov):
            assert list(c) == [M.coverage(a) for a in ix.model.query(s)]
    words, off, base = api.pack_seqs_ragged(seqs, K)
    with pytest.raises(api.PgError, match="cut over ranks"):
        ix.ix.correct_ragged(up(words), up(off), up(base), len(seqs), 3)
    ix.close()
