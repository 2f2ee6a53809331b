"""The inputs of tests/test_gpu_k2_partitions.py are what they claim to be: per partition, with the partition count forced as the GPU
tests force it, the records, the distinct records and the distinct canonical k-mers (tests/emu_skm.cpp: emu_skm_part_stats, the cutter's
own inline code run serially) meet the conditions under which the counting kernel must take several windows, split its key range, switch
its search for copies off or keep it on, and add whole windows of copies to one counter.  Conditions, not measurements: an input that
misses one is changed, never the bound.  No GPU.

What the inputs measure (per partition that holds a record: min / mean / max; every test prints its line with -s), 16 partitions unless said:

  input                         records               distinct records      distinct k-mers
  t6k_k31                       2725 / 3221 / 3760    1434 / 1597 / 1808    5045 / 5718 / 6404
  t6k_k31, 64 partitions         529 /  845 / 1105     282 /  411 /  559     994 / 1430 / 1976
  t8k_k63 (either flavour)      1725 / 2182 / 2620    1120 / 1417 / 1756    8197 / 9944 / 13026
  t6k_k127                      1100 / 1494 / 2138     989 / 1319 / 1893    9635 / 12945 / 18112
  t5k_k24 (K = 25)              2992 / 3230 / 3557    1644 / 1728 / 1845    4859 / 5080 / 5300
  d8k_k63                       1864 / 2171 / 2591    1172 / 1340 / 1703    6737 / 7872 / 9712
  the six, trimmed              633 .. 2135           589 .. 1437           3088 .. 11681   (min .. max over all of them)
  w1_k63                         371 /  407 /  429     371 /  405 /  427    7157 / 7967 / 8481
  w1_k127                        152 /  170 /  193     152 /  169 /  193    5272 / 6098 / 6882
  dd_off_k127                   5761 / 6032 / 6340    5561 / 5816 / 6129    103335 / 109230 / 115107
  dd_on_k127                    4887 / 6072 / 7001    1070 / 1440 / 1662    4398 / 6242 / 7490
  heavy K = 31 / 25 / 63 / 127  hot partitions >= 1309, <= 2185 records; all: 37 .. 2185, 33 .. 367 distinct, 716 .. 1586 k-mers
  heavy, long reads             hot partitions >= 3927, <= 6488 records; all: 102 .. 6488, 93 .. 691 distinct, 1167 .. 2335 k-mers
  one record (2 WIN + 17)       1041 (401 four-word)  1                     1 (poly-A) or 13 (period 13)"""
import numpy as np
import pytest

import k2_partition_cases as kc
from conftest import case_codes
from soapdenovo2_amd import api


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return kc.build_emu(tmp_path_factory.mktemp("emu"))


def _stats(emu, tag, reads, K, m127, log2_parts=kc.LOG2_PARTS, lens=None):
    st = kc.part_stats(emu, reads, K, m127, log2_parts, lens=lens)
    print(f"{tag} K={K} {'four' if m127 else 'two'}-word, {1 << log2_parts} partitions: {kc.describe(st)}")
    assert int(st[0].max()) <= kc.MAX_PART_RECORDS < kc.CHUNK_LIST_RECORDS          # never the chunk-list fallback
    return st


def test_a_window_of_copies_fits_a_counter_half():
    """cnt[0..3] hold two arc counters a word.  Between two windows the halves are clipped to 255, a window adds at most WIN records of nmax
    k-mers to one of them: 512 * 127 + 255 = 65279, 256 short of the carry into the neighbour -- at K <= 31, where a record reaches 127 k-mers
    in the two-word flavour; the same 127 and 511 are the full widths of the two header fields the search for copies packs."""
    assert kc.WIN[2] * kc.nmax(31) + 255 == 65536 - 257
    assert kc.nmax(31) == 127 and kc.WIN[2] == kc.COPIES_MAX
    for K, m127 in [(25, False), (31, False), (63, False), (63, True), (127, True)]:
        assert kc.WIN[kc.nw_of(m127)] * kc.nmax(K, m127) + 255 < 65536
        assert kc.nmax(K, m127) <= 127 and kc.WIN[kc.nw_of(m127)] <= kc.COPIES_MAX


@pytest.mark.parametrize("name,m127", kc.MANY)
def test_many_windows_many_ranges(golden, emu, name, m127):
    c = golden["cases"][name]
    codes, K = case_codes(c), c["K"] | 1
    W = kc.WIN[kc.nw_of(m127)]
    rec, _, kmers = _stats(emu, name, codes, K, m127)
    assert (rec > 2 * W).all(), rec                                  # three windows or more: a clip pass and a re-staged window in every partition
    assert (kmers > 2 * kc.SLOTS).all(), kmers                       # two levels of the key-range split or more
    # the same reads trimmed (count_ragged): still more than one window and more than one key range everywhere
    rec, _, kmers = _stats(emu, name + " trimmed", codes, K, m127, lens=kc.ragged_lens_for(codes, K))
    assert (rec > W).all() and (kmers > kc.SLOTS).all(), (rec, kmers)


def test_around_the_capacity(golden, emu):
    name, m127, log2_parts = kc.AROUND
    c = golden["cases"][name]
    rec, _, kmers = _stats(emu, name, case_codes(c), c["K"], m127, log2_parts)
    assert int(((kmers > 0.6 * kc.SLOTS) & (kmers <= kc.SLOTS)).sum()) >= 8, kmers
    assert int((rec > kc.WIN[2]).sum()) >= 4, rec


@pytest.mark.parametrize("name", sorted(kc.ONE_WINDOW))
def test_one_window_many_ranges(emu, name):
    codes, K, m127 = kc.one_window_codes(name)
    rec, _, kmers = _stats(emu, name, codes, K, m127)
    assert int(((rec <= kc.WIN[kc.nw_of(m127)]) & (kmers > 2 * kc.SLOTS)).sum()) >= 8, (rec, kmers)


def test_adaptive_dedupe_goes_off(emu):
    """More than DD_FIRST records and fewer than 30 % of DD_FIRST copies in the WHOLE partition: whatever order K1's atomics left the records in,
    the first 4096 hold more than 70 % representatives, and at least a window follows."""
    codes, K, m127 = kc.adaptive_codes("dd_off_k127")
    rec, drec, _ = _stats(emu, "dd_off_k127", codes, K, m127)
    assert (rec >= kc.DD_FIRST + kc.WIN[4]).all(), rec
    assert (rec - drec < (100 - kc.DD_PCT) * kc.DD_FIRST // 100).all(), rec - drec


def test_adaptive_dedupe_stays_on(emu):
    codes, K, m127 = kc.adaptive_codes("dd_on_k127")
    rec, drec, kmers = _stats(emu, "dd_on_k127", codes, K, m127)
    assert (rec >= kc.DD_FIRST + kc.WIN[4]).all(), rec
    assert (2 * drec < rec).all(), (drec, rec)


def _cut(codes, K, m127, log2_parts=kc.LOG2_PARTS):
    """Records of a uniform batch through the host twin of the cutter -> (records, partition of each)."""
    n, L = codes.shape
    recs, tags = api.host_skm_cut(api.pack_reads_uniform(codes), n, L, K, m127, log2_parts, 0, 1)
    return recs, (tags >> np.uint64(8)).astype(np.int64)


def _hdr(recs):
    h = recs[:, 0]
    return ((h >> np.uint64(2)) & np.uint64(0xFFFF)).astype(np.int64), ((h >> np.uint64(1)) & np.uint64(1)).astype(np.int64), (h & np.uint64(1)).astype(np.int64)


@pytest.mark.parametrize("K,m127", kc.HEAVY_KS)
def test_heavy_hitters(emu, tmp_path, K, m127):
    codes, fams = kc.heavy_input(K, m127)
    nw, n_max = kc.nw_of(m127), kc.nmax(K, m127)
    assert codes.shape[1] == K - 1 + n_max
    rec, _, _ = _stats(emu, "heavy", codes, K, m127)
    want, _, _ = kc.oracle_reads(codes, K, 5, str(tmp_path / "o"), m127=m127)
    hot_parts = set()
    for name, f in fams.items():
        recs, parts = _cut(f["heavy"][None, :], K, m127)
        n, hl, hr = _hdr(recs)
        assert len(recs) == 1 and n[0] == n_max and hl[0] == 0 and hr[0] == 0, (name, n, hl, hr)      # one record of nmax k-mers
        # the family's records that hold the hot k-mer are in that partition (its variants' first or last k-mer is another node)
        mrecs, mparts = _cut(f["members"], K, m127)
        mn, _, _ = _hdr(mrecs)
        assert (mparts[mn > 1] == parts[0]).all(), name
        hot = int(parts[0])
        hot_parts.add(hot)
        assert 2 * kc.WIN[nw] + 17 <= rec[hot] <= kc.MAX_PART_RECORDS, (name, rec[hot])
        cov, left, right, single = kc.node_fields(kc.find_node(want, f["key"], nw)[nw])
        assert cov == 255 and not single, (name, cov)
        assert left == f["left"] and right == f["right"], (name, left, right)                           # hot arcs 63, the designed small ones exactly
    assert int((rec > 0).sum()) > len(hot_parts)                                                        # the background: the neighbours are not empty


@pytest.mark.parametrize("K,m127", kc.HEAVY_KS)
def test_heavy_hitters_long_reads(emu, tmp_path, K, m127):
    codes, fams = kc.heavy_input(K, m127, long_reads=True)
    nw, n_max = kc.nw_of(m127), kc.nmax(K, m127)
    assert codes.shape[1] == K - 1 + 3 * n_max
    rec, _, _ = _stats(emu, "heavy, long reads", codes, K, m127)
    want, _, _ = kc.oracle_reads(codes, K, 5, str(tmp_path / "o"), m127=m127)
    for name, f in fams.items():
        recs, parts = _cut(f["heavy"][None, :], K, m127)
        n, hl, hr = _hdr(recs)
        assert n.tolist() == [n_max] * 3 and hl.tolist() == [0, 1, 1] and hr.tolist() == [1, 1, 0], (name, n, hl, hr)
        assert len(set(parts.tolist())) == 1
        assert 2 * kc.WIN[nw] + 17 <= rec[int(parts[0])] <= kc.MAX_PART_RECORDS
        cov, left, right, _ = kc.node_fields(kc.find_node(want, f["key"], nw)[nw])
        assert cov == 255 and left == f["left"] and right == f["right"], (name, cov, left, right)


@pytest.mark.parametrize("K,m127,kind", kc.SINGLE)
def test_single_record_inputs(emu, K, m127, kind):
    codes = kc.single_record_input(K, m127, kind)
    W = kc.WIN[kc.nw_of(m127)]
    assert codes.shape[0] == 2 * W + 17
    rec, drec, _ = _stats(emu, "one record, " + kind, codes, K, m127)
    recs, _ = _cut(codes[:1], K, m127)
    n, hl, hr = _hdr(recs)
    assert len(recs) == 1 and n[0] == kc.nmax(K, m127) and hl[0] == 0 and hr[0] == 0
    assert int((rec > 0).sum()) == 1 and int(rec.max()) == 2 * W + 17 and int(drec.max()) == 1     # whole windows of exact copies: copies = WIN
