"""The counting kernel of the partition engine (K2: skm_count_kernel, csrc/partition_kernels.hip) on partitions as large as those of a
multi-million-read input, at test size (run with -m gpu on an MI355X): PG_LOG2_PARTS=4 leaves 16 partitions, so a few thousand reads take
several windows a partition (the clip of the counter halves between them, re-staged windows, later windows off the chunk table), split the
key range several levels deep (one window kept for the other ranges, or several counted again), switch the four-word flavour's search for
copies off or keep it on, and heavy-hitter reads add whole windows of copies to one node's counters (tests/k2_partition_cases.py builds the
inputs, tests/test_k2_partition_cases_host.py holds them to what they claim).  The same heavy hitters go through the global-set engine,
whose packed saturating counters meet the same contention.

The CPU oracle alone decides what is right, bit for bit: the whole export record (key words, all eight arc counters, coverage, the single /
linear / deleted flags, set id and first ordinal), the per-set `last` array, and the 255 rows of the histogram against the oracle's .kmerFreq.
A pass that reports a failure (a partition that could not be split, a chunk list outgrown) raises in finalize and fails the test."""
import numpy as np
import pytest

import k2_partition_cases as kc
from conftest import case_codes, case_config, case_tag, md5_file, md5_gz_text
from test_gpu_pregraph import PARALLEL_PARSE, _run_cli, _sharded_records, _sorted

pytestmark = pytest.mark.gpu

_ORACLE = {}


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """oracle(tag, make_reads, K, P, D, m127) -> (records, last, .kmerFreq rows, reads, lens): once a module for each input and setting."""
    def get(tag, make, K, P, D, m127):
        key = (tag, K, P, D, m127)
        if key not in _ORACLE:
            reads, lens = make()
            prefix = str(tmp_path_factory.mktemp("oracle") / "o")
            _ORACLE[key] = kc.oracle_reads(reads, K, P, prefix, D=D, m127=m127, lens=lens) + (reads, lens)
        return _ORACLE[key]
    return get


def _count(monkeypatch, batches, K, P, m127, D, engine=2, log2_parts=kc.LOG2_PARTS, log2_slots=20):
    """batches: [(reads [n, L], lens or None)] counted in the order given, ordinals as if they had come first to last -> (records, hist, last)."""
    import torch
    from soapdenovo2_amd import api
    if log2_parts is not None:
        monkeypatch.setenv("PG_LOG2_PARTS", str(log2_parts))
    else:
        monkeypatch.delenv("PG_LOG2_PARTS", raising=False)
    kc_ = api.KmerCounter(K, n_sets=P, mer127=m127, log2_slots=log2_slots, engine=engine)
    if engine == 2 and log2_parts is not None:
        assert kc_.stats()["parts_or_slots"] == 1 << log2_parts              # the hook is there: a dropped one would pass on 256 small partitions
    base, jobs = 0, []
    for reads, lens in batches:
        n, L = reads.shape
        kmers = n * (L - K + 1) if lens is None else int((lens.astype(np.int64) - K + 1).sum())
        jobs.append((reads, lens, base, kmers))
        base += kmers
    for reads, lens, ord_base, kmers in jobs[::-1]:                          # last batch first: the first-occurrence ordinal must not care
        if lens is None:
            packed = torch.from_numpy(api.pack_reads_uniform(reads).view(np.int64)).cuda()
            kc_.count_uniform(packed, reads.shape[0], reads.shape[1], ord_base=ord_base)
        else:
            words, off, kb = api.pack_reads_ragged([reads[i, :lens[i]] for i in range(len(lens))], K)
            assert int(kb[-1]) == kmers
            kc_.count_ragged(torch.from_numpy(words.view(np.int64)).cuda(), torch.from_numpy(off.view(np.int64)).cuda(),
                             torch.from_numpy(kb.view(np.int64)).cuda(), len(lens), kmers, ord_base=ord_base)
    hist, last = kc_.finalize(D)
    rec = kc_.export()
    kc_.close()
    return rec, hist, last


def _split(reads, lens, parts):
    b = np.linspace(0, reads.shape[0], parts + 1).astype(int)
    return [(reads[lo:hi], None if lens is None else lens[lo:hi]) for lo, hi in zip(b[:-1], b[1:])]


def _same(got, want, nw):
    rec, hist, last = got
    want_rec, want_last, freq = want[:3]
    assert rec.shape == want_rec.shape
    a, b = _sorted(rec, nw), _sorted(want_rec, nw)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert len(bad) == 0, (len(bad), [[hex(int(x)) for x in a[bad[0]]], [hex(int(x)) for x in b[bad[0]]]])
    assert (last == want_last).all()
    assert [int(x) for x in hist[1:]] == freq


def _golden_reads(golden, name):
    return lambda: (case_codes(golden["cases"][name]), None)


UNIFORM = ([("many", name, m, kc.LOG2_PARTS, 0) for name, m in kc.MANY] + [("many", "t6k_k31", False, kc.LOG2_PARTS, 1), ("many", "t6k_k127", True, kc.LOG2_PARTS, 1)]
           + [("around", kc.AROUND[0], kc.AROUND[1], kc.AROUND[2], 0)]
           + [("one_window", name, kc.ONE_WINDOW[name][1], kc.LOG2_PARTS, D) for name, D in (("w1_k63", 0), ("w1_k63", 1), ("w1_k127", 0))]
           + [("adaptive", name, True, kc.LOG2_PARTS, 0) for name in sorted(kc.ADAPTIVE)])


@pytest.mark.parametrize("kind,name,m127,log2_parts,D", UNIFORM)
def test_large_partitions_match_oracle(golden, oracle, monkeypatch, kind, name, m127, log2_parts, D):
    """Several windows and key ranges a partition, a single window under several ranges, partitions around the set's capacity, the search
    for copies switched off and kept on: uniform batches, three of them, last first."""
    if kind in ("many", "around"):
        make, K = _golden_reads(golden, name), golden["cases"][name]["K"] | 1
    elif kind == "one_window":
        make, K = (lambda: (kc.one_window_codes(name)[0], None)), kc.ONE_WINDOW[name][0]
    else:
        make, K = (lambda: (kc.adaptive_codes(name)[0], None)), 127
    P = 5
    want = oracle(name, make, K, P, D, m127)
    got = _count(monkeypatch, _split(want[3], None, 3), K, P, m127, D, log2_parts=log2_parts, log2_slots=23 if kind == "adaptive" else 20)
    _same(got, want, kc.nw_of(m127))


@pytest.mark.parametrize("name,m127", kc.MANY)
def test_large_partitions_of_trimmed_reads_match_oracle(golden, oracle, monkeypatch, name, m127):
    """The many-window inputs trimmed to random lengths in [K + 1, L], through the ragged cutter, in two batches."""
    K = golden["cases"][name]["K"] | 1

    def make():
        codes = case_codes(golden["cases"][name])
        return codes, kc.ragged_lens_for(codes, K)
    want = oracle(name + " trimmed", make, K, 5, 0, m127)
    got = _count(monkeypatch, _split(want[3], want[4], 2), K, 5, m127, 0)
    _same(got, want, kc.nw_of(m127))


def _heavy_both(K, m127):
    """The mixed heavy-hitter input and its long-read variant as one ragged set for the oracle: two uniform batches for the device."""
    short, _ = kc.heavy_input(K, m127)
    long_, _ = kc.heavy_input(K, m127, long_reads=True)
    reads = np.zeros((len(short) + len(long_), long_.shape[1]), dtype=np.uint8)
    reads[:len(short), :short.shape[1]] = short
    reads[len(short):] = long_
    lens = np.array([short.shape[1]] * len(short) + [long_.shape[1]] * len(long_), dtype=np.int32)
    return reads, lens


@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("log2_parts", [None, kc.LOG2_PARTS])
@pytest.mark.parametrize("engine", [1, 2])
@pytest.mark.parametrize("K,m127", kc.HEAVY_KS)
def test_heavy_hitters_match_oracle(oracle, monkeypatch, K, m127, engine, log2_parts, D):
    """Four hot nodes (poly-A, poly-C, (AT)^n, (CG)^n: a low and a high counter half of either word) fed by windows of up to 512 copies of a
    record of nmax k-mers, small designed arcs beside the saturated ones, then the poly-A and (AT)^n families again at three records a read
    (a second uniform batch of its own length): both engines, the default partition count and 16 partitions, with and without the -d filter."""
    want = oracle("heavy", lambda: _heavy_both(K, m127), K, 5, D, m127)
    reads, lens = want[3], want[4]
    n_short, L_short = int((lens == lens.min()).sum()), int(lens.min())
    batches = [(np.ascontiguousarray(reads[:n_short, :L_short]), None), (np.ascontiguousarray(reads[n_short:]), None)]
    # (Without the hook the record pool is as many sub-pools as partitions, up to 1024, and a partition draws its chunks from one of them: at
    #  log2_slots = 20 that is 22 chunks, 2816 records a batch -- the poly-A partition takes 5200 from the long reads alone and the pass would end
    #  with "record pool exhausted", loudly, as it is meant to.  A context sized for 2^24 k-mers has 170 chunks a sub-pool, room for all four families.)
    got = _count(monkeypatch, batches, K, 5, m127, D, engine=engine, log2_parts=log2_parts, log2_slots=24 if engine == 2 and log2_parts is None else 20)
    _same(got, want, kc.nw_of(m127))
    # (the comparison above covers it; spelled out for the node the input was made for)
    nw = kc.nw_of(m127)
    fams, twice = kc.heavy_input(K, m127)[1], kc.heavy_input(K, m127, long_reads=True)[1]
    if D == 0:
        for name, f in fams.items():
            times = 2 if name in twice else 1                            # (the long reads bring that family's variants once more)
            cov, left, right, _ = kc.node_fields(kc.find_node(got[0], f["key"], nw)[nw])
            assert cov == 255, (name, cov)
            assert left == [min(63, times * x) for x in f["left"]] and right == [min(63, times * x) for x in f["right"]], (name, left, right)


@pytest.mark.parametrize("log2_parts", [None, kc.LOG2_PARTS])
@pytest.mark.parametrize("engine", [1, 2])
@pytest.mark.parametrize("K,m127,kind", kc.SINGLE)
def test_windows_of_one_record_match_oracle(oracle, monkeypatch, K, m127, kind, engine, log2_parts):
    """2 WIN + 17 copies of one read that is one record of nmax k-mers and nothing else: two windows of WIN exact copies (copies - 1 = 511 and
    n = 127 at K = 31, the full widths of the header's two fields), a third of 17."""
    want = oracle("single " + kind, lambda: (kc.single_record_input(K, m127, kind), None), K, 3, 0, m127)
    got = _count(monkeypatch, [(want[3], None)], K, 3, m127, 0, engine=engine, log2_parts=log2_parts)
    _same(got, want, kc.nw_of(m127))


@pytest.mark.parametrize("tag,n_ranks", [("t8k_k63", 3), ("heavy_k31", 2)])
def test_sharded_large_partitions_match_oracle(golden, oracle, monkeypatch, tag, n_ranks):
    """Pass 1 over several ranks with 16 partition ids: three ranks receive 6 / 5 / 5 of them (every context holds ids nobody sends to it);
    of two ranks one receives a heavy hitter's whole partition."""
    monkeypatch.setenv("PG_LOG2_PARTS", str(kc.LOG2_PARTS))
    if tag == "t8k_k63":
        K, P, m127 = 63, 5, False
        want = oracle(tag, _golden_reads(golden, tag), K, P, 0, m127)
    else:
        K, P, m127 = 31, 5, False
        want = oracle("heavy short", lambda: (kc.heavy_input(K, m127)[0], None), K, P, 0, m127)
    out = _sharded_records(want[3], K, P, n_ranks, mer127=m127)
    got = np.concatenate([o[0] for o in out])
    _same((got, out[0][1], np.maximum.reduce([o[2] for o in out])), want, 2)
    assert all(o[3]["recv_records"] > 0 for o in out)


@pytest.mark.parametrize("form", ["default", "SOAPDENOVO2_AMD_P2_PARTITIONED"])
@pytest.mark.parametrize("name", ["t6k_k31", "t8k_k63", "t6k_k127"])
def test_cli_with_16_partitions_writes_the_reference_files(golden, tmp_path, name, form):
    """The executable with 16 partitions: pass 1 stays on the partition engine (no second count through the global set) and, with pass 2's lookups
    through the partition engine as well (skm_answer_kernel has its own key-range split), the five files stay the reference's."""
    c = golden["cases"][name]
    cfg = case_config(c, str(tmp_path), name)
    env = dict(PARALLEL_PARSE, PG_HOST_VERBOSE="1", PG_LOG2_PARTS=str(kc.LOG2_PARTS))
    if form != "default":
        env[form] = "1"
    for run in c["runs"]:
        P, D, a, m = run
        t = case_tag(name, run)
        pre = str(tmp_path / t)
        log = _run_cli(cfg, c["K"], pre, P, D, a, m, extra_env=env)
        assert "counting again with the global k-mer set" not in log, t
        if form != "default":
            assert "through the partition engine" in log, t
        want = golden["md5"][t]
        assert md5_file(pre + ".kmerFreq") == want["kmerFreq"], t
        assert md5_file(pre + ".preGraphBasic") == want["preGraphBasic"], t
        assert md5_file(pre + ".vertex") == want["vertex"], t
        assert md5_gz_text(pre + ".edge.gz") == want["edge"], t
        assert md5_file(pre + ".preArc") == want["preArc"], t
