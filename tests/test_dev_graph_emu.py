"""The device graph stages (csrc/dev_graph.hpp, csrc/dev_tips.hpp) run on the HostBackend -- the same function objects the HIP
kernels run, on host threads -- against a plain model and against the sequential host stages.  No GPU.  The inputs, the models and the
comparisons of the layouts and of the modulus live in tests/dev_graph_cases.py; tests/test_gpu_dev_graph.py runs the same ones on the HipBackend."""
import ctypes as C

import numpy as np
import pytest

from conftest import case_codes, oracle_records, host_runs
from soapdenovo2_amd import api
import dev_graph_cases as cases
from dev_graph_cases import EMPTY, HostHook


@pytest.mark.parametrize("nw", [2, 4])
@pytest.mark.parametrize("S,n,threads", cases.STATIC_SHAPES)
def test_layout_static_equals_first_come_first_served_probing(nw, S, n, threads):
    """Random keys, several sets, loads up to 99 %: at these loads the last probe cluster wraps around the end of the table in
    most sets, which is the rotated-frame path of layout_static."""
    cases.check_static_vs_fcfs(HostHook(threads), S, n, nw)


def test_layout_static_refuses_a_full_pool():
    cases.check_static_full_pool(HostHook(1))


@pytest.mark.parametrize("nw", [2, 4])
@pytest.mark.parametrize("S,n,threads", cases.STATIC_SHAPES)
def test_the_linked_model_equals_the_probing_model(nw, S, n, threads):
    """fcfs_model_linked (the model of the GPU test's large table, where probing a step at a time would take 10^9 steps) against fcfs_model."""
    rec, per_set = cases.static_case(S, n, nw)
    at = 0
    for c in per_set:
        assert cases.fcfs_model_linked(rec[at:at + c, :nw], S, nw) == cases.fcfs_model(rec[at:at + c, :nw], S, nw)
        at += c


@pytest.mark.parametrize("name,P,a,m", [("t6k_k31", 2, 1, False), ("t8k_k63", 2, 1, True), ("t6k_k127", 3, 1, True)])
def test_layout_static_equals_the_host_replay_on_golden_cases(golden, tmp_path, name, P, a, m):
    """-a pools of the golden cases: the emulated device layout puts every k-mer into the slot the sequential host replay
    (pinned slot by slot on the oracle, tests/test_host_graph.py) puts it."""
    c = golden["cases"][name]
    codes = case_codes(c)
    rec, last, K = oracle_records(codes, c["K"], P, mer127=m, a_gb=a, prefix=str(tmp_path / "o"))
    nw = 4 if m else 2
    rec = rec[np.argsort(rec[:, nw + 1], kind="stable")]                    # replay order: (set, first ordinal)
    slots, sizes = api.host_replay_layout(rec, last, P, mer127=m, a_gb=a)
    S = int(sizes[0])
    assert all(int(x) == S for x in sizes)
    per_set = [int(((rec[:, nw + 1] >> np.uint64(56)) == np.uint64(s)).sum()) for s in range(P)]
    # the image is P * S slots of 24 / 40 bytes: a few GB at -a 1 -- keep the comparison to the occupied slots
    out = np.zeros((P * S, nw + 1), dtype=np.uint64)
    cnt = np.array(per_set, dtype=np.uint64)
    rc = api.lib().pg_host_emu_layout_static(np.ascontiguousarray(rec).ctypes.data, cnt.ctypes.data, P, S, int(m), 4, out.ctypes.data)
    assert rc == 0
    sets = (rec[:, nw + 1] >> np.uint64(56)).astype(np.int64)
    got = out[sets * S + slots.astype(np.int64)]
    assert (got == rec[:, :nw + 1]).all()
    assert int((out[:, 0] != EMPTY).sum()) == len(rec)


# PG_TIP_LIST_ROOM (room): the first listing of the dead ends has room for that many a place instead of slots / 8 + 65536, which no input of
# test size is short of: with 1 every listing of two dead ends or more is short and lists again, with 64 some places are short and some are not
TIP_CASES = [pytest.param(name, threads, places, None, id=f"{name}-{threads}-{places}")
             for threads, places in [(1, 1), (5, 1), (5, 3)]
             for name in ["t6k_k31", "t8k_k63", "t6k_k127", "t5k_k24", "m60k_k63", "d8k_k127", "r8k_k127", "d8k_k63", "m100k_k31"]]
TIP_CASES += [pytest.param(name, 5, places, room, id=f"{name}-5-{places}-room{room}") for room in (1, 64) for places in (1, 3) for name in ["t6k_k31", "d8k_k63"]]


@pytest.mark.parametrize("name,threads,places,room", TIP_CASES)
def test_device_tip_decisions_equal_the_sequential_scan(golden, tmp_path, name, threads, places, room, monkeypatch, capfd):
    """removeSingleTips / removeMinorTips as the device decides them (dev_tips.hpp on the HostBackend: the fixed point over start
    decisions) against the sequential slot-order scan (Graph::tip_scan, pinned on the reference's files by tests/test_host_graph.py):
    the same tips, and afterwards the same counter words in every node.  places = 3: the scans over the sets run "where the set
    lives" with a list and a counter per place that the lead gathers, as in a sharded run (backend.hpp)."""
    monkeypatch.setenv("PG_EMU_PLACES", str(places))
    if room is not None:
        monkeypatch.setenv("PG_TIP_LIST_ROOM", str(room))
        monkeypatch.setenv("PG_HOST_VERBOSE", "1")
    c = golden["cases"][name]
    codes = case_codes(c)
    for run in host_runs(c):
        P, D, a, m = run
        rec, last, K = oracle_records(codes, c["K"], P, D=D, mer127=bool(m), a_gb=a, prefix=str(tmp_path / "o"))
        rec = np.ascontiguousarray(rec)
        out = np.zeros(8, dtype=np.uint64)
        rc = api.lib().pg_host_emu_clip_tips(rec.ctypes.data, len(rec), last.ctypes.data, K, int(bool(m)), P, int(D == 0), a, threads, out.ctypes.data)
        assert rc == 0, api.lib().pg_last_error()
        single_seq, minor_seq, single_dev, minor_dev, diff, rounds, cycles = (int(x) for x in out[:7])
        assert (single_dev, minor_dev) == (single_seq, minor_seq), (name, run)
        assert diff == 0, (name, run, diff)
        assert rounds >= cycles >= 1
    if room is not None:
        assert "dead ends listed again" in capfd.readouterr().err


def _growable_vs_replay(rec, last, P, m, threads):
    return cases.growable_vs_replay(HostHook(threads), rec, last, P, m)


@pytest.mark.parametrize("name,P,m", [("t6k_k31", 7, False), ("t8k_k63", 3, True), ("m60k_k63", 8, False), ("t6k_k127", 3, True), ("m100k_k31", 2, False)])
def test_layout_growable_equals_the_host_replay(golden, tmp_path, name, P, m):
    """The growable (-a 0) sets' layout as the device computes it -- the in-place rehash as a fixed point over insertion times,
    dev_rehash.hpp on the HostBackend -- puts every k-mer into the slot the sequential host replay puts it (which is pinned slot by
    slot on the oracle and through the golden files on the reference)."""
    c = golden["cases"][name]
    codes = case_codes(c)
    rec, last, K = oracle_records(codes, c["K"], P, mer127=m, prefix=str(tmp_path / "o"))
    rounds = _growable_vs_replay(rec, last, P, m, threads=4)
    assert int(rounds.max()) >= 2


@pytest.mark.parametrize("blind_max,dense_min", cases.THRESHOLD_SETTINGS)
def test_layout_growable_random_keys_and_the_trailing_duplicate(blind_max, dense_min, monkeypatch):
    """Random keys (no genome structure), set sizes right at the growth thresholds, with and without a duplicate put behind the
    last new key (newhash.c:477 tests the growth before it probes).  blind_max: up to which size the fixed point's rounds are
    launched eight at a time without a read-back (dev_rehash.hpp; default 2^18 keys: all of these sets; 0: none; 2000: some sizes of a set).
    dense_min: from which size the first round runs over a list of the cluster starts whose length stays on the device (default 2^18
    keys: none of these sets; 1: every size that is not launched blind; 0: never)."""
    cases.set_thresholds(monkeypatch, blind_max, dense_min)
    seen = 0
    for n, trailing, rec, last in cases.threshold_sets():
        _growable_vs_replay(rec, last, 1, False, threads=3)
        seen += 1
    assert seen == 2 * len(cases.THRESHOLD_SIZES)


def test_layout_growable_random_keys_four_words():
    """The same with four-word keys (the 127-mer flavour: other initial size, chained 32-bit modulus for the home slot), several
    sets of different sizes in one call."""
    rec, last, P = cases.four_word_sets()
    rounds = _growable_vs_replay(rec, last, P, True, threads=4)
    assert int(rounds[0]) > int(rounds[1])


@pytest.mark.parametrize("mer127", [False, True])
def test_home_slot_by_reciprocal_equals_the_reference_modulus(mer127):
    """key mod size through the precomputed reciprocal (graph_lookup.hpp: rem128) against Python's integers: the exact 128-bit
    modulus of the 63-mer build, and the 127-mer build's 32-bit chunks folded in 64-bit arithmetic -- whose `t << 32` overflows
    once a set is larger than 2^32 slots (newhash.c:36-57); sizes from 1 to 2^63 - 1, keys incl. the extremes."""
    cases.check_home_slots(HostHook(), mer127, every=lambda size: 7 if size > 5 else 1)


def test_layout_growable_fuzz_over_thresholds_and_skewed_homes(monkeypatch):
    """Many small random sets against the host replay with the fixed point's three thresholds drawn at random (rounds launched blind, first
    round over a list of the cluster starts, the re-sweep list by appends or by a prefix sum), both key widths, one to four host threads, and every
    third set with small numbers for keys: their homes crowd (runs of consecutive slots), clusters are thousands of keys long -- the heap behind the
    sweep's six registers -- and wrap around the end of the table."""
    for seed in cases.FUZZ_SEEDS:
        d = cases.fuzz_draw(seed)
        cases.set_thresholds(monkeypatch, d["blind_max"], d["dense_min"], d["list_shift"])
        _growable_vs_replay(d["rec"], d["last"], 1, d["four"], threads=d["threads"])
