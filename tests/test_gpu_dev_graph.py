"""The k-mer-set layouts, the modulus by reciprocal and the append primitive as the product runs them -- the HipBackend instantiations on a
GPU, through pg_device_emu_* -- against the models tests/test_dev_graph_emu.py holds the HostBackend to (tests/dev_graph_cases.py: the same
inputs, seeds and comparisons).  What the host threads cannot show is what differs here: 10^5 concurrent lanes, rocPRIM's multi-block sort
and scans, relaxed device atomics across workgroups, launch order on a stream standing in for a join of threads.  All comparisons exact."""
import numpy as np
import pytest

from conftest import case_codes, oracle_records
import dev_graph_cases as cases
from dev_graph_cases import DeviceHook

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every pg_device_emu_* call allocates its blocks and frees them all.  Unpinned, the device arena gives its memory back each time and
    retires the address range it had (csrc/arena.cpp: trim); some hundreds of calls later a process has no range left and the arena
    switches itself off for the tests that follow.  A caller that allocates and frees in a loop pins the device around the loop
    (include/soapdenovo2_amd.h), and so does this module."""
    from soapdenovo2_amd import api
    with api.arena_pinned(0):
        yield


# ---- layout_static against first come, first served ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [2, 4])
@pytest.mark.parametrize("S,n", [(S, n) for S, n, _ in cases.STATIC_SHAPES])
def test_layout_static_equals_first_come_first_served_probing(nw, S, n):
    """Loads up to 99 % in tables of a few hundred slots, three sets of which one is empty, a quarter of set 0's homes within 5 slots of the
    table's end: the last cluster wraps (asserted), which is the rotated-frame path of layout_static."""
    cases.check_static_vs_fcfs(DeviceHook(), S, n, nw)


def test_layout_static_refuses_a_full_pool():
    cases.check_static_full_pool(DeviceHook())


@pytest.mark.parametrize("nw", [2, 4])
def test_layout_static_many_blocks(nw):
    """S = 262147 with 200000 keys in set 0 and 100000 in set 2: the sort and the scans run over many blocks, and the cluster at the end of
    set 0's table is 50000 keys long and wraps."""
    S, n = cases.STATIC_LARGE
    cases.check_static_vs_fcfs(DeviceHook(), S, n, nw, model=cases.fcfs_model_linked)


# ---- layout_growable against the sequential host replay -----------------------------------------------------------------------------------
@pytest.mark.parametrize("blind_max,dense_min", cases.THRESHOLD_SETTINGS)
def test_layout_growable_random_keys_and_the_trailing_duplicate(blind_max, dense_min, monkeypatch):
    """Set sizes right at the growth thresholds, with and without the trailing duplicate put, under the CPU test's seven settings of
    (PG_RH_BLIND_MAX, PG_RH_DENSE_MIN): blind rounds, read-back rounds and the dense first round over a list with a device-side length."""
    cases.set_thresholds(monkeypatch, blind_max, dense_min)
    seen = 0
    for n, trailing, rec, last in cases.threshold_sets():
        cases.growable_vs_replay(DeviceHook(), rec, last, 1, False)
        seen += 1
    assert seen == 2 * len(cases.THRESHOLD_SIZES)


def test_layout_growable_random_keys_four_words():
    """Four-word keys, three sets of 30000 / 7 / 12345 keys in one call: the two layout lanes run side by side on streams of their own."""
    rec, last, P = cases.four_word_sets()
    rounds = cases.growable_vs_replay(DeviceHook(), rec, last, P, True)
    assert int(rounds[0]) > int(rounds[1])


@pytest.mark.parametrize("group", range(6))
def test_layout_growable_fuzz_over_thresholds_and_skewed_homes(group, monkeypatch):
    """The 120 fuzz seeds of the CPU test, 20 a group, with the same per-seed draws of the three thresholds, the key width and the keys
    (every third set: small numbers, crowded homes, clusters thousands of keys long that wrap)."""
    seeds = list(cases.FUZZ_SEEDS)[20 * group:20 * group + 20]
    assert len(seeds) == 20
    for seed in seeds:
        d = cases.fuzz_draw(seed)
        cases.set_thresholds(monkeypatch, d["blind_max"], d["dense_min"], d["list_shift"])
        cases.growable_vs_replay(DeviceHook(), d["rec"], d["last"], 1, d["four"])


@pytest.mark.parametrize("nw", [2, 4])
def test_layout_growable_above_the_default_thresholds(nw, monkeypatch):
    """Nothing set in the environment: two sets of 300000 keys (> 2^18), random keys and small numbers, side by side on the two lanes.  The
    defaults take the read-back rounds, the dense first round and both list forms at the last sizes, and the blind rounds below."""
    for name in ("PG_RH_BLIND_MAX", "PG_RH_DENSE_MIN", "PG_RH_LIST_SHIFT", "SOAPDENOVO2_AMD_LAYOUT_LANES"):
        monkeypatch.delenv(name, raising=False)
    rec, last, P = cases.large_sets(nw)
    rounds = cases.growable_vs_replay(DeviceHook(), rec, last, P, nw == 4)
    assert all(int(r) >= 2 for r in rounds), rounds


@pytest.mark.parametrize("name,P,m", [("m60k_k63", 8, False), ("t6k_k127", 3, True)])
def test_layout_growable_equals_the_host_replay_on_golden_cases(golden, tmp_path, name, P, m, monkeypatch):
    """Genome k-mer sets (two of the CPU test's golden cases), every round read back."""
    monkeypatch.setenv("PG_RH_BLIND_MAX", "0")
    c = golden["cases"][name]
    codes = case_codes(c)
    rec, last, K = oracle_records(codes, c["K"], P, mer127=m, prefix=str(tmp_path / "o"))
    rounds = cases.growable_vs_replay(DeviceHook(), rec, last, P, m)
    assert int(rounds.max()) >= 2


# ---- key mod size ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mer127", [False, True])
def test_home_slot_by_reciprocal_equals_the_reference_modulus(mer127):
    """The device's own arithmetic (__umul64hi where the host has unsigned __int128) against Python's integers, every key at every size:
    sizes up to 2^63 - 1, where the 127-mer chunk fold overflows by design."""
    cases.check_home_slots(DeviceHook(), mer127)


# ---- the append primitive -------------------------------------------------------------------------------------------------------------------
_flags = {}


def _append_flags(n, pattern):
    if (n, pattern) not in _flags:
        _flags.clear()                                   # (one pattern of 6 M flags at a time)
        f = cases.append_flags(n, pattern)
        f.setflags(write=False)
        _flags[(n, pattern)] = f
    return _flags[(n, pattern)]


@pytest.mark.parametrize("which", cases.APPEND_CAPS)
@pytest.mark.parametrize("n,pattern", cases.APPEND_SHAPES)
def test_append_lists_every_hit_once_and_counts_them_all(n, pattern, which):
    """be_append_kernel (LDS buffer, one returned atomic per ~1000 hits; no host twin): one trip and ragged workgroups, the grid's full
    width, and six trips and a ragged seventh -- with all flags set `held` reaches the buffer's 1280 entries and the loop flushes midway.
    Caps around the number of hits: it counts them all and writes only below cap."""
    flags = _append_flags(n, pattern)
    cap = cases.append_cap(int(flags.sum()), which)
    if cap is None:                                      # hits - 1 where nothing is hit: there is no such list (cap 0 and cap 1 are cases of their own)
        cap = 0
    cases.check_append(DeviceHook(), flags, cap)
