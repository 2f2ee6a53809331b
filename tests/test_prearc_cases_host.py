"""The designed pre-arc cases of tests/prearc_cases.py held to what they claim, and the model of tests/prearc_model.py held to the reference's own
files -- without the library and without a GPU.  tests/test_gpu_prearc.py runs the same cases through the device path; what is shown here is that
each case reaches the path it names (a sequential linear-probing simulation of the table: probe runs, the wrap, the load, the overflow) and that
its expected rows change under the mistake it names (the MODEL is broken the same way; no broken kernel is ever run)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import prearc_cases as cases
import prearc_model as model

COMMITTED = ["t6k_k31_p1_d0_a0_63", "t6k_k31_p8_d0_a0_63", "t8k_k63_p2_d0_a0_63"]


def _tables(c):
    """every lane's table simulated: [(pairs, slots, longest run, crossed the end, lost)]"""
    out = []
    for l in range(c.lanes):
        keys = c.lane_keys(l)
        out.append((keys,) + cases.simulate(keys, c.room))
    return out


def _rows(c, **wrong):
    return model.fold(c.triples(), **wrong)


# ---- the model against the reference's bytes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", COMMITTED)
def test_model_reproduces_the_committed_prearc_files(tag):
    """Triples read back from a reference .preArc -- a line's targets with descending made-up first meetings, each repeated by its multiplicity,
    shuffled -- folded by the model and printed: the reference's own bytes.  An ascending order within a line does not give them."""
    text = open(os.path.join(GOLDEN, tag + ".preArc")).read()
    lists = model.parse_prearc(text)
    assert len(lists) > 100 and max(len(t) for _, t in lists) >= 2 and max(m for _, t in lists for _, m in t) >= 2
    triples = model.triples_of_prearc(lists, seed=3)
    assert len(triples) == sum(m for _, t in lists for _, m in t)
    rows = model.fold(triples)
    assert model.prearc_lines(rows) == text
    f, t, s = (np.array(x, dtype=np.uint64) for x in zip(*triples))
    assert model.prearc_lines(model.fold_np(f, t, s).tolist()) == text
    assert model.prearc_lines(model.fold(triples, wrong_ascending=True)) != text


@pytest.mark.parametrize("name", [n for n in cases.SMALL if n not in cases.OVER])
def test_numpy_model_equals_the_integer_model(name):
    c = cases.small(name)
    assert np.array_equal(model.fold_np(c.frm, c.to, c.seq), model.as_rows(_rows(c)))


# ---- every case reaches what it names ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.SMALL))
def test_case_is_what_it_claims(name):
    c = cases.small(name)
    assert c.mistake and c.room >= 2 and c.room & (c.room - 1) == 0 and c.lanes >= 1
    assert int(c.seq.max()) <= cases.SEQ_MAX and not ((c.frm == 0) & (c.to == 0)).any()
    tabs = _tables(c)
    lost = sum(t[4] for t in tabs)
    assert lost == c.overflow
    # first meetings of one `from` differ: the file order is decided
    first = {}
    for f, t, s in c.triples():
        first[(f, t)] = min(s, first.get((f, t), s))
    per_from = {}
    for (f, t), s in first.items():
        assert per_from.setdefault((f, s), t) == t, (name, f, s)
    cl = c.claims
    if "distinct" in cl:
        assert len(first) == cl["distinct"]
    if "longest" in cl:
        assert max(t[2] for t in tabs) == cl["longest"]
    if "longest_at_least" in cl:
        assert max(t[2] for t in tabs) >= cl["longest_at_least"]
    if "crosses" in cl:
        assert any(t[3] for t in tabs) == cl["crosses"]
    if "load" in cl:
        assert len(first) / c.room == cl["load"]
    if cl.get("same_home"):
        assert len({cases.home(f, t, c.room) for f, t in first}) == 1
    if cl.get("one_from"):
        assert len({f for f, _ in first}) == 1
    if not c.overflow:
        rows = _rows(c)
        assert sum(r[2] for r in rows) == len(c.frm) and len(rows) == len(first)


def test_one_home_is_whole_waves_on_one_entry():
    c = cases.small("one_home")
    f = c.frm.reshape(-1, 64); t = c.to.reshape(-1, 64); s = c.seq.reshape(-1, 64)
    assert len(f) == 200 and (f == f[:, :1]).all() and (t == t[:, :1]).all()
    where = s.argmin(axis=1)
    assert len(set(where.tolist())) > 30 and 0 < (where == 0).sum() + 1 < 20          # the minimum sits anywhere among the 64


def test_wraps_run_on_from_the_last_entries():
    c = cases.small("wraps_room256")
    homes = sorted(cases.home(f, t, 256) for f, t in c.lane_keys(0))
    assert set(homes) <= {252, 253, 254, 255} and len(homes) == 16
    keys, where, _, crossed, lost = _tables(c)[0]
    assert crossed and not lost and sorted(where) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 252, 253, 254, 255]
    c2 = cases.small("wraps_room2")
    assert [cases.home(f, t, 2) for f, t in c2.lane_keys(0)] == [1, 1]
    assert sorted(_tables(c2)[0][1]) == [0, 1]


def test_full_and_over():
    c = cases.small("full")
    assert sorted(_tables(c)[0][1]) == list(range(256))
    assert 1 <= np.bincount(model.as_rows(_rows(c))[:, 2]).nonzero()[0].min() and model.as_rows(_rows(c))[:, 2].max() == 3
    for name, room, d in (("over_room256_d1", 256, 1), ("over_room256_d7", 256, 7), ("over_room2_d1", 2, 1)):
        c = cases.small(name)
        assert c.room == room and c.overflow == d and len(set(zip(c.frm.tolist(), c.to.tolist()))) == len(c.frm) == room + d     # each pair met ONCE


def test_hot_pair():
    c = cases.small("hot")
    hot = (c.frm == 77) & (c.to == 4242)
    assert hot.sum() == 100000 > 1 << 16
    at = int(np.flatnonzero(hot)[c.seq[hot].argmin()])
    assert len(c.frm) // 3 < at < 2 * len(c.frm) // 3
    assert (77, 4242, 100000) in _rows(c)
    assert len(set(zip(c.frm[~hot].tolist(), c.to[~hot].tolist()))) == (~hot).sum() == 1000


@pytest.mark.parametrize("which,lo,hi", [("low16", 0, 16), ("16to31", 16, 32), ("32up", 32, 64), ("48up", 48, 64)])
def test_first_bits_differ_only_where_they_say(which, lo, hi):
    c = cases.small("first_bits_" + which)
    first = {}
    for f, t, s in c.triples():
        first[t] = min(s, first.get(t, s))
    v = list(first.values())
    mask = ((1 << hi) - 1) & ~((1 << lo) - 1)
    assert len({x & ~mask for x in v}) == 1 and len({x & mask for x in v}) == len(v) == 48
    if which == "48up":
        assert max(v) == cases.SEQ_MAX


def test_ids_case():
    c = cases.small("ids")
    pairs = set(zip(c.frm.tolist(), c.to.tolist()))
    BIG = 0xFFFFFFFE
    assert {(BIG, BIG), (1, 1), (1, 2), (2, 1), (BIG, 1), (1, BIG)} <= pairs and min(c.frm) == 1
    assert sum(1 for f, t in pairs if (t, f) in pairs and f != t) >= 8 and sum(1 for f, t in pairs if f == t) >= 3
    per = np.unique(c.frm, return_counts=False)
    assert sum(1 for f, _ in pairs if f == c.claims["busy"]) == 500
    assert sum(1 for f in per.tolist() if sum(1 for g, _ in pairs if g == f) == 1) >= 400 and (per >= 1 << 31).sum() > 50 and (per < 1 << 31).sum() > 50


@pytest.mark.parametrize("L", [2, 3, 8])
@pytest.mark.parametrize("lonely", [False, True])
def test_lanes_case(L, lonely):
    c = cases.small("lanes%d_%s" % (L, "lonely" if lonely else "mixed"))
    assert c.lanes == L and len(c.frm) % L == 0
    on = {}
    for i, (f, t, s) in enumerate(c.triples()):
        on.setdefault((f, t), {}).setdefault(i % L, []).append(s)
    n_lanes = {k: len(v) for k, v in on.items()}
    assert 1 in n_lanes.values() and L in n_lanes.values()
    if min(L - 1, L - 1 if lonely else L) >= 2 and c.claims["n_some"]:
        assert any(1 < n < L for n in n_lanes.values())
    # the earliest meeting of every pair on several lanes lies on the last lane that has it -- never on the first
    for k, v in on.items():
        if len(v) > 1:
            assert min(v, key=lambda l: min(v[l])) == max(v) > min(v)
    top = max(on)
    assert top == c.claims["top"]
    if lonely:                                             # the last lane's table holds one pair only, one every lane has; the merged array ends inside a pair
        assert c.lane_keys(L - 1) == [top] and n_lanes[top] == L
    else:                                                  # the merged array's last entry is a head
        assert n_lanes[top] == 1
    assert len(_rows(c)) == len(on) < sum(n_lanes.values())


@pytest.mark.parametrize("which", ["count", "fold"])
def test_second_trip_cases_are_large_enough(which):
    c = cases.second_trip(which)
    key = (c.frm.astype(np.uint64) << np.uint64(32)) | c.to
    u = np.unique(key)
    assert len(u) == c.claims["distinct"]
    assert c.room > 2048 * 256 and len(u) / c.room > 0.5
    if which == "fold":
        assert len(u) > 8192 * 256
    occ, longest = cases.simulate_np(u >> np.uint64(32), u & np.uint64(0xFFFFFFFF), c.room)
    assert int(occ.sum()) == len(u) and longest > 8
    assert int(np.flatnonzero(occ).max()) >= 2048 * 256                 # entries of the second trip are occupied
    rows = model.fold_np(c.frm, c.to, c.seq)
    assert len(rows) == len(u) and int(rows[:, 2].sum()) == len(c.frm) and (np.diff(rows[:, 0].astype(np.int64)) >= 0).all()
    assert len(np.unique(c.seq)) == len(c.seq)


def test_the_set_of_occupied_entries_does_not_depend_on_the_order():
    rng = np.random.RandomState(5)
    for name in ("one_home", "wraps_room256", "full", "ids", "hot"):
        c = cases.small(name)
        keys = c.lane_keys(0)
        want = sorted(cases.simulate(keys, c.room)[0])
        for _ in range(3):
            again = [keys[i] for i in rng.permutation(len(keys))]
            assert sorted(cases.simulate(again, c.room)[0]) == want
        occ, _ = cases.simulate_np([k[0] for k in keys], [k[1] for k in keys], c.room)
        assert np.flatnonzero(occ).tolist() == want


# ---- every case class tells its mistake from the right answer -----------------------------------------------------------------------------------
def _rows_of_placed(c, **wrong):
    """the model over the triples whose pair found an entry in a table simulated with a mistake, and the triples that did not"""
    keys = c.lane_keys(0)
    where = cases.simulate(keys, c.room, **wrong)[0]
    placed = {k for k, w in zip(keys, where) if w is not None}
    kept = [(f, t, s) for f, t, s in c.triples() if (f, t) in placed]
    return model.fold(kept), len(c.frm) - len(kept)


def test_mistake_a_wrong_wrap_mask_changes_the_wrap_cases():
    for name in ("wraps_room256", "wraps_room2"):
        c = cases.small(name)
        rows, lost = _rows_of_placed(c, wrong_no_wrap=True)
        assert lost > 0 and rows != _rows(c)
    c = cases.small("hot")                                # (a case that does not wrap cannot tell)
    assert _rows_of_placed(c, wrong_no_wrap=True) == (_rows(c), 0)


def test_mistake_a_table_held_full_one_entry_early_changes_full():
    c = cases.small("full")
    rows, lost = _rows_of_placed(c, wrong_steps=c.room - 1)
    assert lost > 0 and rows != _rows(c)


def test_mistake_a_wrong_wrap_mask_changes_the_overflow_count():
    for name in cases.OVER:
        c = cases.small(name)
        assert cases.simulate(c.lane_keys(0), c.room)[3] == c.overflow > 0
        assert cases.simulate(c.lane_keys(0), c.room, wrong_no_wrap=True)[3] != c.overflow or c.room == 2     # (runs lost at the table's end are counted too)


def test_mistake_a_multiplicity_of_16_bits_changes_hot():
    c = cases.small("hot")
    assert _rows(c, wrong_mult_bits=16) != _rows(c)
    assert _rows(cases.small("ids"), wrong_mult_bits=16) == _rows(cases.small("ids"))


def test_mistake_an_ascending_order_changes_every_case_with_two_targets_a_source():
    for name in ("first_bits_low16", "first_bits_16to31", "first_bits_32up", "first_bits_48up", "ids", "one_home", "lanes3_mixed", "hot"):
        c = cases.small(name)
        if name in ("one_home", "lanes3_mixed", "hot") and len({r[0] for r in _rows(c)}) == len(_rows(c)):
            continue
        assert _rows(c, wrong_ascending=True) != _rows(c), name


def test_mistake_a_first_meeting_of_too_few_bits_changes_the_first_bits_cases():
    for name, bits, changes in (("first_bits_16to31", 16, True), ("first_bits_32up", 32, True), ("first_bits_48up", 48, True), ("first_bits_48up", 32, True),
                                ("first_bits_low16", 16, False), ("first_bits_16to31", 32, False), ("first_bits_32up", 48, False)):
        c = cases.small(name)
        assert (_rows(c, wrong_first_bits=bits) != _rows(c)) == changes, (name, bits)


def test_mistake_an_earliest_meeting_taken_from_the_first_copy_changes_the_lanes_cases():
    """a merge that keeps the first lane's meeting, or that drops the other lanes' copies"""
    for L in (2, 3, 8):
        c = cases.small("lanes%d_mixed" % L)
        first_lane_only, seen = [], {}
        for i, (f, t, s) in enumerate(c.triples()):
            lane = seen.setdefault((f, t), i % L)
            if i % L == lane:
                first_lane_only.append((f, t, s))
        assert model.fold(first_lane_only) != _rows(c)
        assert [r[:2] for r in model.fold(first_lane_only)] != [r[:2] for r in _rows(c)]          # the ORDER changes, not only the multiplicities
        lonely = cases.small("lanes%d_lonely" % L)
        without_last = [(f, t, s) for i, (f, t, s) in enumerate(lonely.triples()) if i % L != L - 1]
        assert model.fold(without_last) != _rows(lonely)
