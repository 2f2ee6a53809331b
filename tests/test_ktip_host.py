"""Tip clipping on the CPU: the host twin (pg_kindex_clip_tips on a device = -1 index: csrc/kedit_host.cpp, the rule the kernels share in
csrc/ktip.hpp) against the independent model (tests/ktip_model.py) on the designs of tests/ktip_cases.py -- each also against what its
construction dictates: the totals and the word of every key of the original set after every round --, every refusal, KmerIndex.clip_tips,
and under -fsanitize=address,undefined in a stand-alone program.  tests/test_gpu_ktip.py runs the same through the kernels.  All
comparisons are of integers and exact."""

import pytest

import ktip_cases as G
from host_program import build_and_run


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
@pytest.mark.parametrize("design", G.DESIGNS, ids=lambda d: d.__name__[6:])
def test_host_twin_matches_model_and_design(design, flavour):
    """A 1-read branch of 1 and 7 k-mers on a 5-read path, at max_tip n - 1 and n, the junction canonical and not, the reads reverse
    complemented, and the clipped index beside one built without the tip; a free side that is WEAK_NEXT by coverage and by the deleted
    bit; two dead ends from one k-mer with counters 1:1, 2:1 and 63:63; two minor tips at one junction side; a tip on a tip, by rounds,
    by two calls back to back and by clip_tips; the start of the graph before a fork, an island, a ring and a hairpin's chain, all kept;
    tombstones in the middle of probe runs; an empty index; 257 and 513 tips on one path; noisy reads of a genome with a repeat to the
    fixed point."""
    design(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], -1, (-1, -1))


# ---- the host twin under the sanitizers, in a program of its own ----
def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/kedit_asan.cpp, the tips' and the bubbles' designs in one program over the one host twin: both flavours, a path with
    one-k-mer tips and a tip on a tip, clipped by rounds to the fixed point, then three arms of one bubble and a bubble on an arm, popped
    by rounds to theirs, each checked against the construction -- compiled with the host twin's sources and
    -fsanitize=address,undefined, and run.  Nothing loaded into Python is sanitised."""
    build_and_run(tmp_path, "kedit_asan", ["kindex_host.cpp", "kunitig_host.cpp", "kedit_host.cpp"], ["ktip host twin: ok", "kbubble host twin: ok"])
