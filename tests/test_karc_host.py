"""The dropping of arcs to weak k-mers on the CPU: the host twin (pg_kindex_drop_weak_arcs on a device = -1 index: csrc/kedit_ops_host.cpp,
the rule the kernels share in csrc/karc.hpp) against the independent model (tests/karc_model.py) on the designs of tests/karc_cases.py --
each also against what its construction dictates: the totals and the word of every key of the original set after every round --, every
refusal, KmerIndex.drop_weak_arcs and KmerIndex.simplify(ops=...), and, with the bulges', under -fsanitize=address,undefined in a
stand-alone program (tests/kedit_ops_asan.cpp).  tests/test_gpu_karc.py runs the same through the kernels.  All comparisons are of
integers and exact."""

import pytest

import karc_cases as G
from host_program import build_and_run


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
@pytest.mark.parametrize("design", G.DESIGNS, ids=lambda d: d.__name__[6:])
def test_host_twin_matches_model_and_design(design, flavour):
    """A single-copy read with a substitution on a deep path at 2 / 1, both strands, and at min_arc 2; targets with no record, with the
    deleted bit and tombstoned by clip_tips; three arcs of which two dangle, four that all dangle, two solid targets, counters of 63;
    both sides of one k-mer; 257 and 513 sides on one path; tombstones inside probe runs; an empty index; two calls back to back and
    drop_weak_arcs; noisy reads of a genome with a repeat through simplify with all four operators, the default ops and a bad name."""
    design(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], -1, (-1, -1))


# ---- the host twin under the sanitizers, in a program of its own ----
def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/kedit_ops_asan.cpp, the arcs' and the bulges' designs in one program over the one host twin: both flavours, two designs an
    operator, each checked against the construction -- compiled with the host twin's sources and -fsanitize=address,undefined, and run.
    Nothing loaded into Python is sanitised."""
    build_and_run(tmp_path, "kedit_ops_asan", ["kindex_host.cpp", "kunitig_host.cpp", "kedit_ops_host.cpp"], ["karc host twin: ok", "kbulge host twin: ok"])
