"""The dropping of short isolated unitigs on the CPU: the host twin (pg_kindex_drop_isolated on a device = -1 index:
csrc/kisolated_host.cpp, the rule the kernels share in csrc/kisolated.hpp) against the independent model (tests/kisolated_model.py) on the
designs of tests/kisolated_cases.py -- each also against what its construction dictates: the totals and the word of every key of the
original set after every round --, every refusal, KmerIndex.drop_isolated and KmerIndex.simplify(ops=CLEAN_OPS), and under
-fsanitize=address,undefined in a stand-alone program (tests/kisolated_asan.cpp).  tests/test_gpu_kisolated.py runs the same through the
kernels.  All comparisons are of integers and exact."""

import pytest

import kcorrect_cases as C
import kindex_model as M
import kisolated_cases as G
import kisolated_model as I
import kunitig_model as U
import kwalk_cases as E
from host_program import build_and_run
from karc_cases import ALL_OPS
from karc_cases import model_simplify as four_name_simplify


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
@pytest.mark.parametrize("design", G.DESIGNS, ids=lambda d: d.__name__[6:])
def test_host_twin_matches_model_and_design(design, flavour):
    """Islands of 1, 2, max_len and max_len + 1 k-mers beside a deep path, either start deciding, both strands; sides that are dead
    ends and weak successors; a tip, the path before a fork, a ring, a hairpin's chain and a chain of max_len + 1 beside one island;
    the coverage bound at equality, one above it and saturated; 257 and 513 islands of mixed lengths; tombstones inside probe runs; an
    empty index and one of islands only; two calls back to back and drop_isolated; noisy reads of a genome with a repeat through
    simplify with all five operators, the default ops and a bad name."""
    design(flavour[0], flavour[1], -1)


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], -1, (-1, -1))


def test_the_models_leave_an_island_beside_the_simulated_ring():
    """The premise of the end-to-end test on the GPU, by the models alone over pure-Python records of the simulated read set at 2 / 1:
    the four operators leave more unitigs than the five, the difference is islands, and at max_cov below an island's mean coverage it
    stays."""
    reads, _ = C.simulated()
    K = C.SIM_K
    records = E.records_of(*E.count([(list(reads), 1)], K), 2)
    four, five, bounded = (M.Model.from_records(records, K, 2) for _ in range(3))
    four_name_simplify(four, ALL_OPS, 2, 1, 2 * K, 2 * K)
    left = I.islands(four.cnt, K, 2, 1, 2 * K)
    calls = G.model_simplify(five, G.CLEAN_OPS, 2, 1, 2 * K, 2 * K)
    n_four, n_five = len(U.unitigs(four, 2, 1)[0]), len(U.unitigs(five, 2, 1)[0])
    print("the simulated set at 2 / 1: %d unitigs after four operators, %d after five; islands left by four: %s" %
          (n_four, n_five, [(len(m), sum(I.coverage(four.cnt[k]) for k in m)) for m in left]))
    assert left and sum(t[0] for name, t in calls if name == "isolated") >= len(left) and n_five == n_four - len(left)
    least = min(-(-sum(I.coverage(four.cnt[k]) for k in m) // len(m)) for m in left)       # the least bound that removes one of them
    if least > 1:
        G.model_simplify(bounded, G.CLEAN_OPS, 2, 1, 2 * K, 2 * K, 0, least - 1)
        assert len(U.unitigs(bounded, 2, 1)[0]) == n_four


# ---- the host twin under the sanitizers, in a program of its own ----
def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/kisolated_asan.cpp: both flavours, the lengths and the not-islands designs checked against the construction, the
    refusals -- compiled with the host twin's sources and -fsanitize=address,undefined, and run.  Nothing loaded into Python is
    sanitised."""
    build_and_run(tmp_path, "kisolated_asan", ["kindex_host.cpp", "kunitig_host.cpp", "kisolated_host.cpp"], ["kisolated host twin: ok"])
