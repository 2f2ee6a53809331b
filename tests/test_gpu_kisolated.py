"""The dropping of short isolated unitigs on the GPU: the round's kernels with KisolatedOp (csrc/kindex_kernels.hip, csrc/kisolated.hpp)
against the independent model (tests/kisolated_model.py) on every design of tests/kisolated_cases.py, with the host twin edited in step:
after every round the totals and the word of every key of the original set are compared with the model's and, word for word, with the
twin's.  Islands of one k-mer, whose two starts are one slot's two orientations, start lists that hold both copies of every island and
cross wave and workgroup edges, two rounds queued back to back on one stream and tombstones inside probe runs are among the designs.
Then KmerCounter -> index() -> simplify(ops=CLEAN_OPS) -> unitigs() on the simulated read set of the corrector's tests at 2 / 1.  All
comparisons are of integers and exact; no test asserts a time or a rate."""
import pytest

import kisolated_cases as G
import kunitig_model as U
from soapdenovo2_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every test makes and destroys indexes, so the module pins the device arena (tests/test_gpu_kindex_sharded.py)."""
    with api.arena_pinned(0):
        yield


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
@pytest.mark.parametrize("design", G.DESIGNS, ids=lambda d: d.__name__[6:])
def test_device_matches_model_design_and_host_twin(design, flavour):
    design(flavour[0], flavour[1], 0, twin=-1)


@pytest.mark.parametrize("flavour", G.FLAVOURS, ids=G.flavour_id)
def test_refusals(flavour):
    G.check_refusals(flavour[0], flavour[1], 0, (0, 0))


def test_counter_to_index_to_cleaned_unitigs():
    """At min_cov 2 and min_arc 1 the four operators leave debris beside the ring: simplify's calls with all five names, their order
    and totals, and then the unitigs are the model's, driven the same way over the counter's own records; the calls named "isolated"
    removed at least one island, and the unitigs are fewer than after simplify(ops=SIMPLIFY_OPS) on a second index, by the islands
    removed where the model says so.  On the same records a max_cov one below the least mean coverage of the islands removed keeps
    them all, by the model and on the device."""
    calls, got, totals, model, want, before = G.cleaned(2, 1)
    assert calls == want
    assert got == sorted(U.unitigs(model, 2, 1)[0])
    islands = sum(t[0] for name, t in calls if name == "isolated")
    print("simplify at 2 / 1: %d calls %s, %d islands removed, unitigs %d with four operators, %d with five" % (len(calls), calls, islands, before, totals["unitigs"]))
    assert islands >= 1 and totals["unitigs"] < before and totals["solid"] == totals["covered"]


def test_max_cov_keeps_and_removes_the_simulated_island():
    """simplify(ops=CLEAN_OPS, max_cov=...) on the simulated set at 2 / 1, at max_cov 1 and 2: calls and unitigs are the model's at
    either bound; what each bound keeps or removes is what the model says (the island the four operators leave there has a coverage sum
    of 6 over 3 k-mers, if the counter's records are the pure-Python ones: kept at 1, removed at 2)."""
    seen = {}
    for max_cov in (1, 2):
        calls, got, totals, model, want, before = G.cleaned(2, 1, max_cov)
        assert calls == want and got == sorted(U.unitigs(model, 2, 1)[0])
        seen[max_cov] = (sum(t[0] for name, t in calls if name == "isolated"), max(t[3] for name, t in calls if name == "isolated"), totals["unitigs"])
    print("max_cov -> (islands removed, most kept in a round, unitigs): %s" % seen)
