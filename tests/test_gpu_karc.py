"""The dropping of arcs to weak k-mers on the GPU: the round's kernels with KarcOp (csrc/kindex_kernels.hip, csrc/karc.hpp) against the
independent model (tests/karc_model.py) on every design of tests/karc_cases.py, with the host twin edited in step: after every round
the totals and the word of every key of the original set are compared with the model's and, word for word, with the twin's.  Two lanes
that write the two halves of one word, start lists that cross wave and workgroup edges, two rounds queued back to back on one stream and
tombstones inside probe runs are among the designs.  Then KmerCounter -> index() -> simplify(ops = all four) -> unitigs() on the
simulated read set of the corrector's tests at 2 / 1.  All comparisons are of integers and exact; no test asserts a time or a rate."""
import pytest

import karc_cases as G
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


def test_counter_to_index_to_fully_simplified_unitigs():
    """At min_cov 2 and min_arc 1 the error k-mers are weak and the forks keep their arcs to them: simplify's calls, their order and
    totals, and then the unitigs are the model's, driven the same way; arcs were dropped, and the unitigs are fewer than after
    simplify() with the default ops."""
    calls, got, totals, model, want, before = G.simplified(2, 1)
    assert calls == want
    assert got == sorted(U.unitigs(model, 2, 1)[0])
    dropped = sum(t[1] for name, t in calls if name == "arcs")
    print("simplify at 2 / 1: %d calls %s, %d arcs dropped, unitigs %d with the default ops, %d with all four" % (len(calls), calls, dropped, before, totals["unitigs"]))
    assert dropped > 0 and totals["unitigs"] < before and totals["solid"] == totals["covered"]
