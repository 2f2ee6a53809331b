"""Bubble popping on strongest paths on the GPU: the round's kernels with KbulgeOp (csrc/kindex_kernels.hip, csrc/kbulge.hpp) against
the independent model (tests/kbulge_model.py) on every design of tests/kbulge_cases.py, with the host twin popped in step: after every
round the totals and the word of every key of the original set are compared with the model's and, word for word, with the twin's.  Then
KmerCounter -> index() -> simplify(ops = all four) -> unitigs() on the simulated read set of the corrector's tests at 1 / 1.  All
comparisons are of integers and exact; no test asserts a time or a rate."""
import pytest

import kbulge_cases as G
import kunitig_model as U
from karc_cases import simplified
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
    """At min_cov 1 and min_arc 1 every error k-mer is solid: simplify's calls, their order and totals, and then the unitigs are the
    model's, driven the same way; arms were popped, and the unitigs are fewer than after simplify() with the default ops."""
    calls, got, totals, model, want, before = simplified(1, 1)
    assert calls == want
    assert got == sorted(U.unitigs(model, 1, 1)[0])
    popped = sum(t[0] for name, t in calls if name == "bulges")
    print("simplify at 1 / 1: %d calls %s, %d arms popped, unitigs %d with the default ops, %d with all four" % (len(calls), calls, popped, before, totals["unitigs"]))
    assert popped > 0 and totals["unitigs"] < before and totals["solid"] == totals["covered"]
