"""The read corrector on the GPU: kcor_kernel (csrc/kindex_kernels.hip, csrc/kcorrect.hpp) against the independent model
(tests/kcorrect_model.py) on every case of tests/kcorrect_cases.py, against the host twin on the simulated read set, in place against
two buffers, and the round trip count -> index -> correct -> count again.  All comparisons are of integers and exact; no test asserts a
time or a rate."""
import numpy as np
import pytest

import kcorrect_cases as E
import kindex_model as M
from conftest import oracle_records
from soapdenovo2_amd import api

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_device_matches_model(flavour):
    E.check_flavour(flavour[0], flavour[1], device=0)


@pytest.fixture(scope="module")
def simulated_records(tmp_path_factory):
    return oracle_records(E.simulated()[0], E.SIM_K, 8, prefix=str(tmp_path_factory.mktemp("kcorrect") / "o"))[0]


def _sim_params():
    return dict(min_cov=E.SIM_MIN_COV, max_fixes=api.CORRECT_MAX_FIXES, min_run=api.CORRECT_MIN_RUN)


def test_device_matches_host_twin_on_the_simulated_set(simulated_records):
    """The oracle's records of the simulated reads, indexed on the device and by the host twin: the same output words and reports,
    uniform and ragged -- and the model's (test_kcorrect_host.py checks what those are worth)."""
    reads = list(E.simulated()[0])
    host = E.Corrector(E.SIM_K, False, -1, records=simulated_records)
    dev = E.Corrector(E.SIM_K, False, 0, records=simulated_records, model=host.model)
    try:
        for uniform in (True, False):
            h_got, h_rep = host.run(reads, uniform=uniform, **_sim_params())
            d_got, d_rep = dev.check(reads, "simulated, uniform=%s" % uniform, uniform=uniform, **_sim_params())
            assert (h_got == d_got).all() and (h_rep == d_rep).all()
            assert int((d_rep & np.uint64(0xFF)).sum()) > 300
    finally:
        host.close()
        dev.close()


def test_in_place_equals_two_buffers(simulated_records):
    import torch
    reads = list(E.simulated()[0])
    dev = E.Corrector(E.SIM_K, False, 0, records=simulated_records)
    try:
        words, _, _, L = E.pack(reads, E.SIM_K, 2, True)
        d_in = dev.up(words.copy())
        out, rep = dev.ix.correct_uniform(d_in, len(reads), L, **_sim_params())
        assert out.data_ptr() != d_in.data_ptr() and (dev.down(d_in) == words).all()
        same, rep2 = dev.ix.correct_uniform(d_in, len(reads), L, out=d_in, **_sim_params())
        assert same.data_ptr() == d_in.data_ptr()
        assert torch.equal(out, d_in) and torch.equal(rep, rep2) and not (dev.down(out) == words).all()
        # a corrected batch is a fixed point for the reads that were restored: a second run makes no further fix in them
        _, rep3 = dev.ix.correct_uniform(d_in, len(reads), L, **_sim_params())
        clean = (dev.down(rep) & np.uint64(E.FLAGS)) == 0
        assert not dev.down(rep3)[clean].any()
    finally:
        dev.close()


def test_round_trip_through_the_counter():
    """KmerCounter counts the simulated reads -> finalize -> index() -> correct_uniform -> a fresh KmerCounter counts the corrected
    batch where it lies: as many distinct k-mers as the model's corrected reads hold, and fewer than before."""
    import torch
    reads, _ = E.simulated()
    K, n, L = E.SIM_K, reads.shape[0], reads.shape[1]
    before = len(M.count_reads(reads, K)[0])
    packed = torch.from_numpy(api.pack_reads_uniform(reads).view(np.int64)).cuda()
    kc = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    assert kc.distinct() == before
    ix = kc.index()
    records = kc.export()
    kc.close()
    fixed, _ = E.simulated_model_output(M.Model.from_records(records, K, 2))
    after = len(M.count_reads(fixed, K)[0])
    out, rep = ix.correct_uniform(packed, n, L, **_sim_params())
    ix.close()
    kc2 = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc2.count_uniform(out, n, L, 0)
    kc2.finalize(0)
    distinct = kc2.distinct()
    kc2.close()
    print("distinct k-mers before %d, after %d (model %d)" % (before, distinct, after))
    assert distinct == after and after < before
