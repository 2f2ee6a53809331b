"""The walk on the GPU: kwalk_kernel (csrc/kindex_kernels.hip, csrc/kwalk.hpp) against the independent model (tests/kwalk_model.py) and
word for word against the host twin on every case and batch of tests/kwalk_cases.py, two walks queued back to back on one stream, and
KmerCounter -> index() -> walk on the simulated read set of the corrector's tests.  All comparisons are of integers and exact; no test
asserts a time or a rate."""
import numpy as np
import pytest

import kcorrect_cases as C
import kindex_model as M
import kwalk_cases as E
import kwalk_model as W
from soapdenovo2_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every test makes and destroys indexes, so the module pins the device arena (tests/test_gpu_kindex_sharded.py)."""
    with api.arena_pinned(0):
        yield


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_device_matches_model_design_and_host_twin(flavour):
    E.check_flavour(flavour[0], flavour[1], device=0, twin=-1)


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_batches_at_the_wave_and_workgroup_edges(flavour):
    E.check_batches(flavour[0], flavour[1], device=0)


@pytest.mark.parametrize("flavour", [(13, False), (31, False), (65, True)], ids=E.flavour_id)
def test_random_counter_words(flavour):
    E.check_fuzz("n513", flavour[0], flavour[1], 0, [(1, 1), (100, 50), (200, 20)])
    E.check_fuzz("colliding", flavour[0], flavour[1], 0, [(100, 50)])


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=E.flavour_id)
def test_refusals(flavour):
    E.check_refusals(flavour[0], flavour[1], 0, (0, 0))


def test_two_walks_back_to_back_on_one_stream():
    """Two batches walked one after the other with no host wait in between, their outputs read afterwards: each is its own model's."""
    import torch
    K = 31
    w = E.Walker(E.records_of(*E.linear_counts(K, 3), 2), K, False, 0)
    try:
        first, second = E.batch(K, 129), E.batch(K, 33)[::-1]
        a = [w.up(x) for x in api.pack_seqs_ragged(first, K)]
        b = w.up(api.pack_reads_uniform(np.stack(second)))
        torch.cuda.synchronize()
        got_a = w.ix.walk_ragged(a[0], a[1], a[2], len(first), 1, 1, 70)
        got_b = w.ix.walk_uniform(b, len(second), K, 1, 1, 33)
        for (rows, rep), seqs, m in ((got_a, first, 70), (got_b, second, 33)):
            w_rows, w_rep, _ = W.want(w.model, seqs, 1, 1, m)
            assert (w.down(rows) == w_rows).all() and (w.down(rep) == w_rep).all()
    finally:
        w.close()


def test_counter_to_index_to_walk():
    """KmerCounter counts the simulated reads (a circular genome of 3 000 bases, 900 reads of 100 bases with substitutions, K = 31) ->
    finalize -> index() -> walks from 200 k-mers cut from the reads, at min_cov 3 and min_arc 2: the model's words over the counter's
    own records, the host twin's words, and walks that do extend."""
    import torch
    reads, _ = C.simulated()
    K, n, L = C.SIM_K, reads.shape[0], reads.shape[1]
    packed = torch.from_numpy(api.pack_reads_uniform(reads).view(np.int64)).cuda()
    kc = api.KmerCounter(K, n_sets=8, log2_slots=18)
    kc.count_uniform(packed, n, L, 0)
    kc.finalize(0)
    ix = kc.index()
    records = kc.export()
    kc.close()
    model = M.Model.from_records(records, K, 2)
    seeds = [reads[i, (7 * i) % (L - K + 1):][:K] for i in range(200)]
    d_seeds = torch.from_numpy(api.pack_reads_uniform(np.stack(seeds)).view(np.int64)).cuda()
    rows, rep = ix.walk_uniform(d_seeds, len(seeds), K, C.SIM_MIN_COV, 2, 256)
    ix.close()
    rows, rep = rows.cpu().numpy().view(np.uint64), rep.cpu().numpy().view(np.uint64)
    w_rows, w_rep, walks = W.want(model, seeds, C.SIM_MIN_COV, 2, 256)
    assert (rep == w_rep).all() and (rows == w_rows).all()
    host = api.KmerIndex.from_records(records, K, False, -1)
    h_rows, h_rep = host.walk_uniform(api.pack_reads_uniform(np.stack(seeds)), len(seeds), K, C.SIM_MIN_COV, 2, 256)
    host.close()
    assert (h_rows == rows).all() and (h_rep == rep).all()
    f = api.walk_fields(rep)
    print("walks: mean length %.1f, reasons %s" % (f["len"].mean(), {r: f["reason"].count(r) for r in set(f["reason"])}))
    assert f["len"].max() == 256 and (f["len"] > 0).sum() > 200
