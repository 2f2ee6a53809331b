"""The walk on the CPU: the host twin (pg_kindex_walk on a device = -1 index: csrc/kwalk_host.cpp, the rule the kernel shares in
csrc/kwalk.hpp) against the independent model (tests/kwalk_model.py) on the designed cases of tests/kwalk_cases.py -- each also against
the text its construction dictates --, on tables of random counter words, at the batch sizes of the kernel's wave and workgroup edges,
every refusal, api.extend_seqs, and under -fsanitize=address,undefined in a stand-alone program.  tests/test_gpu_kwalk.py runs the same
through the kernel.  All comparisons are of integers and exact."""

import numpy as np
import pytest

import kwalk_cases as E
import kwalk_model as W
from host_program import build_and_run
from soapdenovo2_amd import api


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_host_twin_matches_model_and_design(flavour):
    """Every designed case: a linear genome from a seed, its reverse complement and a longer sequence; a shared prefix (BRANCH_OUT,
    BRANCH_IN); a branch of one read beside one of five at min_arc 1 and 2; WEAK_NEXT by coverage and by the deleted bit; a circular
    genome (LOOP); max_ext of 1, 31, 32, 33, 64 and 65; SEED_WEAK; NO_KMER in a ragged batch; counters at 63 with min_arc = 63 -- the
    model's rows and report words, the design's text and reason, either output alone, and a uniform batch where the lengths allow one."""
    E.check_flavour(flavour[0], flavour[1], device=-1)


@pytest.mark.parametrize("flavour", E.FLAVOURS, ids=E.flavour_id)
def test_batches_at_the_wave_and_workgroup_edges(flavour):
    E.check_batches(flavour[0], flavour[1], device=-1)


@pytest.mark.parametrize("flavour", [(13, False), (31, False), (65, True)], ids=E.flavour_id)
def test_random_counter_words(flavour):
    E.check_fuzz("n513", flavour[0], flavour[1], -1, [(1, 1), (100, 50), (200, 20)])
    E.check_fuzz("colliding", flavour[0], flavour[1], -1, [(100, 50)])


@pytest.mark.parametrize("flavour", [(31, False), (65, True)], ids=E.flavour_id)
def test_refusals(flavour):
    E.check_refusals(flavour[0], flavour[1], -1, (-1, -1))


def test_extend_seqs_and_walk_fields():
    """api.extend_seqs takes and returns base codes: a stretch of the linear genome comes back as the whole genome, its reverse
    complement as the genome's; walk_fields names the reasons."""
    K = 31
    g = E.linear(K)
    ix = api.KmerIndex.from_records(E.records_of(*E.linear_counts(K, 3), 2), K, False, -1)
    try:
        seqs = [g[60:60 + K + 9], E.rc(g[40:40 + K]), g[:K - 2]]
        out, f = api.extend_seqs(seqs, ix, 1)
        assert (out[0] == g).all() and (out[1] == E.rc(g)).all() and (out[2] == seqs[2]).all()
        assert f["reason"] == ["dead_end"] * 4 + ["no_kmer"] * 2 and list(f["code"]) == [3, 3, 3, 3, 1, 1]
        assert list(f["len"]) == [len(g) - 60 - K - 9, 60, 40, len(g) - 40 - K, 0, 0]
        short, f = api.extend_seqs(seqs[:1], ix, 1, 1, 7)
        assert (short[0] == g[53:60 + K + 9 + 7]).all() and f["reason"] == ["max_ext", "max_ext"]
        model = E.M.Model.from_records(E.records_of(*E.linear_counts(K, 3), 2), K, 2)
        assert list(f["coverage_sum"]) == [cov for _, _, cov in W.walks_of(model, seqs[0], 1, 1, 7)]
    finally:
        ix.close()


# ---- the host twin under the sanitizers, in a program of its own ----
def test_host_twin_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/kwalk_asan.cpp: both flavours, a ragged and a uniform batch with exactly nw + 1 words of tail, the output buffers on the heap
    at exactly the stated sizes -- compiled with the host twin's sources and -fsanitize=address,undefined, and run.  Nothing loaded into
    Python is sanitised."""
    build_and_run(tmp_path, "kwalk_asan", ["kindex_host.cpp", "kwalk_host.cpp"], ["kwalk host twin: ok"])
