"""ctypes binding of libsoapdenovo2_amd.so -- the C ABI declared in include/soapdenovo2_amd.h.

Python is plumbing here (tests, bench.py, the multi-GPU launcher): the product is the shared library and
the SOAPdenovo-63mer / SOAPdenovo-127mer executables next to it.  There is no Python or CPU fallback for the
device operators: if the library is missing, or no HIP device is usable, the calls raise.

Mirrors the reference's entry points `int call_pregraph(int argc, char **argv)` (standardPregraph/pregraph.c:62) as
:func:`call_pregraph` and `int call_align(int argc, char **argv)` (standardPregraph/map.c:94) as :func:`call_map`.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import subprocess
import sys
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "libsoapdenovo2_amd.so")
BIN_DIR = os.path.join(_HERE, "bin")

PG_ORD_BITS = 56
PG_ORD_MASK = (1 << PG_ORD_BITS) - 1

_lib = None


class PgError(RuntimeError):
    pass


def build(verbose: bool = False) -> None:
    """Compile the HIP extension and executables for gfx950 (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", ROOT, "-j8"], capture_output=not verbose, text=True)
    if out.returncode != 0:
        raise PgError("build failed:\n" + (out.stdout or "") + (out.stderr or ""))


# int fetch(void *user, uint64_t first_record, uint64_t n_records, uint64_t *dst)  (pg_graph_begin_streamed)
FETCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p)


def lib() -> C.CDLL:
    """Load the shared library (import torch first when torch is used in the same process, so that both
    share torch's HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SOAPDENOVO2_AMD_LIB", LIB_PATH)        # A/B builds of the library (development aid)
    if not os.path.exists(path):
        raise PgError(f"{path} is missing: run `make` (or __graft_entry__.build()) first; "
                      "there is no fallback implementation")
    L = C.CDLL(path, mode=C.RTLD_GLOBAL)
    u64p = C.c_void_p
    L.pg_last_error.restype = C.c_char_p
    L.pg_version.restype = C.c_char_p
    L.call_pregraph.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.call_pregraph_127mer.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.call_align.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.call_align_127mer.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    L.pg_map_reads.argtypes = [C.c_int, C.c_int, C.c_int, u64p, u64p, u64p, u64p, C.c_uint64, u64p, u64p, C.c_uint32,
                               u64p, u64p, u64p, C.c_uint64, C.c_int, u64p, u64p, u64p, u64p]
    L.pg_map_hits.argtypes = list(L.pg_map_reads.argtypes) + [u64p, u64p]
    L.pg_map_long_reads.argtypes = list(L.pg_map_hits.argtypes)
    L.pg_map_reads_sharded.argtypes = [u64p, C.c_int] + list(L.pg_map_reads.argtypes)[1:]
    L.pg_map_hits_sharded.argtypes = [u64p, C.c_int] + list(L.pg_map_hits.argtypes)[1:]
    L.pg_map_long_reads_sharded.argtypes = list(L.pg_map_hits_sharded.argtypes)
    L.pg_host_map_owner.argtypes = [u64p, C.c_uint64, C.c_int, C.c_int, u64p]
    L.pg_host_map_plan.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, u64p]
    L.pg_map_wave_ids.argtypes = [C.c_int]
    L.pg_map_long_last_stats.argtypes = [u64p]
    L.pg_map_long_last_stats.restype = None
    L.pg_packed_words.restype = C.c_size_t
    L.pg_packed_words.argtypes = [C.c_uint32]
    L.pg_pack_read.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.pg_host_build_graph.argtypes = [u64p, C.c_uint64, u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pg_host_write_kmerfreq.argtypes = [u64p, C.c_char_p]
    L.pg_host_graph_begin.restype = C.c_void_p
    L.pg_host_graph_begin.argtypes = [u64p, C.c_uint64, u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    L.pg_graph_begin.restype = C.c_void_p
    L.pg_graph_begin.argtypes = [u64p, C.c_uint64, u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.pg_graph_begin_streamed.restype = C.c_void_p
    L.pg_graph_begin_streamed.argtypes = [FETCH_FN, C.c_void_p, C.c_uint64, u64p, u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_char_p, C.c_int]
    L.pg_graph_begin_device.restype = C.c_void_p
    L.pg_graph_begin_device.argtypes = [u64p, C.c_int, C.c_uint64, u64p, u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.pg_host_graph_add_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
    L.pg_host_graph_finish.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    L.pg_host_graph_resolve_repeats.argtypes = [C.c_void_p, C.c_int]
    L.pg_graph_use_device.argtypes = [C.c_void_p, C.c_int]
    L.pg_expect_kmers.argtypes = [C.c_void_p, C.c_uint64]
    L.pg_set_read_len_bound.argtypes = [C.c_void_p, C.c_uint32]
    L.pg_expect.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.pg_host_plan_memory.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, u64p]
    L.pg_sort_records.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.pg_host_graph_add_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
    L.pg_host_read_all.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.pg_host_replay_layout.argtypes = [u64p, C.c_uint64, u64p, C.c_int, C.c_int, C.c_int, u64p, u64p]
    L.pg_create.restype = C.c_void_p
    L.pg_create.argtypes = [C.c_int] * 5
    L.pg_create_engine.restype = C.c_void_p
    L.pg_create_engine.argtypes = [C.c_int] * 6
    L.pg_create_planned.restype = C.c_void_p
    L.pg_create_planned.argtypes = [C.c_int] * 6 + [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.pg_create_sized.restype = C.c_void_p
    L.pg_create_sized.argtypes = [C.c_int] * 6 + [C.c_uint64]
    L.pg_destroy.argtypes = [C.c_void_p]
    L.pg_reset.argtypes = [C.c_void_p, C.c_void_p]
    L.pg_set_autogrow.argtypes = [C.c_void_p, C.c_int]
    L.pg_count_reads.argtypes = [C.c_void_p, u64p, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pg_route_count.argtypes = [C.c_void_p, u64p, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, u64p, C.c_void_p]
    L.pg_route_scatter.argtypes = [C.c_void_p, u64p, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int,
                                   u64p, u64p, u64p, C.c_void_p]
    L.pg_count_records.argtypes = [C.c_void_p, u64p, C.c_uint64, C.c_void_p]
    if not hasattr(L, "pg_skm_route"):          # an older A/B build of the library
        _lib = L
        return L
    L.pg_skm_route.argtypes = [C.c_void_p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, u64p, u64p, C.c_uint64, u64p, C.c_void_p]
    L.pg_skm_ingest.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, C.c_void_p]
    L.pg_distinct.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    L.pg_table_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.pg_stats.argtypes = [C.c_void_p, u64p]
    L.pg_finalize.argtypes = [C.c_void_p, C.c_int, u64p, u64p, C.c_void_p]
    L.pg_export.argtypes = [C.c_void_p, u64p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    L.pg_export_take.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pg_export_take_ws.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pg_sort_records_ws.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    L.pg_device_free.argtypes = [C.c_void_p]
    L.pg_device_arena_pin.argtypes = [C.c_int]
    L.pg_device_arena_unpin.argtypes = [C.c_int]
    L.pg_device_arena_stats.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    L.pg_host_emu_arena_blocks.restype = C.c_longlong
    L.pg_host_emu_arena_blocks.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.pg_export_peek.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.pg_records_checksum.argtypes = [C.c_void_p, C.c_uint64, C.c_int, u64p, C.c_void_p]
    L.pg_set_counts.argtypes = [C.c_void_p, u64p, C.c_void_p]
    L.pg_last_put.argtypes = [C.c_void_p, u64p, C.c_void_p]
    L.pg_host_last_put_matters.argtypes = [u64p, C.c_int, C.c_int, C.c_int]
    # multi-GPU exchange (include/soapdenovo2_amd.h, section 4)
    L.pg_comm_unique_id.argtypes = [C.c_void_p]
    L.pg_comm_create.restype = C.c_void_p
    L.pg_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.pg_comm_create_local.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.pg_comm_destroy.argtypes = [C.c_void_p]
    L.pg_comm_rank.argtypes = [C.c_void_p]
    L.pg_comm_size.argtypes = [C.c_void_p]
    L.pg_comm_transport.argtypes = [C.c_void_p]
    L.pg_comm_stats.argtypes = [C.c_void_p, u64p]
    L.pg_comm_pipeline_stats.argtypes = [C.c_void_p, u64p]
    L.pg_comm_create_host.restype = C.c_void_p
    L.pg_comm_create_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.pg_comm_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pg_exchange_counts.argtypes = [C.c_void_p, u64p, u64p, C.c_void_p]
    L.pg_exchange_records.argtypes = [C.c_void_p, u64p, u64p, C.c_uint64, C.c_int, u64p, u64p, u64p, u64p, C.c_void_p]
    L.pg_exchange_allreduce_u64.argtypes = [C.c_void_p, u64p, C.c_uint64, C.c_void_p]
    L.pg_exchange_gather_records.argtypes = [C.c_void_p, u64p, C.c_uint64, C.c_int, C.c_int, u64p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    L.pg_count_reads_sharded.argtypes = [C.c_void_p, C.c_void_p, u64p, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    L.pg_host_skm_cut.restype = C.c_int64
    L.pg_host_skm_cut.argtypes = [u64p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, u64p, u64p, C.c_uint64]
    L.pg_host_skm_expand.restype = C.c_int64
    L.pg_host_skm_expand.argtypes = [u64p, C.c_uint64, C.c_int, C.c_int, u64p, C.c_uint64]
    L.pg_host_emu_layout_growable.argtypes = [u64p, C.c_uint64, u64p, C.c_int, C.c_int, C.c_int, u64p, u64p, u64p, u64p, C.c_uint64]
    L.pg_host_regroup_plan.argtypes = [u64p, C.c_uint64, C.c_int, C.c_int, u64p, u64p]
    L.pg_host_emu_clip_tips.argtypes = [u64p, C.c_uint64, u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u64p]
    L.pg_host_emu_layout_static.argtypes = [u64p, u64p, C.c_int, C.c_uint64, C.c_int, C.c_int, u64p]
    L.pg_host_emu_home_slots.argtypes = [u64p, C.c_uint64, C.c_int, C.c_uint64, u64p]
    L.pg_device_emu_layout_static.argtypes = [C.c_int, u64p, u64p, C.c_int, C.c_uint64, C.c_int, u64p]
    L.pg_device_emu_layout_growable.argtypes = [C.c_int, u64p, C.c_uint64, u64p, C.c_int, C.c_int, u64p, u64p, u64p, C.c_uint64]
    L.pg_device_emu_home_slots.argtypes = [C.c_int, u64p, C.c_uint64, C.c_int, C.c_uint64, u64p]
    L.pg_device_emu_append.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, u64p, u64p]
    L.pg_device_emu_clip_tips.argtypes = [C.c_int, u64p, C.c_uint64, u64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u64p]
    L.pg_device_emu_prearcs.argtypes = [C.c_int, u64p, u64p, u64p, C.c_uint64, C.c_uint64, C.c_int, u64p, u64p, u64p]
    # the k-mer index (include/soapdenovo2_amd.h, section 3)
    L.pg_kindex_build.restype = C.c_void_p
    L.pg_kindex_build.argtypes = [C.c_int, C.c_int, C.c_int, u64p, C.c_uint64, C.c_void_p]
    L.pg_kindex_from_ctx.restype = C.c_void_p
    L.pg_kindex_from_ctx.argtypes = [C.c_void_p, C.c_void_p]
    L.pg_kindex_query.argtypes = [C.c_void_p, u64p, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, u64p, u64p, C.c_void_p]
    L.pg_kindex_correct.argtypes = [C.c_void_p, u64p, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u64p,
                                    C.c_void_p]
    L.pg_kindex_trim.argtypes = [C.c_void_p, u64p, C.c_uint64, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, u64p, u64p,
                                 u64p, u64p, u64p, u64p, C.c_void_p]
    L.pg_kindex_trim_times.argtypes = [C.c_void_p, u64p]
    L.pg_kindex_walk.argtypes = [C.c_void_p, u64p, C.c_uint64, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u64p,
                                 C.c_void_p]
    L.pg_kindex_unitigs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u64p, u64p, u64p, u64p, u64p, C.c_void_p]
    L.pg_kindex_unitigs_ranked.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u64p, u64p, u64p, u64p, u64p, C.c_void_p]
    L.pg_kindex_clip_tips.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u64p, C.c_void_p]
    L.pg_kindex_pop_bubbles.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, C.c_void_p]
    L.pg_kindex_drop_weak_arcs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, u64p, C.c_void_p]
    L.pg_kindex_pop_bulges.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, C.c_void_p]
    L.pg_kindex_drop_isolated.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, C.c_void_p]
    L.pg_kindex_info.argtypes = [C.c_void_p, u64p]
    L.pg_kindex_destroy.argtypes = [C.c_void_p]
    L.pg_kindex_destroy.restype = None
    L.pg_host_kindex_bytes.restype = C.c_uint64
    L.pg_host_kindex_bytes.argtypes = [C.c_uint64, C.c_int]
    L.pg_kindex_build_sharded.restype = C.c_void_p
    L.pg_kindex_build_sharded.argtypes = [u64p, C.c_int, C.c_int, C.c_int, u64p, u64p, u64p, C.c_int, C.c_void_p]
    L.pg_kindex_from_ctx_sharded.restype = C.c_void_p
    L.pg_kindex_from_ctx_sharded.argtypes = [C.c_void_p, u64p, C.c_int, C.c_void_p]
    L.pg_kindex_query_words.argtypes = [C.c_void_p, u64p, C.c_uint64, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, u64p, u64p, C.c_void_p]
    L.pg_kindex_correct_rows.argtypes = [C.c_void_p, u64p, C.c_uint64, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                         C.c_uint32, u64p, u64p, C.c_void_p]
    L.pg_kindex_correct_rows_stats.argtypes = [C.c_void_p, u64p]
    L.pg_kindex_ranks.argtypes = [C.c_void_p]
    L.pg_kindex_rank_info.argtypes = [C.c_void_p, C.c_int, u64p]
    L.pg_kindex_query_times.argtypes = [C.c_void_p, u64p]
    L.pg_host_kindex_plan.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, u64p]
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "pg_last_error", "pg_version", "call_pregraph", "call_pregraph_127mer", "pg_packed_words", "pg_pack_read",
    "pg_host_build_graph", "pg_host_graph_begin", "pg_host_graph_add_reads", "pg_host_graph_finish", "pg_process_exits_after_this", "pg_host_graph_resolve_repeats", "pg_host_graph_add_packed", "pg_graph_use_device", "pg_sort_records", "pg_expect_kmers", "pg_create_sized", "pg_graph_begin", "pg_graph_begin_streamed", "pg_host_read_all", "pg_host_replay_layout", "pg_host_write_kmerfreq", "pg_create", "pg_create_engine", "pg_destroy", "pg_reset", "pg_set_autogrow", "pg_count_reads", "pg_route_count",
    "pg_route_scatter", "pg_count_records", "pg_skm_route", "pg_skm_ingest", "pg_distinct", "pg_stats", "pg_table_info", "pg_finalize", "pg_export",
    "pg_export_take", "pg_export_take_ws", "pg_export_peek", "pg_records_checksum", "pg_sort_records_ws", "pg_device_free", "pg_device_arena_pin", "pg_device_arena_unpin", "pg_device_arena_stats", "pg_host_emu_arena_blocks", "pg_set_counts", "pg_last_put", "pg_host_last_put_matters", "pg_comm_unique_id", "pg_comm_create", "pg_comm_create_local", "pg_comm_destroy", "pg_comm_rank", "pg_comm_size",
    "pg_comm_transport", "pg_comm_stats", "pg_exchange_counts", "pg_exchange_records", "pg_exchange_allreduce_u64",
    "pg_exchange_gather_records", "pg_count_reads_sharded", "pg_host_skm_cut", "pg_host_skm_expand",
    "pg_host_emu_layout_static", "pg_graph_begin_device", "pg_host_emu_clip_tips", "pg_exchange_regroup_by_set", "pg_comm_regroup_stats", "pg_graph_begin_sharded", "pg_host_regroup_plan", "pg_host_bam_pair_state", "pg_device_scratch_offer", "pg_device_scratch_withdraw", "pg_host_emu_layout_growable", "pg_exchange_regroup_by_set_ws", "pg_host_edge_file_in_background", "pg_graph_add_packed_device", "pg_host_emu_home_slots", "pg_comm_pipeline_stats", "pg_comm_create_host", "pg_comm_flush",
    "pg_set_read_len_bound", "pg_graph_add_packed_device_ragged", "pg_expect", "pg_host_plan_memory", "pg_create_planned", "pg_graph_add_packed_device_segments",
    "call_align", "call_align_127mer", "pg_map_reads", "pg_map_hits", "pg_map_long_reads", "pg_map_wave_ids", "pg_map_long_last_stats",
    "pg_map_reads_sharded", "pg_map_hits_sharded", "pg_map_long_reads_sharded", "pg_host_map_owner", "pg_host_map_plan",
    "pg_kindex_build", "pg_kindex_from_ctx", "pg_kindex_query", "pg_kindex_correct", "pg_kindex_info", "pg_kindex_destroy", "pg_host_kindex_bytes",
    "pg_kindex_build_sharded", "pg_kindex_from_ctx_sharded", "pg_kindex_query_words", "pg_kindex_ranks", "pg_kindex_rank_info", "pg_kindex_query_times",
    "pg_host_kindex_plan", "pg_kindex_trim", "pg_kindex_trim_times", "pg_kindex_correct_rows", "pg_kindex_correct_rows_stats",
    "pg_kindex_walk", "pg_kindex_unitigs", "pg_kindex_unitigs_ranked", "pg_kindex_clip_tips", "pg_kindex_pop_bubbles", "pg_kindex_drop_weak_arcs", "pg_kindex_pop_bulges",
    "pg_kindex_drop_isolated",
    "pg_device_emu_layout_static", "pg_device_emu_layout_growable", "pg_device_emu_home_slots", "pg_device_emu_append", "pg_device_emu_clip_tips",
    "pg_device_emu_prearcs",
]


PLAN_FIELDS = ["peak", "peak_stage", "tables", "record_pool", "export_allocated", "export_after_count", "reads_kept", "batch_and_exchange", "kmer_sets",
               "layout_arrays", "sort_work_space_outside_pool", "log2_partition_ids", "log2_partitions_stored", "direct_chunks", "pool_records", "fits",
               "stage1_pass1_count", "stage2_hand_over", "stage3_layout", "stage4_graph_pass2", "est_kmers", "export_records", "set_slots", "log2_slots"]


def plan_memory(reads_total: int, read_len: int, distinct_total: int, K: int, n_sets: int = 8, a_gb: int = 0, n_ranks: int = 1,
                device_bytes: int = 288 * 10**9, fastq_bytes: int = 0) -> dict:
    """pg_host_plan_memory: the device memory one rank of the command takes, stage by stage (no GPU)."""
    out = np.zeros(24, dtype=np.uint64)
    _check(lib().pg_host_plan_memory(reads_total, read_len, fastq_bytes, distinct_total, K, 1 if K > 63 else 0, n_sets, a_gb, n_ranks, device_bytes,
                                     out.ctypes.data_as(C.POINTER(C.c_uint64))), "pg_host_plan_memory")
    d = {k: int(v) for k, v in zip(PLAN_FIELDS, out)}
    d["counts_twice"] = bool(d["log2_slots"] >> 32)
    d["log2_slots"] &= 0xFFFFFFFF
    return d


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise PgError(f"{what} failed ({rc}): {lib().pg_last_error().decode()}")


def binary(mer127: bool = False) -> str:
    return os.path.join(BIN_DIR, "SOAPdenovo-127mer" if mer127 else "SOAPdenovo-63mer")


def call_pregraph(args: Sequence[str], mer127: bool = False, in_process: bool = False) -> int:
    """`pregraph <args>`; args as for the reference, e.g. ["-s", cfg, "-K", "31", "-o", prefix, "-p", "8"].

    By default runs the executable in a child process (fatal input errors `exit()` like the reference's);
    in_process=True calls the C entry point directly."""
    if in_process:
        argv = [b"pregraph"] + [str(a).encode() for a in args]
        arr = (C.c_char_p * (len(argv) + 1))(*argv, None)
        fn = lib().call_pregraph_127mer if mer127 else lib().call_pregraph
        return fn(len(argv), arr)
    return subprocess.run([binary(mer127), "pregraph"] + [str(a) for a in args]).returncode


def call_map(args: Sequence[str], mer127: bool = False, in_process: bool = False, env=None) -> int:
    """`map <args>` (the reference's call_align, standardPregraph/map.c:94); args as for the reference, e.g.
    ["-s", cfg, "-g", prefix, "-p", "8", "-f"].  Runs the executable in a child process unless in_process=True."""
    if in_process:
        argv = [b"map"] + [str(a).encode() for a in args]
        arr = (C.c_char_p * (len(argv) + 1))(*argv, None)
        fn = lib().call_align_127mer if mer127 else lib().call_align
        return fn(len(argv), arr)
    return subprocess.run([binary(mer127), "map"] + [str(a) for a in args], env=env).returncode


def _pack_many(seqs):
    """pg_pack_read's layout for a list of base-code arrays: (words, word offsets [n + 1], lengths)."""
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum((lens.astype(np.uint64) + 31) // 32)
    words = np.zeros(int(off[-1]) + 1, dtype=np.uint64)
    for i, s in enumerate(seqs):
        s = np.asarray(s, dtype=np.uint64) & np.uint64(3)
        pos = np.arange(len(s))
        np.bitwise_or.at(words, off[i] + (pos >> 5).astype(np.uint64), s << (np.uint64(62) - np.uint64(2) * (pos & 31).astype(np.uint64)))
    return words, off, lens


def _map_call(name: str, device, *args):
    """pg_<name>(device, ...) for an int, pg_<name>_sharded(devices, n, ...) for a sequence of device ordinals (one rank each)."""
    if isinstance(device, (int, np.integer)):
        _check(getattr(lib(), "pg_" + name)(int(device), *args), "pg_" + name)
        return
    devs = np.ascontiguousarray(list(device), dtype=np.int32)
    _check(getattr(lib(), "pg_" + name + "_sharded")(devs.ctypes.data, len(devs), *args), "pg_" + name + "_sharded")


def map_reads(contigs, ctg_ids, id_len, id_bal, reads, K: int, align_len: int, mer127: bool = False, device=0):
    """The `map` stage's index + read kernel on one batch (pg_map_reads): contigs (base-code arrays, each of K + 2 bases or more) with
    their ids, the length / bal_edge of every contig id, reads (base-code arrays).  device = -1 runs the host twin.  A sequence of
    ordinals for `device` cuts the index over that many ranks, one a GPU named (pg_map_reads_sharded; an ordinal may repeat, all -1:
    the host twin of the cut).  Returns (ctg, pos, orien, footprint) arrays, one entry a read."""
    cw, co, cl = _pack_many(contigs)
    rw, ro, rl = _pack_many(reads)
    ids = np.ascontiguousarray(ctg_ids, dtype=np.uint32)
    il = np.ascontiguousarray(id_len, dtype=np.int32)
    ib = np.ascontiguousarray(id_bal, dtype=np.int8)
    n = len(reads)
    ctg = np.zeros(n, np.uint32); pos = np.zeros(n, np.int32); ori = np.zeros(n, np.uint8); fp = np.zeros(n, np.uint8)
    p = lambda a: a.ctypes.data
    _map_call("map_reads", device, K, 1 if mer127 else 0, p(cw), p(co), p(cl), p(ids), len(contigs), p(il), p(ib), len(il),
              p(rw), p(ro), p(rl), n, align_len, p(ctg), p(pos), p(ori), p(fp))
    return ctg, pos, ori, fp


def map_hits(contigs, ctg_ids, id_len, id_bal, reads, K: int, align_len: int, mer127: bool = False, device=0):
    """map_reads that also returns the hit word of every k-mer (pg_map_hits): (ctg, pos, orien, footprint, rows, kmer_off); read r's hit
    words are rows[kmer_off[r]:kmer_off[r + 1]] (csrc/map_decide.hpp gives their layout; 0 = absent or deleted key).  `device` as for
    map_reads (a sequence: pg_map_hits_sharded)."""
    cw, co, cl = _pack_many(contigs)
    rw, ro, rl = _pack_many(reads)
    ids = np.ascontiguousarray(ctg_ids, dtype=np.uint32)
    il = np.ascontiguousarray(id_len, dtype=np.int32)
    ib = np.ascontiguousarray(id_bal, dtype=np.int8)
    n = len(reads)
    ctg = np.zeros(n, np.uint32); pos = np.zeros(n, np.int32); ori = np.zeros(n, np.uint8); fp = np.zeros(n, np.uint8)
    n_k = int(sum(max(0, int(l) - K + 1) for l in rl if l >= K + 1))
    rows = np.full(n_k + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)         # (every word must be written: 0 is an answer)
    koff = np.zeros(n + 1, np.uint64)
    p = lambda a: a.ctypes.data
    _map_call("map_hits", device, K, 1 if mer127 else 0, p(cw), p(co), p(cl), p(ids), len(contigs), p(il), p(ib), len(il),
              p(rw), p(ro), p(rl), n, align_len, p(ctg), p(pos), p(ori), p(fp), p(rows), p(koff))
    return ctg, pos, ori, fp, rows[:n_k], koff


def map_long_reads(contigs, ctg_ids, id_len, id_bal, reads, K: int, align_len: int, mer127: bool = False, device=0,
                   want_hits: bool = False):
    """One batch of the long-read pass (pg_map_long_reads): the wave-per-read kernel on `device`, the host twin with device = -1.
    Arguments as map_reads (a sequence for `device`: pg_map_long_reads_sharded); returns what map_reads returns, or what map_hits
    returns with want_hits=True."""
    cw, co, cl = _pack_many(contigs)
    rw, ro, rl = _pack_many(reads)
    ids = np.ascontiguousarray(ctg_ids, dtype=np.uint32)
    il = np.ascontiguousarray(id_len, dtype=np.int32)
    ib = np.ascontiguousarray(id_bal, dtype=np.int8)
    n = len(reads)
    ctg = np.zeros(n, np.uint32); pos = np.zeros(n, np.int32); ori = np.zeros(n, np.uint8); fp = np.zeros(n, np.uint8)
    n_k = int(sum(max(0, int(l) - K + 1) for l in rl if l >= K + 1))
    rows = np.full(n_k + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) if want_hits else None
    koff = np.zeros(n + 1, np.uint64) if want_hits else None
    p = lambda a: a.ctypes.data if a is not None else None
    _map_call("map_long_reads", device, K, 1 if mer127 else 0, p(cw), p(co), p(cl), p(ids), len(contigs), p(il), p(ib), len(il),
              p(rw), p(ro), p(rl), n, align_len, p(ctg), p(pos), p(ori), p(fp), p(rows), p(koff))
    return (ctg, pos, ori, fp, rows[:n_k], koff) if want_hits else (ctg, pos, ori, fp)


def map_long_last_stats():
    """(reads answered in passes, distinct ids summed over the reads) of the last map_long_reads call on a device
    (pg_map_long_last_stats); (0, 0) after a host-twin call."""
    out = np.zeros(2, dtype=np.uint64)
    lib().pg_map_long_last_stats(out.ctypes.data)
    return int(out[0]), int(out[1])


MAP_PLAN_FIELDS = ["table", "slots", "keys", "rows", "staging", "reads", "build", "peak", "budget", "fits", "one_table", "fewest_ranks"]


def map_plan(n_ctg_kmers: int, mer127: bool = False, n_ranks: int = 1, batch_kmers: int = 10**8, device_bytes: int = 288 * 10**9) -> dict:
    """pg_host_map_plan: the device memory one rank of `map` takes with the index cut over n_ranks (1: one table), whether that fits
    the budget, and the fewest ranks that would (no GPU)."""
    out = np.zeros(12, dtype=np.uint64)
    _check(lib().pg_host_map_plan(n_ctg_kmers, 1 if mer127 else 0, n_ranks, batch_kmers, device_bytes, out.ctypes.data), "pg_host_map_plan")
    d = {k: int(v) for k, v in zip(MAP_PLAN_FIELDS, out)}
    d["fits"] = bool(d["fits"])
    return d


def map_owner(keys: np.ndarray, n_ranks: int, mer127: bool = False) -> np.ndarray:
    """pg_host_map_owner: the rank of n_ranks that owns each packed canonical key; keys = [n, 4 if mer127 else 2] uint64."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, 4 if mer127 else 2)
    out = np.zeros(len(keys), dtype=np.uint32)
    _check(lib().pg_host_map_owner(keys.ctypes.data, len(keys), 1 if mer127 else 0, n_ranks, out.ctypes.data), "pg_host_map_owner")
    return out


def map_wave_ids(mer127: bool = False) -> int:
    """Distinct contig ids of a read that the wave-per-read kernel's LDS table holds (pg_map_wave_ids); reads with more are answered
    in passes, with the same result."""
    return int(lib().pg_map_wave_ids(1 if mer127 else 0))


# ---------------------------------------------------------------------------------------------------------
# host helpers
# ---------------------------------------------------------------------------------------------------------
def packed_words(length: int) -> int:
    return (length + 31) // 32


def pack_reads_uniform(codes: np.ndarray) -> np.ndarray:
    """(n, L) uint8 base codes -> (n * words_per_read + 8,) uint64 in the device read format (vectorised
    equivalent of pg_pack_read: first base in the most significant bits, reads word-aligned; 8 words of
    readable padding at the end)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, L = codes.shape
    wpr = packed_words(L)
    padded = np.zeros((n, wpr * 32), dtype=np.uint64)
    padded[:, :L] = codes & 3
    shifts = (62 - 2 * np.arange(32, dtype=np.uint64)).astype(np.uint64)
    words = (padded.reshape(n, wpr, 32) << shifts[None, None, :]).sum(axis=2, dtype=np.uint64)
    out = np.zeros(n * wpr + 8, dtype=np.uint64)
    out[: n * wpr] = words.reshape(-1)
    return out


def pack_reads_ragged(reads: Sequence[np.ndarray], K: int):
    """List of 1-D uint8 code arrays (each len >= K + 1) -> (words, word_off, kmer_base) numpy uint64 arrays."""
    L = lib()
    n = len(reads)
    word_off = np.zeros(n, dtype=np.uint64)
    kmer_base = np.zeros(n + 1, dtype=np.uint64)
    total = 0
    for i, r in enumerate(reads):
        word_off[i] = total
        total += packed_words(len(r))
        kmer_base[i + 1] = kmer_base[i] + np.uint64(len(r) - K + 1)
    words = np.zeros(total + 8, dtype=np.uint64)
    for i, r in enumerate(reads):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        L.pg_pack_read(r.ctypes.data, len(r), words[int(word_off[i]):].ctypes.data)
    return words, word_off, kmer_base


def host_build_graph(records: np.ndarray, set_last_put, K: int, n_sets: int, prefix: str, mer127: bool = False,
                     cut_single: bool = True, a_gb: int = 0, max_read_len: int = 100, n_threads: int = 0):
    """records: (n, nw + 2) uint64.  Writes <prefix>.vertex/.edge.gz/.preGraphBasic; returns (n_vertex, n_edge)."""
    records = np.ascontiguousarray(records, dtype=np.uint64)
    slp = np.ascontiguousarray(set_last_put, dtype=np.uint64)
    nv, ne = C.c_int(0), C.c_int(0)
    rc = lib().pg_host_build_graph(records.ctypes.data, records.shape[0], slp.ctypes.data, K, int(mer127), n_sets,
                                   int(cut_single), a_gb, max_read_len, n_threads, prefix.encode(), C.byref(nv), C.byref(ne))
    _check(rc, "pg_host_build_graph")
    return nv.value, ne.value


def host_pregraph_files(records: np.ndarray, set_last_put, codes: np.ndarray, lens, K: int, n_sets: int, prefix: str,
                        mer127: bool = False, cut_single: bool = True, a_gb: int = 0, max_read_len: int = 100, n_threads: int = 0,
                        batches: int = 1, resolve_repeats: bool = False, packed: bool = False,
                        device: int = -1, device_edges: bool = False, streamed: bool = False):
    """All host stages incl. pass 2: writes .edge.gz .preArc .vertex .preGraphBasic (and, with resolve_repeats, the
    reference's -R files .path and .markOnEdge); returns (n_vertex, n_edge, n_prearc)."""
    records = np.ascontiguousarray(records, dtype=np.uint64)
    slp = np.ascontiguousarray(set_last_put, dtype=np.uint64)
    if streamed:                         # records handed over through the fetch callback, in replay order
        rw = records.shape[1]
        order = np.argsort(records[:, rw - 1], kind="stable")
        srt = np.ascontiguousarray(records[order])
        per_set = np.bincount((srt[:, rw - 1] >> np.uint64(56)).astype(np.int64), minlength=n_sets).astype(np.uint64)

        def _fetch(user, first, n, dst):
            C.memmove(dst, srt[first:].ctypes.data, n * rw * 8)
            return 0
        cb = FETCH_FN(_fetch)
        h = lib().pg_graph_begin_streamed(cb, None, srt.shape[0], per_set.ctypes.data, slp.ctypes.data, K, int(mer127), n_sets, int(cut_single),
                                          a_gb, max_read_len, n_threads, prefix.encode(), device if device_edges else -1)
    elif device_edges:                   # edges (and then pass 2) on HIP device `device`
        h = lib().pg_graph_begin(records.ctypes.data, records.shape[0], slp.ctypes.data, K, int(mer127), n_sets, int(cut_single),
                                 a_gb, max_read_len, n_threads, prefix.encode(), device)
    else:
        h = lib().pg_host_graph_begin(records.ctypes.data, records.shape[0], slp.ctypes.data, K, int(mer127), n_sets, int(cut_single),
                                      a_gb, max_read_len, n_threads, prefix.encode())
    if not h:
        raise PgError("pg_graph_begin failed: " + lib().pg_last_error().decode())
    if resolve_repeats:
        _check(lib().pg_host_graph_resolve_repeats(h, 1), "pg_host_graph_resolve_repeats")
    if device >= 0:                      # pass 2 on the HIP device instead of the host threads
        _check(lib().pg_graph_use_device(h, device), "pg_graph_use_device")
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, stride = codes.shape
    if lens is not None:
        lens = np.ascontiguousarray(lens, dtype=np.int32)
    bounds = np.linspace(0, n, batches + 1).astype(int)
    nv, ne, na = C.c_int(0), C.c_int(0), C.c_longlong(0)
    try:
        for b in range(batches):
            lo, hi = int(bounds[b]), int(bounds[b + 1])
            if hi > lo and packed:           # the reads as pass 1 packs them (pg_pack_read), back to back
                ls = lens[lo:hi] if lens is not None else np.full(hi - lo, stride, dtype=np.int32)
                words, _, _ = pack_reads_ragged([codes[i, :ls[i - lo]] for i in range(lo, hi)], K)
                ls = np.ascontiguousarray(ls, dtype=np.int32)
                _check(lib().pg_host_graph_add_packed(h, words.ctypes.data, ls.ctypes.data, hi - lo, n_threads), "pg_host_graph_add_packed")
            elif hi > lo:
                _check(lib().pg_host_graph_add_reads(h, codes[lo:].ctypes.data, lens[lo:].ctypes.data if lens is not None else None,
                                                     hi - lo, stride, n_threads), "pg_host_graph_add_reads")
    except PgError:                          # (pg_host_graph_finish releases the graph however it ends; the batch's error is the one to report)
        lib().pg_host_graph_finish(h, C.byref(nv), C.byref(ne), C.byref(na))
        raise
    _check(lib().pg_host_graph_finish(h, C.byref(nv), C.byref(ne), C.byref(na)), "pg_host_graph_finish")
    return nv.value, ne.value, na.value


def device_emu_prearcs(frm, to, seq, room: int, lanes: int = 1, device: int = 0) -> np.ndarray:
    """pg_device_emu_prearcs: the triples (frm[i], to[i], seq[i]) through pass 2's own pre-arc path on HIP device `device` -- `lanes` tables of `room`
    entries, triple i into table i mod lanes by add_prearc, read out and folded as a run's.  Returns the (from, to, multiplicity) rows in .preArc
    order.  A table that overflows raises PgError ("pre-arc table overflow") whose `overflow` is the number of triples that found no entry."""
    frm = np.ascontiguousarray(frm, dtype=np.uint32)
    to = np.ascontiguousarray(to, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint64)
    assert frm.shape == to.shape == seq.shape and frm.ndim == 1
    n = len(frm)
    out3 = np.zeros((max(n, 1), 3), dtype=np.uint32)
    cnt = np.zeros(2, dtype=np.uint64)
    rc = lib().pg_device_emu_prearcs(device, frm.ctypes.data, to.ctypes.data, seq.ctypes.data, n, room, lanes, out3.ctypes.data, cnt[0:].ctypes.data,
                                     cnt[1:].ctypes.data)
    if rc != 0:
        err = PgError(f"pg_device_emu_prearcs failed ({rc}): {lib().pg_last_error().decode()}")
        err.overflow = int(cnt[1])
        raise err
    return out3[:int(cnt[0])]


def host_read_all(config: str, K: int):
    """All reads the reference would hand to a pass over the inputs, in its order: (codes [n, stride] uint8, lens int32, n_records,
    max_rd_len).  (The BAM reader's pairing state is back at -3 after every file, readseq1by1.c:584-587: each pass sees the same reads.)"""
    nrec, nacc, mrl = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    _check(lib().pg_host_read_all(config.encode(), K, None, None, 0, 0, C.byref(nrec), C.byref(nacc), C.byref(mrl)), "pg_host_read_all")
    n, stride = nacc.value, max(mrl.value, 1)
    codes = np.zeros((max(n, 1), stride), dtype=np.uint8)
    lens = np.zeros(max(n, 1), dtype=np.int32)
    _check(lib().pg_host_read_all(config.encode(), K, codes.ctypes.data, lens.ctypes.data, n, stride, C.byref(nrec), C.byref(nacc),
                                  C.byref(mrl)), "pg_host_read_all")
    return codes[:n], lens[:n], nrec.value, mrl.value


def host_bam_state() -> int:
    return int(lib().pg_host_bam_pair_state(0, 0))


def host_replay_layout(records: np.ndarray, set_last_put, n_sets: int, mer127: bool = False, a_gb: int = 0):
    """Slot of every record in its reference k-mer set, and the per-set table sizes."""
    records = np.ascontiguousarray(records, dtype=np.uint64)
    slp = np.ascontiguousarray(set_last_put, dtype=np.uint64)
    slots = np.zeros(records.shape[0], dtype=np.uint64)
    sizes = np.zeros(n_sets, dtype=np.uint64)
    _check(lib().pg_host_replay_layout(records.ctypes.data, records.shape[0], slp.ctypes.data, int(mer127), n_sets, a_gb,
                                       slots.ctypes.data, sizes.ctypes.data), "pg_host_replay_layout")
    return slots, sizes


def host_write_kmerfreq(hist: np.ndarray, prefix: str) -> None:
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    assert hist.shape == (256,)
    _check(lib().pg_host_write_kmerfreq(hist.ctypes.data, prefix.encode()), "pg_host_write_kmerfreq")


# ---------------------------------------------------------------------------------------------------------
# device operators (torch tensors carry the device memory; the kernels are the library's)
# ---------------------------------------------------------------------------------------------------------
PG_COMM_RCCL, PG_COMM_P2P, PG_COMM_HOST = 0, 1, 2
HOST_A2A_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))


class Comm:
    """One rank of a pass-1 communicator (pg_comm_*): `Comm.rccl(n, rank, device, id)` for one rank per process,
    `Comm.local(devices)` for several ranks (host threads) in this process."""

    def __init__(self, handle, owner=True):
        self.h = handle
        self.owner = owner
        self._keep = None

    @staticmethod
    def host(n_ranks: int, rank: int, device: int, alltoallv) -> "Comm":
        """One rank per process, the variable all-to-all brought by the caller (pg_comm_create_host): alltoallv(send: bytes-like
        view, send_off, send_cnt, recv: writable view, recv_off, recv_cnt) over HOST memory, lists of n_ranks byte offsets / counts.
        For ranks that cannot talk RCCL (e.g. several processes on one GPU under gloo): exchange staged through the host."""
        def thunk(_user, send, soff, scnt, recv, roff, rcnt):
            try:
                so, sc = [int(soff[i]) for i in range(n_ranks)], [int(scnt[i]) for i in range(n_ranks)]
                ro, rc = [int(roff[i]) for i in range(n_ranks)], [int(rcnt[i]) for i in range(n_ranks)]
                s_len = max([o + c for o, c in zip(so, sc)] + [0])
                r_len = max([o + c for o, c in zip(ro, rc)] + [0])
                sv = (C.c_char * max(s_len, 1)).from_address(send)
                rv = (C.c_char * max(r_len, 1)).from_address(recv)
                alltoallv(memoryview(sv).cast("B"), so, sc, memoryview(rv).cast("B"), ro, rc)
                return 0
            except Exception as e:                                   # an exception must not unwind through the C frames
                import sys, traceback
                traceback.print_exc(file=sys.stderr)
                return 1
        fn = HOST_A2A_FN(thunk)
        h = lib().pg_comm_create_host(n_ranks, rank, device, C.cast(fn, C.c_void_p), None)
        if not h:
            raise PgError("pg_comm_create_host failed: " + lib().pg_last_error().decode())
        c = Comm(h)
        c._keep = fn                                                 # the callback lives as long as the communicator
        return c

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(lib().pg_comm_unique_id(C.addressof(buf)), "pg_comm_unique_id")
        return bytes(buf)

    @staticmethod
    def rccl(n_ranks: int, rank: int, device: int, uid: bytes) -> "Comm":
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        h = lib().pg_comm_create(n_ranks, rank, device, C.addressof(buf))
        if not h:
            raise PgError("pg_comm_create failed: " + lib().pg_last_error().decode())
        return Comm(h)

    @staticmethod
    def local(devices: Sequence[int], transport: int = -1):
        n = len(devices)
        dv = (C.c_int * n)(*devices)
        out = (C.c_void_p * n)()
        _check(lib().pg_comm_create_local(n, C.addressof(dv), transport, C.addressof(out)), "pg_comm_create_local")
        return [Comm(out[i]) for i in range(n)]

    @property
    def rank(self) -> int:
        return lib().pg_comm_rank(self.h)

    @property
    def size(self) -> int:
        return lib().pg_comm_size(self.h)

    @property
    def transport(self) -> str:
        return {PG_COMM_RCCL: "rccl", PG_COMM_P2P: "p2p", PG_COMM_HOST: "host"}[lib().pg_comm_transport(self.h)]

    def pipeline_stats(self) -> dict:
        out = np.zeros(8, dtype=np.uint64)
        _check(lib().pg_comm_pipeline_stats(self.h, out.ctypes.data), "pg_comm_pipeline_stats")
        return {"exchange_ms": int(out[0]) / 1000.0, "bytes_sent": int(out[1]), "host_waits": int(out[2]), "repeated_cuts": int(out[3]), "rounds": int(out[4]),
                "owner_region_records": int(out[5])}

    def flush(self, counter, stream=None) -> None:
        """What the last round of counter.count_sharded left in flight is appended to its partition streams (pg_finalize does it too)."""
        _check(lib().pg_comm_flush(counter.h, self.h, stream if stream is not None else counter._stream()), "pg_comm_flush")

    def stats(self) -> dict:
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().pg_comm_stats(self.h, out.ctypes.data), "pg_comm_stats")
        return {"rounds": int(out[0]), "sent_records": int(out[1]), "recv_records": int(out[2]), "cap": int(out[3])}

    def allreduce_u64(self, d_tensor, stream=None) -> None:
        _check(lib().pg_exchange_allreduce_u64(self.h, d_tensor.data_ptr(), d_tensor.numel(), stream), "pg_exchange_allreduce_u64")

    def close(self) -> None:
        if self.h and self.owner:
            lib().pg_comm_destroy(self.h)
        self.h = None


def arena_stats(device: int = 0) -> dict:
    """The library's device arena (csrc/arena.hpp): what it reserved, mapped and handed out on `device`."""
    out = (C.c_uint64 * 8)()
    lib().pg_device_arena_stats(device, out)
    keys = ("active", "reserved", "mapped", "in_use", "peak_in_use", "blocks_cut", "pieces_created", "create_us")
    return dict(zip(keys, [int(x) for x in out]))


class arena_pinned:
    """`with api.arena_pinned(0): ...` keeps the arena's physical memory across contexts created and destroyed inside the block."""
    def __init__(self, device: int = 0):
        self.device = device
    def __enter__(self):
        lib().pg_device_arena_pin(self.device)
        return self
    def __exit__(self, *a):
        lib().pg_device_arena_unpin(self.device)


def edge_file_in_background(on: bool) -> None:
    """<prefix>.edge.gz of the graphs THIS THREAD begins is written beside pass 2 (the library's flag is thread-local: call it on the
    thread that calls graph_begin*, not on another one)."""
    lib().pg_host_edge_file_in_background(1 if on else 0)


def hip_free(ptr) -> None:
    """hipFree of a device pointer the library handed over (pg_export_take)."""
    lib().pg_device_free(ptr)


def host_skm_cut(packed: np.ndarray, n_reads: int, read_len: int, K: int, mer127: bool, log2_parts: int, ord_base: int, n_owners: int):
    """Host twin of pg_skm_route (the same inline code the kernels run, skm.hpp): the batch's super-k-mer records and, per
    record, partition << 8 | owner.  -> (records [n, W] uint64, tags [n] uint64)."""
    nw = 4 if mer127 else 2
    W = 6 if nw == 2 else 8
    cap = n_reads * (read_len - K + 1)
    recs = np.zeros((cap, W), dtype=np.uint64)
    tags = np.zeros(cap, dtype=np.uint64)
    packed = np.ascontiguousarray(packed, dtype=np.uint64)
    n = lib().pg_host_skm_cut(packed.ctypes.data, n_reads, read_len, K, int(mer127), log2_parts, ord_base, n_owners, recs.ctypes.data,
                              tags.ctypes.data, cap)
    if n < 0:
        raise PgError("pg_host_skm_cut failed: " + lib().pg_last_error().decode())
    return recs[:n], tags[:n]


def host_skm_expand(records: np.ndarray, K: int, mer127: bool):
    """Host twin of the record expansion of K2: every k-mer occurrence of the records as rows
    (key words..., left, right, ordinal)."""
    nw = 4 if mer127 else 2
    records = np.ascontiguousarray(records, dtype=np.uint64)
    cap = int(((records[:, 0] >> np.uint64(2)) & np.uint64(0xFFFF)).sum()) if len(records) else 0
    out = np.zeros((max(cap, 1), nw + 3), dtype=np.uint64)
    n = lib().pg_host_skm_expand(records.ctypes.data, records.shape[0], K, int(mer127), out.ctypes.data, cap)
    if n < 0:
        raise PgError("pg_host_skm_expand failed: " + lib().pg_last_error().decode())
    return out[:n]


class KmerCounter:
    """Pass-1 counting context on one GPU (pg_create ... pg_export)."""

    def __init__(self, K: int, n_sets: int = 8, mer127: bool = False, log2_slots: int = 24, device: int = 0, engine: int = 0):
        import torch  # noqa: F401  (must be loaded before the library, see lib())
        self.torch = torch
        self.K, self.P, self.mer127, self.device = K, n_sets, mer127, device
        self.nw = 4 if mer127 else 2
        self.h = (lib().pg_create_engine(device, K, int(mer127), n_sets, log2_slots, engine) if engine
                  else lib().pg_create(device, K, int(mer127), n_sets, log2_slots))
        if not self.h:
            raise PgError("pg_create failed: " + lib().pg_last_error().decode())

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def count_uniform(self, d_packed, n_reads: int, read_len: int, ord_base: int = 0) -> int:
        """d_packed: int64/uint64 CUDA tensor in the device read format.  Returns the k-mers in the batch."""
        n_kmers = n_reads * (read_len - self.K + 1)
        _check(lib().pg_count_reads(self.h, d_packed.data_ptr(), None, None, n_reads, read_len, n_kmers, ord_base,
                                    self._stream()), "pg_count_reads")
        return n_kmers

    def set_read_len_bound(self, max_len: int) -> None:
        """No read of the ragged batches to come is longer (0: unknown -- every ragged batch then asks the device and waits)."""
        _check(lib().pg_set_read_len_bound(self.h, max_len), "pg_set_read_len_bound")

    def count_ragged(self, d_packed, d_word_off, d_kmer_base, n_reads: int, n_kmers: int, ord_base: int = 0) -> int:
        _check(lib().pg_count_reads(self.h, d_packed.data_ptr(), d_word_off.data_ptr(), d_kmer_base.data_ptr(), n_reads, 0,
                                    n_kmers, ord_base, self._stream()), "pg_count_reads")
        return n_kmers

    def route_count(self, d_packed, n_reads: int, read_len: int, n_owners: int):
        t = self.torch
        counts = t.zeros(n_owners, dtype=t.int64, device=f"cuda:{self.device}")
        n_kmers = n_reads * (read_len - self.K + 1)
        _check(lib().pg_route_count(self.h, d_packed.data_ptr(), None, None, n_reads, read_len, n_kmers, n_owners,
                                    counts.data_ptr(), self._stream()), "pg_route_count")
        return counts

    def route_scatter(self, d_packed, n_reads: int, read_len: int, ord_base: int, n_owners: int, owner_off, out):
        t = self.torch
        cursor = t.zeros(n_owners, dtype=t.int64, device=f"cuda:{self.device}")
        n_kmers = n_reads * (read_len - self.K + 1)
        _check(lib().pg_route_scatter(self.h, d_packed.data_ptr(), None, None, n_reads, read_len, n_kmers, ord_base, n_owners,
                                      owner_off.data_ptr(), cursor.data_ptr(), out.data_ptr(), self._stream()), "pg_route_scatter")

    def record_words(self) -> int:
        return 6 if self.nw == 2 else 8

    def skm_route(self, d_packed, n_reads: int, read_len: int, ord_base: int, n_owners: int, cap: int):
        """Engine 2, multi-GPU step 1 -> (records [n_owners, cap, W] int64, parts [n_owners, cap] int32, counts [n_owners] int64)."""
        t = self.torch
        dev = f"cuda:{self.device}"
        recs = t.empty((n_owners, cap, self.record_words()), dtype=t.int64, device=dev)
        parts = t.empty((n_owners, cap), dtype=t.int32, device=dev)
        counts = t.zeros(n_owners, dtype=t.int64, device=dev)
        _check(lib().pg_skm_route(self.h, d_packed.data_ptr(), n_reads, read_len, ord_base, n_owners, recs.data_ptr(), parts.data_ptr(),
                                  cap, counts.data_ptr(), self._stream()), "pg_skm_route")
        return recs, parts, counts

    def skm_ingest(self, d_records, d_parts, n_records: int) -> None:
        _check(lib().pg_skm_ingest(self.h, d_records.data_ptr(), d_parts.data_ptr(), n_records, self._stream()), "pg_skm_ingest")

    def count_records(self, d_records, n_records: int) -> None:
        _check(lib().pg_count_records(self.h, d_records.data_ptr(), n_records, self._stream()), "pg_count_records")

    def count_sharded(self, comm: "Comm", d_packed, n_reads: int, read_len: int, ord_base: int = 0, stream=None) -> None:
        """One round of multi-GPU pass 1 (collective over comm): cut, all-to-all, append.  d_packed may be None with n_reads = 0."""
        st = stream if stream is not None else self._stream()
        _check(lib().pg_count_reads_sharded(self.h, comm.h, d_packed.data_ptr() if d_packed is not None else None, None, None, n_reads,
                                            read_len if n_reads else 0, 0, ord_base, st), "pg_count_reads_sharded")

    def set_autogrow(self, on: bool) -> None:
        _check(lib().pg_set_autogrow(self.h, int(on)), "pg_set_autogrow")

    def reset(self) -> None:
        _check(lib().pg_reset(self.h, self._stream()), "pg_reset")

    def distinct(self) -> int:
        out = C.c_uint64(0)
        _check(lib().pg_distinct(self.h, C.byref(out), self._stream()), "pg_distinct")
        return out.value

    def table_info(self):
        s, b = C.c_uint64(0), C.c_uint32(0)
        _check(lib().pg_table_info(self.h, C.byref(s), C.byref(b)), "pg_table_info")
        return s.value, b.value

    def finalize(self, delow: int = 0, want_last_put: bool = True):
        hist = np.zeros(256, dtype=np.uint64)
        last = np.zeros(self.P, dtype=np.uint64)
        _check(lib().pg_finalize(self.h, delow, hist.ctypes.data, last.ctypes.data if want_last_put else None, self._stream()),
               "pg_finalize")
        return hist, last

    def set_counts(self) -> np.ndarray:
        out = np.zeros(256, dtype=np.uint64)
        _check(lib().pg_set_counts(self.h, out.ctypes.data, self._stream()), "pg_set_counts")
        return out[: self.P]

    def last_put(self) -> np.ndarray:
        out = np.zeros(self.P, dtype=np.uint64)
        _check(lib().pg_last_put(self.h, out.ctypes.data, self._stream()), "pg_last_put")
        return out

    def stats(self) -> dict:
        out = np.zeros(8, dtype=np.uint64)
        _check(lib().pg_stats(self.h, out.ctypes.data), "pg_stats")
        keys = ["engine", "distinct", "records", "unit_bytes", "pool_used", "pool_chunks", "parts_or_slots", "export_capacity"]
        return {k: int(v) for k, v in zip(keys, out)}

    def checksum(self) -> np.ndarray:
        """Order-independent digest of the distinct k-mers after finalize (pg_records_checksum on the export array in place):
        [column sums mod 2^64 (nw + 2 of them, zero-padded to 6), sum of the coverage fields, saturated nodes]."""
        ptr, n = C.c_void_p(0), C.c_uint64(0)
        _check(lib().pg_export_peek(self.h, C.byref(ptr), C.byref(n)), "pg_export_peek")
        out = np.zeros(8, dtype=np.uint64)
        _check(lib().pg_records_checksum(ptr, n.value, self.nw + 2, out.ctypes.data, self._stream()), "pg_records_checksum")
        return out

    def index(self, devices=None) -> "KmerIndex":
        """The k-mer index of the distinct k-mers, after finalize (pg_kindex_from_ctx): on this counter's device, and its own --
        the counter may be closed while the index lives.  devices = a sequence of ordinals: the index cut over those ranks
        (pg_kindex_from_ctx_sharded), the first one the lead."""
        if devices is None:
            h = lib().pg_kindex_from_ctx(self.h, self._stream())
            if not h:
                raise PgError("pg_kindex_from_ctx failed: " + lib().pg_last_error().decode())
            return KmerIndex(h, self.K, self.mer127, self.device)
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        h = lib().pg_kindex_from_ctx_sharded(self.h, devs.ctypes.data, len(devs), self._stream())
        if not h:
            raise PgError("pg_kindex_from_ctx_sharded failed: " + lib().pg_last_error().decode())
        return KmerIndex(h, self.K, self.mer127, int(devs[0]) if len(devs) else -1)

    def export(self, sort: bool = False) -> np.ndarray:
        """(n, nw + 2) uint64 records on the host (key words, cnt, set << 56 | first ordinal); with sort=True in the layout
        replay's insertion order (pg_sort_records on the device)."""
        t = self.torch
        n = self.distinct()
        rw = self.nw + 2
        d = t.empty(max(n, 1) * rw, dtype=t.int64, device=f"cuda:{self.device}")
        got = C.c_uint64(0)
        _check(lib().pg_export(self.h, d.data_ptr(), n, C.byref(got), self._stream()), "pg_export")
        assert got.value == n
        if sort:
            with t.cuda.device(self.device):
                _check(lib().pg_sort_records(d.data_ptr(), n, int(self.nw == 4), self._stream()), "pg_sort_records")
        return d[: n * rw].cpu().numpy().view(np.uint64).reshape(n, rw)

    def close(self) -> None:
        if self.h:
            lib().pg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------
# the k-mer index (pg_kindex_*): which k-mers of a batch of sequences were counted, and how often
# ---------------------------------------------------------------------------------------------------------
KINDEX_SUMMARY_FIELDS = ["present", "coverage_sum", "coverage_min", "first_absent"]


# The corrector's defaults (arguments of pg_kindex_correct, not constants of the kernel).
# max_fixes = 8: at a substitution rate of 1 % a read of 100 to 250 bases carries 1 to 2.5 errors on average and more than 8 about once
# in 10^5 reads; a read that needs more is more likely foreign or chimeric than unlucky, and is better left as it is (flag `limit`).
# min_run = 4: one solid k-mer is weak evidence at small K (a 4.6 Mb genome holds 14 % of all 13-mers, so a wrong base hits one by chance
# one time in seven; four in a row by chance need a real path of K + 3 bases), while two errors four or more bases apart are still
# fixed one after the other -- a run as long as K would leave every read with two errors inside one k-mer uncorrected.  Near a read's
# end, where fewer than min_run k-mers hold the base, all of them must be solid.
CORRECT_MAX_FIXES = 8
CORRECT_MIN_RUN = 4
CORRECT_FLAGS = {"no_kmers": 8, "no_anchor": 9, "stop_right": 10, "stop_left": 11, "limit": 12}


def report_fields(report) -> dict:
    """The corrector's report words split up: `fixes` (bases written), one boolean array a flag of CORRECT_FLAGS, and `weak` (the weak
    k-mers of the read as given).  Takes a numpy array or a torch tensor; returns numpy arrays."""
    if not isinstance(report, np.ndarray):
        report = report.cpu().numpy()
    w = np.ascontiguousarray(report).view(np.uint64)
    out = {"fixes": (w & np.uint64(0xff)).astype(np.int64), "weak": (w >> np.uint64(32)).astype(np.int64)}
    for name, bit in CORRECT_FLAGS.items():
        out[name] = (w >> np.uint64(bit)) & np.uint64(1) != 0
    return out


TRIM_TOTALS_FIELDS = ["kept", "words", "kmers", "bases_removed"]


def span_fields(spans) -> dict:
    """The trim's span words split up: `start` (the first base of a read's longest solid stretch) and `len` (its bases; 0: the read has
    no solid k-mer).  Takes a numpy array or a torch tensor; returns numpy arrays."""
    if not isinstance(spans, np.ndarray):
        spans = spans.cpu().numpy()
    w = np.ascontiguousarray(spans).view(np.uint64)
    return {"start": (w & np.uint64(0xffffffff)).astype(np.int64), "len": (w >> np.uint64(32)).astype(np.int64)}


# The walk (pg_kindex_walk).  WALK_REASONS[code] names a stop reason; WALK_MAX_EXT is the default of max_ext (32 words a row), WALK_EXT_BOUND
# the most the entry takes.
WALK_REASONS = {1: "no_kmer", 2: "seed_weak", 3: "dead_end", 4: "branch_out", 5: "weak_next", 6: "branch_in", 7: "loop", 8: "max_ext"}
WALK_MAX_EXT = 1024
WALK_EXT_BOUND = 1 << 20


def walk_fields(report) -> dict:
    """The walk's report words split up, one entry a walk (two walks a sequence: 2r from its last k-mer, 2r + 1 from the reverse complement
    of its first): `len` (bases appended), `reason` (a list of WALK_REASONS names), `code` (the reasons as numbers) and `coverage_sum` (of
    the appended k-mers).  Takes a numpy array or a torch tensor of 2 words a walk; returns numpy arrays."""
    if not isinstance(report, np.ndarray):
        report = report.cpu().numpy()
    w = np.ascontiguousarray(report).view(np.uint64).reshape(-1, 2)
    code = ((w[:, 0] >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    return {"len": (w[:, 0] & np.uint64(0xffffffff)).astype(np.int64), "code": code, "reason": [WALK_REASONS.get(int(c), "?") for c in code],
            "coverage_sum": w[:, 1].astype(np.int64)}


# The unitigs (pg_kindex_unitigs).  UNITIG_REASONS[code] names the reason of a unitig's side: the walk's end reasons, and hairpin, cycle, cut.
UNITIG_REASONS = {3: "dead_end", 4: "branch_out", 5: "weak_next", 6: "branch_in", 9: "hairpin", 10: "cycle", 11: "cut"}
UNITIG_MAX_KMERS = 1 << 24
UNITIG_KMERS_BOUND = 1 << 26
UNITIG_ENGINES = ("walk", "rank")
UNITIG_TOTALS_FIELDS = ["unitigs", "words", "bases", "covered", "solid", "cyclic", "cut", "overflow"]
Unitigs = collections.namedtuple("Unitigs", "packed word_off kmer_base report totals")


def unitig_fields(report) -> dict:
    """The unitigs' report words split up, one entry a unitig: `len` (bases), `left` and `right` (lists of UNITIG_REASONS names),
    `left_code` and `right_code` (the reasons as numbers) and `coverage_sum` (of the unitig's k-mers).  Takes a numpy array or a torch
    tensor of 2 words a unitig; returns numpy arrays."""
    if not isinstance(report, np.ndarray):
        report = report.cpu().numpy()
    w = np.ascontiguousarray(report).view(np.uint64).reshape(-1, 2)
    left = ((w[:, 0] >> np.uint64(32)) & np.uint64(0xff)).astype(np.int64)
    right = ((w[:, 0] >> np.uint64(40)) & np.uint64(0xff)).astype(np.int64)
    return {"len": (w[:, 0] & np.uint64(0xffffffff)).astype(np.int64), "left_code": left, "right_code": right,
            "left": [UNITIG_REASONS.get(int(c), "?") for c in left], "right": [UNITIG_REASONS.get(int(c), "?") for c in right],
            "coverage_sum": w[:, 1].astype(np.int64)}


# a round's four totals of an operator that edits the graph (the tips, the bubbles) by the operator's names
def _edit_fields(names, totals) -> dict:
    if not isinstance(totals, np.ndarray):
        totals = totals.cpu().numpy()
    return {k: int(v) for k, v in zip(names, np.ascontiguousarray(totals).view(np.uint64))}


# The tips (pg_kindex_clip_tips).  TIP_MAX_BOUND is the most max_tip the entry takes; its default is 2 K, the reference's tip length.
TIP_MAX_BOUND = 1 << 16
TIP_TOTALS_FIELDS = ["tips", "kmers", "solid", "kept"]


def tip_fields(totals) -> dict:
    """A round's totals (pg_kindex_clip_tips) by name: `tips` clipped, `kmers` removed, `solid` k-mers before the round, and the
    candidates `kept` because they were not minor.  Takes a numpy array or a torch tensor of 4 words."""
    return _edit_fields(TIP_TOTALS_FIELDS, totals)


# The bubbles (pg_kindex_pop_bubbles).  BUBBLE_MAX_BOUND is the most max_len and max_diff the entry takes; max_len's default is 2 K.
BUBBLE_MAX_BOUND = 1 << 16
BUBBLE_TOTALS_FIELDS = ["branches", "kmers", "solid", "kept"]


def bubble_fields(totals) -> dict:
    """A round's totals (pg_kindex_pop_bubbles) by name: `branches` popped, `kmers` removed, `solid` k-mers before the round, and the
    candidates `kept`: the branches that were not popped.  Takes a numpy array or a torch tensor of 4 words."""
    return _edit_fields(BUBBLE_TOTALS_FIELDS, totals)


# The arcs (pg_kindex_drop_weak_arcs) and the bulges (pg_kindex_pop_bulges, whose bounds are the bubbles').
ARC_TOTALS_FIELDS = ["sides", "arcs", "solid", "kept"]
BULGE_TOTALS_FIELDS = ["arms", "kmers", "solid", "kept"]
SIMPLIFY_OPS = ("arcs", "tips", "bubbles", "bulges")          # every operator simplify knows, in the order of the full set


def arc_fields(totals) -> dict:
    """A round's totals (pg_kindex_drop_weak_arcs) by name: `sides` pruned, `arcs` cleared, `solid` k-mers before the round, and the
    sides `kept`: those with several arcs out none of which dangles.  Takes a numpy array or a torch tensor of 4 words."""
    return _edit_fields(ARC_TOTALS_FIELDS, totals)


def bulge_fields(totals) -> dict:
    """A round's totals (pg_kindex_pop_bulges) by name: `arms` popped, `kmers` removed, `solid` k-mers before the round, and the
    arms `kept`.  Takes a numpy array or a torch tensor of 4 words."""
    return _edit_fields(BULGE_TOTALS_FIELDS, totals)


# The islands (pg_kindex_drop_isolated).  ISOLATED_MAX_BOUND is the most max_len the entry takes; its default is 2 K, as for the siblings.
ISOLATED_MAX_BOUND = 1 << 16
ISOLATED_TOTALS_FIELDS = ["islands", "kmers", "solid", "kept"]
CLEAN_OPS = SIMPLIFY_OPS + ("isolated",)                       # every operator simplify knows: SIMPLIFY_OPS and, behind them, the islands


def isolated_fields(totals) -> dict:
    """A round's totals (pg_kindex_drop_isolated) by name: `islands` removed, `kmers` removed, `solid` k-mers before the round, and the
    islands `kept`: those within max_len whose coverage is above max_cov a k-mer.  Takes a numpy array or a torch tensor of 4 words."""
    return _edit_fields(ISOLATED_TOTALS_FIELDS, totals)


def host_kindex_bytes(n_records: int, mer127: bool = False) -> int:
    """pg_host_kindex_bytes: the table an index of n_records k-mers cuts (no GPU)."""
    return int(lib().pg_host_kindex_bytes(n_records, 1 if mer127 else 0))


KINDEX_PLAN_FIELDS = ["table", "slots", "keys", "chunk", "rows", "staging", "batch_copy", "peak", "budget", "fits", "one_table", "fewest_ranks"]


def kindex_plan(n_records: int, mer127: bool = False, n_ranks: int = 1, batch_kmers: int = 10**8, batch_words: int = 10**7,
                device_bytes: int = 288 * 10**9) -> dict:
    """pg_host_kindex_plan: the device memory one rank of a k-mer index takes with the index cut over n_ranks (1: one table), whether that
    fits the budget, and the fewest ranks that would (no GPU)."""
    out = np.zeros(12, dtype=np.uint64)
    _check(lib().pg_host_kindex_plan(n_records, 1 if mer127 else 0, n_ranks, batch_kmers, batch_words, device_bytes, out.ctypes.data),
           "pg_host_kindex_plan")
    d = {k: int(v) for k, v in zip(KINDEX_PLAN_FIELDS, out)}
    d["fits"] = bool(d["fits"])
    return d


class KmerIndex:
    """A lookup table over the distinct k-mers of pass 1 (pg_kindex_*): `KmerCounter.index()` after finalize, or
    `KmerIndex.from_records(records, K)`.  On a GPU the batches and the answers are torch tensors of that device; with device = -1
    (the host twin, no GPU) they are numpy arrays.  An answer is a record's cnt word, 0 for a k-mer that is not in the set.
    An index cut over ranks (`device` a sequence of ordinals, `from_parts`, `KmerCounter.index(devices)`) answers the same queries with
    the same words; its batches and answers lie on the lead's device, `device`; it trims reads, and corrects them through correct_rows_uniform / correct_rows_ragged (correct_uniform and
    correct_ragged refuse it)."""

    def __init__(self, handle, K: int, mer127: bool, device: int):
        self.h, self.K, self.mer127, self.device = handle, K, mer127, device
        self.nw = 4 if mer127 else 2
        self.sharded = lib().pg_kindex_ranks(handle) > 0
        if device >= 0:
            import torch
            self.torch = torch

    @staticmethod
    def from_parts(parts, K: int, mer127: bool = False, devices=(0,)) -> "KmerIndex":
        """The index cut over the ranks `devices` (pg_kindex_build_sharded; ordinals may repeat, the first is the lead, all -1: the host
        twin).  parts: a list of (n, nw + 2) record arrays with keys distinct across all of them -- a numpy array is a part in host
        memory, a torch tensor a part on the tensor's device."""
        rw = (4 if mer127 else 2) + 2
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        lead = int(devs[0]) if len(devs) else -1
        keep, ptrs, counts, where = [], [], [], []
        for part in parts:
            if isinstance(part, np.ndarray):
                a = np.ascontiguousarray(part, dtype=np.uint64).reshape(-1, rw)
                keep.append(a)
                ptrs.append(a.ctypes.data if a.shape[0] else 0)
                counts.append(a.shape[0])
                where.append(-1)
            else:
                t = part.contiguous().view(-1)
                if not t.is_cuda or t.element_size() != 8:
                    raise PgError("KmerIndex.from_parts: a tensor part is 64-bit words on a GPU")
                keep.append(t)
                ptrs.append(t.data_ptr() if t.numel() else 0)
                counts.append(t.numel() // rw)
                where.append(t.device.index)
        stream = None
        if lead >= 0 and any(d >= 0 for d in where):
            import torch
            if not 0 <= lead < torch.cuda.device_count():
                raise PgError("KmerIndex.from_parts: HIP device %d does not exist" % lead)
            for t, d in zip(keep, where):                                     # (the build takes one stream, the lead's)
                if d >= 0 and d != lead:
                    torch.cuda.current_stream(d).synchronize()
            stream = C.c_void_p(torch.cuda.current_stream(lead).cuda_stream)
        a_ptrs, a_counts, a_where = np.array(ptrs, dtype=np.uint64), np.array(counts, dtype=np.uint64), np.array(where, dtype=np.int32)
        h = lib().pg_kindex_build_sharded(devs.ctypes.data, len(devs), K, 1 if mer127 else 0, a_ptrs.ctypes.data, a_counts.ctypes.data,
                                          a_where.ctypes.data, len(ptrs), stream)
        if not h:
            raise PgError("pg_kindex_build_sharded failed: " + lib().pg_last_error().decode())
        return KmerIndex(h, K, mer127, lead)

    @staticmethod
    def from_records(records, K: int, mer127: bool = False, device=0) -> "KmerIndex":
        """records: (n, nw + 2) records as KmerCounter.export returns them, any order -- a numpy array (copied to `device` for the
        build, or indexed where it lies by the host twin with device = -1) or a torch tensor on `device`.  device = a sequence of
        ordinals: the index cut over those ranks (from_parts), a numpy array as one host part, a tensor as one device part."""
        if not isinstance(device, (int, np.integer)):
            return KmerIndex.from_parts([records], K, mer127, device)
        rw = (4 if mer127 else 2) + 2
        keep = None
        if device < 0:
            keep = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, rw)
            n, ptr, stream = keep.shape[0], keep.ctypes.data, None
        else:
            import torch
            if isinstance(records, np.ndarray):
                records = torch.from_numpy(np.ascontiguousarray(records, dtype=np.uint64).reshape(-1).view(np.int64)).to(f"cuda:{device}")
            keep = records.contiguous().view(-1)
            if keep.device.index != device or keep.element_size() != 8:
                raise PgError("KmerIndex.from_records: the records are 64-bit words on the index's device")
            n, ptr = keep.numel() // rw, keep.data_ptr()
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        h = lib().pg_kindex_build(device, K, 1 if mer127 else 0, ptr if n else None, n, stream)
        if not h:
            raise PgError("pg_kindex_build failed: " + lib().pg_last_error().decode())
        return KmerIndex(h, K, mer127, device)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream) if self.device >= 0 else None

    def _ptr(self, a):
        if a is None:
            return None
        if self.device < 0:
            if a.dtype != np.uint64 or not a.flags["C_CONTIGUOUS"]:
                raise PgError("KmerIndex: the host twin takes contiguous numpy uint64 arrays")
            return a.ctypes.data
        return a.data_ptr()

    def _query(self, packed, word_off, kmer_base, n_seqs, uniform_len, n_kmers, wave, counts, summary):
        if not counts and not summary:
            raise PgError("KmerIndex: ask for the counts, the summary or both")
        # (one element at least: an empty array has no address, and a null pointer means "not wanted")
        if self.device < 0:
            out = np.zeros(max(n_kmers, 1), dtype=np.uint64) if counts else None
            summ = np.zeros((max(n_seqs, 1), 4), dtype=np.uint64) if summary else None
        else:
            t, dev = self.torch, f"cuda:{self.device}"
            out = t.zeros(max(n_kmers, 1), dtype=t.int64, device=dev) if counts else None
            summ = t.zeros((max(n_seqs, 1), 4), dtype=t.int64, device=dev) if summary else None
        if self.sharded:                            # (the ranks off the lead's device receive the batch: its extent goes along)
            n_words = int(packed.size if self.device < 0 else packed.numel()) if packed is not None else 0
            _check(lib().pg_kindex_query_words(self.h, self._ptr(packed), n_words, self._ptr(word_off), self._ptr(kmer_base), n_seqs, uniform_len,
                                               n_kmers, int(bool(wave)), self._ptr(out), self._ptr(summ), self._stream()), "pg_kindex_query_words")
        else:
            _check(lib().pg_kindex_query(self.h, self._ptr(packed), self._ptr(word_off), self._ptr(kmer_base), n_seqs, uniform_len, n_kmers,
                                         int(bool(wave)), self._ptr(out), self._ptr(summ), self._stream()), "pg_kindex_query")
        out = out[:n_kmers] if counts else None
        summ = summ[:n_seqs] if summary else None
        return (out, summ) if counts and summary else (out if counts else summ)

    def query_uniform(self, d_packed, n_seqs: int, seq_len: int, wave: bool = False, counts: bool = True, summary: bool = False):
        """Every sequence of seq_len bases, sequence r at word r * packed_words(seq_len) (pack_reads_uniform): the cnt words of its
        max(0, seq_len - K + 1) k-mers at [r * that ..) of the counts, a row of KINDEX_SUMMARY_FIELDS in the summary.  Returns the counts,
        the summary, or (counts, summary).  wave=True: a wavefront instead of a lane per sequence (contig-sized sequences)."""
        nk = max(0, seq_len - self.K + 1)
        return self._query(d_packed, None, None, n_seqs, seq_len, n_seqs * nk, wave, counts, summary)

    def query_ragged(self, d_packed, d_word_off, d_kmer_base, n_seqs: int, n_kmers: int, wave: bool = False, counts: bool = True,
                     summary: bool = False):
        """Sequences of any lengths (pack_seqs_ragged): sequence r starts at word d_word_off[r] and its answers at d_kmer_base[r]."""
        return self._query(d_packed, d_word_off, d_kmer_base, n_seqs, 0, n_kmers, wave, counts, summary)

    def _correct(self, packed, word_off, kmer_base, n_reads, uniform_len, min_cov, max_fixes, min_run, out):
        n_words = int(packed.size if self.device < 0 else packed.numel())
        if out is None:
            out = np.empty_like(packed) if self.device < 0 else self.torch.empty_like(packed)
        elif int(out.size if self.device < 0 else out.numel()) < n_words:
            raise PgError("KmerIndex: `out` is shorter than the batch")
        # (one element at least: an empty array has no address)
        report = np.zeros(max(n_reads, 1), dtype=np.uint64) if self.device < 0 else \
            self.torch.zeros(max(n_reads, 1), dtype=self.torch.int64, device=f"cuda:{self.device}")
        _check(lib().pg_kindex_correct(self.h, self._ptr(packed), self._ptr(word_off), self._ptr(kmer_base), n_reads, uniform_len, n_words, min_cov,
                                       max_fixes, min_run, self._ptr(out), self._ptr(report), self._stream()), "pg_kindex_correct")
        return out, report[:n_reads]

    def correct_uniform(self, d_packed, n_reads: int, read_len: int, min_cov: int, max_fixes: int = CORRECT_MAX_FIXES,
                        min_run: int = CORRECT_MIN_RUN, out=None):
        """Substitution errors of a batch of reads of read_len bases (pack_reads_uniform; the whole of d_packed is the batch, its
        readable tail included) corrected against the index (pg_kindex_correct): returns (packed_out, report).  packed_out is a new
        buffer, or `out` -- which may be d_packed itself: in place, same result.  A k-mer is solid when it is in the index with
        coverage >= min_cov; report_fields splits the report words.  See CORRECT_MAX_FIXES / CORRECT_MIN_RUN for the defaults."""
        return self._correct(d_packed, None, None, n_reads, read_len, min_cov, max_fixes, min_run, out)

    def correct_ragged(self, d_packed, d_word_off, d_kmer_base, n_reads: int, min_cov: int, max_fixes: int = CORRECT_MAX_FIXES,
                       min_run: int = CORRECT_MIN_RUN, out=None):
        """correct_uniform for reads of any lengths (pack_seqs_ragged); a read shorter than K comes back as it is, flagged."""
        return self._correct(d_packed, d_word_off, d_kmer_base, n_reads, 0, min_cov, max_fixes, min_run, out)

    def _correct_rows(self, packed, word_off, kmer_base, n_reads, uniform_len, n_kmers, min_cov, max_fixes, min_run, out):
        n_words = int(packed.size if self.device < 0 else packed.numel())
        if out is None:
            out = np.empty_like(packed) if self.device < 0 else self.torch.empty_like(packed)
        elif int(out.size if self.device < 0 else out.numel()) < n_words:
            raise PgError("KmerIndex: `out` is shorter than the batch")
        # (one element at least: an empty array has no address)
        report = np.zeros(max(n_reads, 1), dtype=np.uint64) if self.device < 0 else \
            self.torch.zeros(max(n_reads, 1), dtype=self.torch.int64, device=f"cuda:{self.device}")
        _check(lib().pg_kindex_correct_rows(self.h, self._ptr(packed), n_words, self._ptr(word_off), self._ptr(kmer_base), n_reads, uniform_len,
                                            n_kmers, min_cov, max_fixes, min_run, self._ptr(out), self._ptr(report), self._stream()),
               "pg_kindex_correct_rows")
        return out, report[:n_reads]

    def correct_rows_uniform(self, d_packed, n_reads: int, read_len: int, min_cov: int, max_fixes: int = CORRECT_MAX_FIXES,
                             min_run: int = CORRECT_MIN_RUN, out=None):
        """correct_uniform on any index, an index cut over ranks included (pg_kindex_correct_rows): the same arguments, the same
        (packed_out, report), bit for bit.  The trials are answered by rounds of batch queries over the ranks, and the call waits for
        the GPU once a round (correct_rows_stats); on an index in one table it is correct_uniform."""
        nk = max(0, read_len - self.K + 1)
        return self._correct_rows(d_packed, None, None, n_reads, read_len, n_reads * nk, min_cov, max_fixes, min_run, out)

    def correct_rows_ragged(self, d_packed, d_word_off, d_kmer_base, n_reads: int, min_cov: int, max_fixes: int = CORRECT_MAX_FIXES,
                            min_run: int = CORRECT_MIN_RUN, out=None, n_kmers=None):
        """correct_rows_uniform for reads of any lengths (pack_seqs_ragged).  n_kmers = d_kmer_base[n_reads]; where it is not given it
        is read from there, which on a GPU waits for the stream."""
        if n_kmers is None:
            n_kmers = int(d_kmer_base[n_reads]) if n_reads else 0
        return self._correct_rows(d_packed, d_word_off, d_kmer_base, n_reads, 0, n_kmers, min_cov, max_fixes, min_run, out)

    def correct_rows_stats(self) -> dict:
        """The last correct_rows_* call of this index (pg_kindex_correct_rows_stats): rounds that held a trial, trials, k-mers asked in
        trials, and the times the host waited for the GPU; zeros after a call on an index in one table."""
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().pg_kindex_correct_rows_stats(self.h, out.ctypes.data), "pg_kindex_correct_rows_stats")
        return {"rounds": int(out[0]), "trials": int(out[1]), "trial_kmers": int(out[2]), "host_waits": int(out[3])}

    def _trim(self, packed, word_off, kmer_base, n_reads, uniform_len, n_kmers, min_cov, min_len, pack):
        n_words = int(packed.size if self.device < 0 else packed.numel())
        min_len = self.K + 1 if min_len is None else min_len
        # (one element at least: an empty array has no address)
        if self.device < 0:
            new = lambda n: np.zeros(max(n, 1), dtype=np.uint64)
        else:
            new = lambda n: self.torch.zeros(max(n, 1), dtype=self.torch.int64, device=f"cuda:{self.device}")
        spans = new(n_reads)
        outs = (new(n_words), new(n_reads), new(n_reads + 1), new(n_reads), new(4)) if pack else (None,) * 5
        _check(lib().pg_kindex_trim(self.h, self._ptr(packed), n_words, self._ptr(word_off), self._ptr(kmer_base), n_reads, uniform_len, n_kmers,
                                    min_cov, min_len, self._ptr(spans), *[self._ptr(o) for o in outs], self._stream()), "pg_kindex_trim")
        return (spans[:n_reads],) + outs if pack else spans[:n_reads]

    def trim_uniform(self, d_packed, n_reads: int, read_len: int, min_cov: int, min_len=None, pack: bool = True):
        """Every read of a batch of reads of read_len bases (pack_reads_uniform; the whole of d_packed is the batch, its readable tail
        included) trimmed to its longest stretch of solid k-mers (pg_kindex_trim; solid as in correct_uniform).  Returns the span words
        (span_fields) and, when packing, (spans, packed_out, word_off_out, kmer_base_out, src_out, totals): the reads whose span has
        min_len bases or more (default K + 1: what KmerCounter.count_ragged takes) as one ragged batch in their input order, src_out the
        input index of each, totals = TRIM_TOTALS_FIELDS.  The outputs have the capacities the call needs -- packed_out as many words
        as d_packed, word_off_out and src_out n_reads, kmer_base_out n_reads + 1 -- and totals says how much of them is used; nothing
        waits for the GPU here, so read totals when the sizes are wanted.  Works on an index cut over ranks as well."""
        nk = max(0, read_len - self.K + 1)
        return self._trim(d_packed, None, None, n_reads, read_len, n_reads * nk, min_cov, min_len, pack)

    def trim_ragged(self, d_packed, d_word_off, d_kmer_base, n_reads: int, n_kmers: int, min_cov: int, min_len=None, pack: bool = True):
        """trim_uniform for reads of any lengths (pack_seqs_ragged); a read shorter than K has no k-mer and is dropped."""
        return self._trim(d_packed, d_word_off, d_kmer_base, n_reads, 0, n_kmers, min_cov, min_len, pack)

    def trim_times(self) -> dict:
        """Milliseconds of the last trim of a device index, from its events (pg_kindex_trim_times; waits for the trim)."""
        out = np.zeros(4, dtype=np.float64)
        _check(lib().pg_kindex_trim_times(self.h, out.ctypes.data), "pg_kindex_trim_times")
        return {"span": float(out[0]), "scan": float(out[1]), "pack": float(out[2]), "total": float(out[3])}

    def _walk(self, packed, word_off, kmer_base, n_seqs, uniform_len, min_cov, min_arc, max_ext):
        n_words = int(packed.size if self.device < 0 else packed.numel())
        row = packed_words(max_ext) if 0 < max_ext <= WALK_EXT_BOUND else 1     # (the entry refuses the rest; nothing is written then)
        # (one element at least: an empty array has no address)
        if self.device < 0:
            new = lambda n: np.zeros(max(n, 1), dtype=np.uint64)
        else:
            new = lambda n: self.torch.zeros(max(n, 1), dtype=self.torch.int64, device=f"cuda:{self.device}")
        ext, report = new(2 * n_seqs * row), new(4 * n_seqs)
        _check(lib().pg_kindex_walk(self.h, self._ptr(packed), n_words, self._ptr(word_off), self._ptr(kmer_base), n_seqs, uniform_len, min_cov,
                                    min_arc, max_ext, self._ptr(ext), self._ptr(report), self._stream()), "pg_kindex_walk")
        return ext[:2 * n_seqs * row].reshape(2 * n_seqs, row), report[:4 * n_seqs]

    def walk_uniform(self, d_packed, n_seqs: int, seq_len: int, min_cov: int, min_arc: int = 1, max_ext: int = WALK_MAX_EXT):
        """Unitigs walked from both ends of every sequence of a batch of seq_len bases (pack_reads_uniform; the whole of d_packed is the
        batch, its readable tail included) over the arc counters of the index (pg_kindex_walk).  Sequence r gives walk 2r, to the right
        of its last k-mer, and walk 2r + 1, to the right of the reverse complement of its first k-mer; a walk goes on while exactly one
        arc with a counter >= min_arc leaves the current k-mer, its successor is solid (coverage >= min_cov) and has that one arc
        coming in, for at most max_ext bases.  Returns (ext, report): ext[v] = walk v's bases in packed_words(max_ext) words
        (unpack_seq), report = two words a walk (walk_fields).  An index cut over ranks is refused."""
        return self._walk(d_packed, None, None, n_seqs, seq_len, min_cov, min_arc, max_ext)

    def walk_ragged(self, d_packed, d_word_off, d_kmer_base, n_seqs: int, min_cov: int, min_arc: int = 1, max_ext: int = WALK_MAX_EXT):
        """walk_uniform for sequences of any lengths (pack_seqs_ragged); one shorter than K gives two empty walks, reason no_kmer."""
        return self._walk(d_packed, d_word_off, d_kmer_base, n_seqs, 0, min_cov, min_arc, max_ext)

    def unitigs(self, min_cov: int, min_arc: int = 1, max_kmers: int = UNITIG_MAX_KMERS, engine: str = "walk") -> "Unitigs":
        """The whole graph of the index compacted into unitigs (pg_kindex_unitigs): every maximal unambiguous path -- exactly one arc
        with a counter >= min_arc out, a solid successor (coverage >= min_cov) with exactly that arc in -- once, in the orientation
        whose first k-mer is not greater, rings from their least k-mer; a walk stops after max_kmers k-mers (reason cut).  Returns
        Unitigs(packed, word_off, kmer_base, report, totals): a ragged batch of totals[0] sequences that query_ragged, walk_ragged and
        KmerCounter.count_ragged take as it lies (word_off and kmer_base have one entry more than there are unitigs, packed the
        readable tail), report = two words a unitig (unitig_fields) and totals = UNITIG_TOTALS_FIELDS as a numpy array.  Two calls:
        a count call, whose totals are read -- the one wait for the GPU here -- to allocate exactly, and the full call.  The order of
        the unitigs is unspecified.  An index cut over ranks is refused.
        engine: "walk" (the default) walks every chain with one lane, a dependent lookup a k-mer; "rank" (pg_kindex_unitigs_ranked) ranks
        all chains at once in ceil(log2 n) rounds and has no guard -- nothing is cut, a ring of any length is emitted, and a max_kmers
        other than the default is a ValueError -- at the price of scratch of 100 bytes a stored k-mer.  Where "walk" cuts nothing the
        two return the same unitigs.  The library does not choose between them."""
        if engine not in UNITIG_ENGINES:
            raise ValueError("KmerIndex.unitigs: engine is one of %s, not %r" % (", ".join(UNITIG_ENGINES), engine))
        if engine == "rank" and max_kmers != UNITIG_MAX_KMERS:
            raise ValueError("KmerIndex.unitigs: engine 'rank' has no guard: max_kmers stays at its default")
        if self.device < 0:
            new = lambda n: np.zeros(max(n, 1), dtype=np.uint64)
        else:
            new = lambda n: self.torch.zeros(max(n, 1), dtype=self.torch.int64, device=f"cuda:{self.device}")
        if engine == "rank":
            name, call = "pg_kindex_unitigs_ranked", lambda *a: lib().pg_kindex_unitigs_ranked(self.h, min_cov, min_arc, *a)
        else:
            name, call = "pg_kindex_unitigs", lambda *a: lib().pg_kindex_unitigs(self.h, min_cov, min_arc, max_kmers, *a)
        totals = new(8)
        _check(call(0, 0, None, None, None, None, self._ptr(totals), self._stream()), name)
        t = totals if self.device < 0 else totals.cpu().numpy().view(np.uint64)
        n, words = int(t[0]), int(t[1])
        packed, word_off, kmer_base, report = new(words), new(n + 1), new(n + 1), new(2 * n)
        _check(call(n, words, self._ptr(packed), self._ptr(word_off), self._ptr(kmer_base), self._ptr(report), self._ptr(totals), self._stream()), name)
        t = totals.copy() if self.device < 0 else totals.cpu().numpy().view(np.uint64)
        if int(t[7]):
            raise PgError("KmerIndex.unitigs: the full call needs more than the count call said")
        return Unitigs(packed[:words], word_off[:n + 1], kmer_base[:n + 1], report[:2 * n], t)

    def _edit_rounds(self, entry: str, args: tuple, max_rounds: int) -> list:
        """Rounds of the ABI entry `entry` with `args` until one removes nothing or max_rounds were called; each round's four totals."""
        call, rounds = getattr(lib(), entry), []
        while len(rounds) < max_rounds:
            totals = np.zeros(4, dtype=np.uint64) if self.device < 0 else self.torch.zeros(4, dtype=self.torch.int64, device=f"cuda:{self.device}")
            _check(call(self.h, *args, self._ptr(totals), self._stream()), entry)
            rounds.append(totals if self.device < 0 else totals.cpu().numpy().view(np.uint64))
            if not int(rounds[-1][0]):
                break
        return rounds

    def clip_tips(self, min_cov: int, min_arc: int, max_tip=None, max_rounds: int = 64) -> list:
        """Minor tips clipped from the index's graph, in place (pg_kindex_clip_tips): a tip is a chain of at most max_tip k-mers
        (default 2 K) that is free -- a dead end or a weak successor -- on one side and joins a k-mer with several arcs in on the
        other, and it is minor, and removed, when its arc into that k-mer has a strictly smaller counter than the strongest of the
        others.  A removed k-mer reads as absent from then on, to every operator; the records the index came from are not touched.
        Clipping a tip can turn the path it hung on into a tip, so rounds are called until one clips nothing or max_rounds is reached;
        each round's totals are read once -- the one wait for the GPU a round.  Returns the rounds' totals, a list of numpy arrays of
        TIP_TOTALS_FIELDS (tip_fields names them), the round that clipped nothing included.  Use the clipped index at the same or
        higher thresholds.  An index cut over ranks is refused."""
        max_tip = 2 * self.K if max_tip is None else max_tip
        return self._edit_rounds("pg_kindex_clip_tips", (min_cov, min_arc, max_tip), max_rounds)

    def pop_bubbles(self, min_cov: int, min_arc: int, max_len=None, max_diff: int = 0, max_rounds: int = 64) -> list:
        """Simple bubbles popped from the index's graph, in place (pg_kindex_pop_bubbles): a branch is a chain of at most max_len
        k-mers (default 2 K) that leaves one k-mer with several arcs out and joins another with several arcs in; two branches between
        the same two k-mers whose lengths differ by at most max_diff are siblings, and a branch is removed when a sibling has a strictly
        greater mean coverage -- ties are kept, so the strongest branch of every bubble stays.  A removed k-mer reads as absent from
        then on, to every operator; the records the index came from are not touched.  A bubble on a branch makes the outer bubble
        wait, so rounds are called until one pops nothing or max_rounds is reached; each round's totals are read once -- the one wait
        for the GPU a round.  Returns the rounds' totals, a list of numpy arrays of BUBBLE_TOTALS_FIELDS (bubble_fields names them),
        the round that popped nothing included.  Use the popped index at the same or higher thresholds.  An index cut over ranks is
        refused."""
        max_len = 2 * self.K if max_len is None else max_len
        return self._edit_rounds("pg_kindex_pop_bubbles", (min_cov, min_arc, max_len, max_diff), max_rounds)

    def drop_weak_arcs(self, min_cov: int, min_arc: int, max_rounds: int = 64) -> list:
        """Arcs to weak k-mers dropped from the index's graph, in place (pg_kindex_drop_weak_arcs): an arc of a solid k-mer whose
        counter is at least min_arc and whose target is not solid -- no such k-mer, a removed one, or coverage below min_cov -- gets
        the counter 0 in the solid k-mer's own word.  No k-mer is removed and none changes between solid and weak, so the second round
        finds nothing; rounds are called until one clears nothing or max_rounds is reached.  Returns the rounds' totals, a list of
        numpy arrays of ARC_TOTALS_FIELDS (arc_fields names them).  An index cut over ranks is refused."""
        return self._edit_rounds("pg_kindex_drop_weak_arcs", (min_cov, min_arc), max_rounds)

    def pop_bulges(self, min_cov: int, min_arc: int, max_len=None, max_diff: int = 0, max_rounds: int = 64) -> list:
        """Bubbles popped on their strongest paths, in place (pg_kindex_pop_bulges): an arm is pop_bubbles' branch, a chain of at most
        max_len k-mers (default 2 K) between a fork and a join; it is removed when the walk from the fork along the strictly
        strongest arc out of every k-mer, each also the strictly strongest arc into the next, reaches the join another way, with a
        length within max_diff of the arm's and a strictly greater mean coverage.  That path need not be a simple chain -- two errors
        less than K apart, a bubble or a tip on it --, it is never removed in the round that uses it, and ties end it, so the arm is
        then kept.  Rounds are called until one pops nothing or max_rounds is reached.  Returns the rounds' totals, a list of numpy
        arrays of BULGE_TOTALS_FIELDS (bulge_fields names them).  An index cut over ranks is refused."""
        max_len = 2 * self.K if max_len is None else max_len
        return self._edit_rounds("pg_kindex_pop_bulges", (min_cov, min_arc, max_len, max_diff), max_rounds)

    def drop_isolated(self, min_cov: int, min_arc: int, max_len=None, max_cov: int = 255, max_rounds: int = 64) -> list:
        """Short isolated unitigs dropped from the index's graph, in place (pg_kindex_drop_isolated): an island is a chain of at most
        max_len k-mers (default 2 K) that is free -- a dead end or a weak successor -- on both sides, and it is removed when the sum
        of its k-mers' coverage is at most max_cov a k-mer (1 to 255; the default, 255, is where the coverage saturates: every island
        within max_len).  A removed k-mer reads as absent from then on, to every operator; the records the index came from are not
        touched.  Rings, chains with a hairpin end and tips are not islands.  Rounds are called until one removes nothing or
        max_rounds is reached.  Returns the rounds' totals, a list of numpy arrays of ISOLATED_TOTALS_FIELDS (isolated_fields names
        them).  The library chooses neither bound for the caller.  An index cut over ranks is refused."""
        max_len = 2 * self.K if max_len is None else max_len
        return self._edit_rounds("pg_kindex_drop_isolated", (min_cov, min_arc, max_len, max_cov), max_rounds)

    def simplify(self, min_cov: int, min_arc: int, max_tip=None, max_len=None, max_diff: int = 0, max_rounds: int = 64,
                 ops=("tips", "bubbles"), max_cov: int = 255) -> list:
        """Every operator named in ops to its fixed point, in the order given, and all of them again -- a tip on a branch hides a
        bubble, a popped bubble can leave a tip, a removed k-mer leaves its neighbours' arcs dangling -- until a whole cycle removes
        nothing or max_rounds rounds were called in all.  ops: names of CLEAN_OPS -- "arcs" (drop_weak_arcs), "tips" (clip_tips),
        "bubbles" (pop_bubbles), "bulges" (pop_bulges), "isolated" (drop_isolated, with max_len and max_cov); the default is the tips
        and the bubbles, SIMPLIFY_OPS the four that edit the connected graph, CLEAN_OPS those and the islands behind them; a name
        that is none of them raises ValueError.  Returns the rounds in call order, a list of (name, totals)."""
        ops = tuple(ops)
        for name in ops:
            if name not in CLEAN_OPS:
                raise ValueError("KmerIndex.simplify: ops holds %r; the operators are %s" % (name, ", ".join(CLEAN_OPS)))
        run = {"arcs": lambda left: self.drop_weak_arcs(min_cov, min_arc, left), "tips": lambda left: self.clip_tips(min_cov, min_arc, max_tip, left),
               "bubbles": lambda left: self.pop_bubbles(min_cov, min_arc, max_len, max_diff, left),
               "bulges": lambda left: self.pop_bulges(min_cov, min_arc, max_len, max_diff, left),
               "isolated": lambda left: self.drop_isolated(min_cov, min_arc, max_len, max_cov, left)}
        out = []
        while len(out) < max_rounds:
            removed = 0
            for name in ops:
                left = max_rounds - len(out)
                rounds = run[name](left)
                out += [(name, r) for r in rounds]
                removed += sum(int(r[0]) for r in rounds)
            if not removed:
                break
        return out

    def info(self) -> dict:
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().pg_kindex_info(self.h, out.ctypes.data), "pg_kindex_info")
        fields = lambda o: {"keys": int(o[0]), "slots": int(o[1]), "bytes": int(o[2]), "device": int(o.view(np.int64)[3])}
        d = fields(out)
        d["ranks"] = []                             # (one table: its own four words)
        for i in range(max(1, lib().pg_kindex_ranks(self.h))):
            one = np.zeros(4, dtype=np.uint64)
            _check(lib().pg_kindex_rank_info(self.h, i, one.ctypes.data), "pg_kindex_rank_info")
            d["ranks"].append(fields(one))
        return d

    def query_times(self) -> dict:
        """Milliseconds of the last query of a device index cut over ranks, from its events (pg_kindex_query_times; waits for the query)."""
        out = np.zeros(4, dtype=np.float64)
        _check(lib().pg_kindex_query_times(self.h, out.ctypes.data), "pg_kindex_query_times")
        return {"probe": float(out[0]), "merge": float(out[1]), "summary": float(out[2]), "total": float(out[3])}

    def close(self) -> None:
        if self.h:
            lib().pg_kindex_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_seqs_ragged(seqs: Sequence[np.ndarray], K: int):
    """pack_reads_ragged for the k-mer index's batches: sequences of any length, those shorter than K included (they have no k-mers and
    keep their place) -> (words, word_off [n], kmer_base [n + 1]) numpy uint64, with 8 words of readable padding."""
    L = lib()
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    word_off = np.zeros(n, dtype=np.uint64)
    kmer_base = np.zeros(n + 1, dtype=np.uint64)
    if n:
        word_off[1:] = np.cumsum((lens[:-1] + 31) // 32)
        kmer_base[1:] = np.cumsum(np.maximum(lens - K + 1, 0))
    words = np.zeros(int(((lens + 31) // 32).sum()) + 8, dtype=np.uint64)
    for i, s in enumerate(seqs):
        s = np.ascontiguousarray(s, dtype=np.uint8)
        if len(s):
            L.pg_pack_read(s.ctypes.data, len(s), words[int(word_off[i]):].ctypes.data)
    return words, word_off, kmer_base


def kmer_coverage(seqs: Sequence[np.ndarray], index: KmerIndex, wave: bool = False):
    """The coverage of every k-mer of every sequence (base-code arrays, any lengths): a list of uint8 arrays, sequence i's of
    max(0, len - K + 1) entries, 0 for a k-mer that is not in the set."""
    words, word_off, kmer_base = pack_seqs_ragged(seqs, index.K)
    n_k = int(kmer_base[-1])
    if index.device < 0:
        cnt = index.query_ragged(words, word_off, kmer_base, len(seqs), n_k)
    else:
        t, dev = index.torch, f"cuda:{index.device}"
        up = lambda a: t.from_numpy(a.view(np.int64)).to(dev)
        cnt = index.query_ragged(up(words), up(word_off), up(kmer_base), len(seqs), n_k, wave=wave).cpu().numpy().view(np.uint64)
    cov = ((cnt >> np.uint64(24)) & np.uint64(0xff)).astype(np.uint8)
    return [cov[int(kmer_base[i]):int(kmer_base[i + 1])] for i in range(len(seqs))]


def unpack_seq(words: np.ndarray, length: int) -> np.ndarray:
    """The first `length` base codes of a packed sequence (the inverse of pg_pack_read)."""
    w = np.asarray(words[:packed_words(length)], dtype=np.uint64)
    shifts = (62 - 2 * np.arange(32, dtype=np.uint64)).astype(np.uint64)
    return ((w[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.uint8).reshape(-1)[:length]


def correct_reads(reads: Sequence[np.ndarray], index: KmerIndex, min_cov: int, max_fixes: int = CORRECT_MAX_FIXES,
                  min_run: int = CORRECT_MIN_RUN):
    """Substitution errors of reads (base-code arrays, any lengths) corrected against the index: (a list of base-code arrays of the
    same lengths, the report words as a numpy uint64 array -- see report_fields)."""
    words, word_off, kmer_base = pack_seqs_ragged(reads, index.K)
    # (an index cut over ranks: the rows form, which gives the same words)
    correct = functools.partial(index.correct_rows_ragged, n_kmers=int(kmer_base[-1])) if index.sharded else index.correct_ragged
    if index.device < 0:
        out, report = correct(words, word_off, kmer_base, len(reads), min_cov, max_fixes, min_run)
    else:
        t, dev = index.torch, f"cuda:{index.device}"
        up = lambda a: t.from_numpy(a.view(np.int64)).to(dev)
        out, report = correct(up(words), up(word_off), up(kmer_base), len(reads), min_cov, max_fixes, min_run)
        out, report = out.cpu().numpy().view(np.uint64), report.cpu().numpy().view(np.uint64)
    return [unpack_seq(out[int(word_off[i]):], len(r)) for i, r in enumerate(reads)], report


def trim_reads(reads: Sequence[np.ndarray], index: KmerIndex, min_cov: int, min_len=None):
    """Reads (base-code arrays, any lengths) trimmed to their longest solid stretch against the index: (a list of the base-code arrays of
    the kept reads, the input index of each as a numpy array, the span words of all reads -- see span_fields)."""
    words, word_off, kmer_base = pack_seqs_ragged(reads, index.K)
    n_k = int(kmer_base[-1])
    if index.device < 0:
        res = index.trim_ragged(words, word_off, kmer_base, len(reads), n_k, min_cov, min_len)
    else:
        t, dev = index.torch, f"cuda:{index.device}"
        up = lambda a: t.from_numpy(a.view(np.int64)).to(dev)
        res = [o.cpu().numpy().view(np.uint64) for o in index.trim_ragged(up(words), up(word_off), up(kmer_base), len(reads), n_k, min_cov, min_len)]
    spans, packed_out, word_off_out, _, src, totals = res
    n_kept = int(totals[0])
    lens = span_fields(spans)["len"]
    kept = [unpack_seq(packed_out[int(word_off_out[i]):], int(lens[int(src[i])])) for i in range(n_kept)]
    return kept, src[:n_kept].astype(np.int64), spans


def extend_seqs(seqs: Sequence[np.ndarray], index: KmerIndex, min_cov: int, min_arc: int = 1, max_ext: int = WALK_MAX_EXT):
    """Sequences (base-code arrays, any lengths; one of K bases is a seed k-mer) extended at both ends while the index's graph is
    unambiguous: (a list of base-code arrays, sequence i's = rc(walk 2i + 1) + seqs[i] + walk 2i, and the fields of all 2 n walks --
    see walk_fields)."""
    words, word_off, kmer_base = pack_seqs_ragged(seqs, index.K)
    if index.device < 0:
        ext, report = index.walk_ragged(words, word_off, kmer_base, len(seqs), min_cov, min_arc, max_ext)
    else:
        t, dev = index.torch, f"cuda:{index.device}"
        up = lambda a: t.from_numpy(a.view(np.int64)).to(dev)
        ext, report = [o.cpu().numpy().view(np.uint64) for o in index.walk_ragged(up(words), up(word_off), up(kmer_base), len(seqs), min_cov, min_arc, max_ext)]
    f = walk_fields(report)
    out = []
    for i, s in enumerate(seqs):
        right, left = unpack_seq(ext[2 * i], int(f["len"][2 * i])), unpack_seq(ext[2 * i + 1], int(f["len"][2 * i + 1]))
        out.append(np.concatenate([(left[::-1] ^ 2).astype(np.uint8), np.asarray(s, dtype=np.uint8), right]))
    return out, f


def unitig_seqs(index: KmerIndex, min_cov: int, min_arc: int = 1, max_kmers: int = UNITIG_MAX_KMERS, engine: str = "walk"):
    """The unitigs of the index's graph as base codes, for tests and small uses: (a list of base-code arrays, the fields of all of them
    -- see unitig_fields --, the totals as a dict of UNITIG_TOTALS_FIELDS).  The order of the unitigs is unspecified."""
    u = index.unitigs(min_cov, min_arc, max_kmers, engine)
    down = (lambda a: a) if index.device < 0 else (lambda a: a.cpu().numpy().view(np.uint64))
    packed, word_off, report = down(u.packed), down(u.word_off), down(u.report)
    f = unitig_fields(report)
    seqs = [unpack_seq(packed[int(word_off[i]):], int(f["len"][i])) for i in range(int(u.totals[0]))]
    return seqs, f, {k: int(v) for k, v in zip(UNITIG_TOTALS_FIELDS, u.totals)}
