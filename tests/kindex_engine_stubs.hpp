// kindex_engine_stubs.hpp -- what a stand-alone program that links the k-mer index's host half alone (csrc/kindex_host.cpp, with or
// without csrc/ktrim_host.cpp) has to supply itself: the error string and the device engine's entry points (csrc/kindex.hpp,
// kcorrect.hpp, ktrim.hpp), here as stubs that fail.  Included once, by the program's one source file.
#pragma once
#include <string>

#include "../include/soapdenovo2_amd.h"
#include "kcorrect.hpp"
#include "kindex.hpp"
#include "ktrim.hpp"

static std::string g_err;
void pg_set_error(const std::string& s) { g_err = s; }
extern "C" const char* pg_last_error(void) { return g_err.c_str(); }

namespace pg {
static int no_device() { pg_set_error("no device engine in this program"); return PG_ENODEV; }
int kidx_device_build(::pg_kindex*, const uint64_t*, uint64_t, void*) { return no_device(); }
int kidx_device_query(::pg_kindex*, const KidxBatch&, int, uint64_t*, uint64_t*, void*) { return no_device(); }
void kidx_device_free(::pg_kindex*) {}
int kidx_device_build_sharded(::pg_kindex*, const uint64_t* const*, const uint64_t*, const int*, int, void*) { return no_device(); }
int kidx_device_query_sharded(::pg_kindex*, const KidxBatch&, int, uint64_t*, uint64_t*, void*) { return no_device(); }
int kidx_device_query_times(::pg_kindex*, double*) { return no_device(); }
int kcor_device_correct(::pg_kindex*, const KidxBatch&, const KcorParams&, uint64_t*, uint64_t*, void*) { return no_device(); }
int ktrim_device_trim(::pg_kindex*, const KidxBatch&, uint32_t, uint32_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, void*) { return no_device(); }
int ktrim_device_times(::pg_kindex*, double*) { return no_device(); }
}  // namespace pg
