// kindex_engine_stubs.hpp -- what a stand-alone program that links the k-mer index's host half (csrc/kindex_host.cpp, with any of the
// other *_host.cpp files of the index) has to supply itself: the error string and every entry point of the device engine
// (kindex_kernels.hip; declared in csrc/kindex.hpp, kcorrect.hpp, kcorrect_rows.hpp, ktrim.hpp, kwalk.hpp, kunitig.hpp, krank.hpp and
// kedit.hpp), here as stubs that fail.  Included once, by the program's one source file (through khost_program.hpp).
#pragma once
#include <string>

#include "../include/soapdenovo2_amd.h"
#include "karc.hpp"
#include "kbubble.hpp"
#include "kbulge.hpp"
#include "kcorrect.hpp"
#include "kcorrect_rows.hpp"
#include "kindex.hpp"
#include "krank.hpp"
#include "ktip.hpp"
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
int kcor_device_correct_rows(::pg_kindex*, const KidxBatch&, const KcorParams&, uint64_t*, uint64_t*, void*, uint64_t*) { return no_device(); }
int kwalk_device_walk(::pg_kindex*, const KidxBatch&, const KwalkParams&, uint64_t*, uint64_t*, void*) { return no_device(); }
int kunitig_device_unitigs(::pg_kindex*, const KunitigParams&, uint64_t, uint64_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, void*) {
    return no_device();
}
int kunitig_device_unitigs_ranked(::pg_kindex*, const KunitigParams&, uint64_t, uint64_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, void*) {
    return no_device();
}
template <class Op>
int kedit_device_round(::pg_kindex*, const typename Op::Params&, uint64_t*, void*) { return no_device(); }
template int kedit_device_round<KtipOp>(::pg_kindex*, const KtipParams&, uint64_t*, void*);
template int kedit_device_round<KbubbleOp>(::pg_kindex*, const KbubbleParams&, uint64_t*, void*);
template int kedit_device_round<KarcOp>(::pg_kindex*, const KarcParams&, uint64_t*, void*);
template int kedit_device_round<KbulgeOp>(::pg_kindex*, const KbubbleParams&, uint64_t*, void*);
}  // namespace pg
