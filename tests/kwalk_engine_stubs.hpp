// kwalk_engine_stubs.hpp -- kindex_engine_stubs.hpp for a stand-alone program that links csrc/kwalk_host.cpp too: the walk's device
// engine entry (csrc/kwalk.hpp) as a stub that fails, beside the index's.  Included once, by the program's one source file.
#pragma once
#include "kindex_engine_stubs.hpp"
#include "kwalk.hpp"

namespace pg {
int kwalk_device_walk(::pg_kindex*, const KidxBatch&, const KwalkParams&, uint64_t*, uint64_t*, void*) { return no_device(); }
}  // namespace pg
