// kunitig_engine_stubs.hpp -- kindex_engine_stubs.hpp for a stand-alone program that links csrc/kunitig_host.cpp too: the unitigs' device
// engine entry (csrc/kunitig.hpp) as a stub that fails, beside the index's.  Included once, by the program's one source file.
#pragma once
#include "kindex_engine_stubs.hpp"
#include "kunitig.hpp"

namespace pg {
int kunitig_device_unitigs(::pg_kindex*, const KunitigParams&, uint64_t, uint64_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, void*) {
    return no_device();
}
}  // namespace pg
