// device_list.hpp -- SOAPDENOVO2_AMD_DEVICES=0,1,2,...: the GPU ordinals a command's ranks run on, one rank an entry, for `pregraph`
// (call_pregraph.cpp) and `map` (call_map.cpp).  An ordinal may repeat, which puts several ranks on one GPU -- how the N-rank paths are
// tested on a box with one GPU.  Parsing stops at the first thing that is neither a number nor a comma behind one.
#pragma once
#include <stdlib.h>

#include <vector>

namespace pg {

constexpr int DEVICE_LIST_MAX_RANKS = 256;       // most ranks of one command (pg_comm_create_local's bound)

inline std::vector<int> parse_device_list(const char* e) {
    std::vector<int> devices;
    if (!e) return devices;
    for (const char* q = e; *q;) {
        char* end = nullptr;
        const long v = strtol(q, &end, 10);
        if (end == q) break;
        devices.push_back((int)v);
        q = *end == ',' ? end + 1 : end;
        if (end == q && *q) break;
    }
    return devices;
}

}  // namespace pg
