// bl_lookup_launch.hpp — what bl_capi.hip needs of bl_lookup.hip for bl_scan_kmer_counts: the table object and the scan's launcher.
#pragma once
#include <hip/hip_runtime.h>
#include "bl_lookup_core.hpp"

struct bl_ctx;

// The count table (include/biolib_amd.h: bl_table).  Its three device arrays are exact-size allocations of their own.
struct bl_table {
    bl_ctx* ctx;
    int device;
    bllk::TableView view;  // keys / counts / index: device pointers (keys and counts NULL for an empty table)
};

namespace bllk {
hipError_t launch_scan_counts(const ScanCountParams& p, hipStream_t stream);
}
