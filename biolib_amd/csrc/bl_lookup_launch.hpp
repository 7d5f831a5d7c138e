// bl_lookup_launch.hpp — what the other translation units need of bl_lookup.hip: the table object, the scan's launcher
// (bl_scan_kmer_counts, bl_capi.hip) and the first and last step of making a table (bl_table_combine, bl_table_ops.hip; bl_clean.hip).
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
// The last step of making a table: view.keys / counts / n / key_words / key_bits are set (sorted distinct keys in exact-size allocations
// of the table's own); chooses P under the context's "table_prefix_bits", allocates the index, fills it with index_fill_kernel and waits
// for the stream.  On an error the caller frees the table.
hipError_t finish_table(bl_ctx* ctx, bl_table* t, hipStream_t stream);
// The first step: the object with ctx / device / key_words / key_bits / n set and, when n > 0, its exact-size keys and counts arrays for the
// caller to fill.  BL_OK, or the error is set, nothing is left behind and *t is NULL.
int new_table(bl_ctx* ctx, uint32_t key_words, uint32_t key_bits, uint64_t n, bl_table** t);
void free_table(bl_table* t);  // the three arrays and the object
}
