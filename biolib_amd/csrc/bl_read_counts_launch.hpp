// bl_read_counts_launch.hpp — what bl_capi.hip needs of bl_read_counts.hip for bl_scan_read_counts: the two launchers.
#pragma once
#include <hip/hip_runtime.h>
#include "bl_read_counts_core.hpp"

namespace blrc {
constexpr int ITPB = 256;            // threads per workgroup of the identity fill
constexpr int INIT_GRID_MAX = 2048;  // its workgroups at most: a thread strides over the touched records
hipError_t launch_read_counts_init(const ReadCountParams& p, hipStream_t stream);  // the identity into the records the range touches
hipError_t launch_read_counts(const ReadCountParams& p, hipStream_t stream);
}
