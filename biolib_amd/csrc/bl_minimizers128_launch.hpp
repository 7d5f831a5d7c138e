// bl_minimizers128_launch.hpp — host-callable launchers of the gfx950 kernels in bl_minimizers128.hip: the two passes of
// bl_scan_minimizers128 (the tile prefix scan of bl_launch.hpp, launch_tile_scan, runs between them).
#pragma once
#include <hip/hip_runtime.h>
#include "bl_minimizers128_core.hpp"

namespace bl {
hipError_t launch_minimizers128_count(const Min128Params& p, hipStream_t stream);
hipError_t launch_minimizers128_emit(const Min128Params& p, hipStream_t stream);
}  // namespace bl
