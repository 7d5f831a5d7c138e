// bl_syncmers128_launch.hpp — host-callable launchers of the gfx950 kernels in bl_syncmers128.hip: the two passes of
// bl_scan_syncmers128 (the tile prefix scan of bl_launch.hpp, launch_tile_scan, runs between them).
#pragma once
#include <hip/hip_runtime.h>
#include "bl_syncmers128_core.hpp"

namespace bl {
hipError_t launch_syncmers128_count(const Sync128Params& p, hipStream_t stream);
hipError_t launch_syncmers128_emit(const Sync128Params& p, hipStream_t stream);
}  // namespace bl
