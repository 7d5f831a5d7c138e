// bl_scan128_launch.hpp — host-callable launchers of the gfx950 tile kernels of the 128-bit scans: the dense k-mer scan, and the two
// passes each of the hash sampler (bl_kmers128.hip), the syncmers (bl_syncmers128.hip) and the window minimizers
// (bl_minimizers128.hip).  The tile prefix scan of bl_launch.hpp, launch_tile_scan, runs between a count and an emit pass.
#pragma once
#include <hip/hip_runtime.h>
#include "bl_minimizers128_core.hpp"
#include "bl_syncmers128_core.hpp"

namespace bl {
hipError_t launch_kmers128(const Kmer128Params& p, hipStream_t stream);
hipError_t launch_kmers128_count(const Kmer128Params& p, hipStream_t stream);
hipError_t launch_kmers128_emit(const Kmer128Params& p, hipStream_t stream);
hipError_t launch_syncmers128_count(const Sync128Params& p, hipStream_t stream);
hipError_t launch_syncmers128_emit(const Sync128Params& p, hipStream_t stream);
hipError_t launch_minimizers128_count(const Min128Params& p, hipStream_t stream);
hipError_t launch_minimizers128_emit(const Min128Params& p, hipStream_t stream);
}  // namespace bl
