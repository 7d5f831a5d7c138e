// bl_kmers128_launch.hpp — host-callable launchers of the gfx950 kernels in bl_kmers128.hip: the dense 128-bit k-mer scan, and the two
// passes of its hash sampler (the tile prefix scan of bl_launch.hpp, launch_tile_scan, runs between them).
#pragma once
#include <hip/hip_runtime.h>
#include "bl_kmers128_core.hpp"

namespace bl {
hipError_t launch_kmers128(const Kmer128Params& p, hipStream_t stream);
hipError_t launch_kmers128_count(const Kmer128Params& p, hipStream_t stream);
hipError_t launch_kmers128_emit(const Kmer128Params& p, hipStream_t stream);
}  // namespace bl
