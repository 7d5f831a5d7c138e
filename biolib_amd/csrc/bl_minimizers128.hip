// bl_minimizers128.hip — gfx950 kernels of bl_scan_minimizers128 (window minimizers of k-mers up to k = 64, 16-byte keys) and their
// launchers.  The per-thread bodies are in bl_minimizers128_core.hpp; the prefix scan between the two passes is launch_tile_scan
// (bl_launch.hpp).
#include <hip/hip_runtime.h>
#include "bl_scan128_launch.hpp"
#include "bl_tile128.hpp"

namespace bl {

namespace {

constexpr unsigned MIN128_SLOTS_LIVE = DIG_LO | DIG_HASH | DIG_POS | DIG_HI;  // the count comes from the prefix scan

struct Min128Shared {
    uint64_t hash[MIN128_SLOTS];  // the (canonical) units' hashes, from one chunk in front of the tile on
    uint32_t codes[MIN128_NCHUNK];
    uint32_t flags[MIN128_NCHUNK];
    unsigned long long dig[5];
    uint32_t wave_tot[TPB / 64];
    uint16_t valid[MIN128_NVALID + 1];
};

struct Min128EmitShared {
    uint32_t codes[MIN128_NCHUNK];
    uint32_t flags[MIN128_NCHUNK];
    uint32_t wave_tot[TPB / 64];
};

}  // namespace

// Both passes stage from r0 = q0 - 16 on: the chunk in front of the tile is staged like any other (zeros before the batch).
// Pass 1: per lane the mask of its records and their offsets, per tile their number; the digest of the records.
__global__ __launch_bounds__(TPB) void min128_count_kernel(const Min128Params p)
{
    __shared__ Min128Shared sh;
    const int tid = threadIdx.x;
    Kmer128Acc acc{0, 0, 0, 0, 0};
    zero_digest128<MIN128_SLOTS_LIVE>(sh.dig, tid);
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const int64_t r0 = p.km.origin + (int64_t)tile * H - 16;
        __syncthreads();  // the previous tile's hashes, codes and wave totals have been read
        stage_tile128<MIN128_NCHUNK>(p.km, sh.codes, sh.flags, tid, r0);
        __syncthreads();
        min128_hash_thread(p, sh.codes, sh.flags, sh.hash, sh.valid, tid, r0);
        __syncthreads();
        Min128Offs offs;
        const uint32_t sel = min128_window_thread(p, sh.hash, sh.valid, tid, r0, offs);
        min128_digest_thread(p.km, sh.codes, sh.hash, tid, r0, sel, offs, acc);
        if (p.lane_offs) min128_offs_store(p.lane_offs, tile, tid, offs);  // uniform: kept with the lane masks, for a second pass only
        publish_tile_count(p.km, sh.wave_tot, tile, tid, sel);
    }
    fold_digest128<MIN128_SLOTS_LIVE, 0>(p.km.shards, sh.dig, tid, acc);
}

// Pass 2: every tile's records at the tile's offset, lanes in order.
__global__ __launch_bounds__(TPB) void min128_emit_kernel(const Min128Params p)
{
    __shared__ Min128EmitShared sh;
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const unsigned long long base = tile_emit_base(p.km, tile);
        if (base >= p.km.capacity) continue;
        const int64_t r0 = p.km.origin + (int64_t)tile * H - 16;
        const uint32_t sel = p.km.lane_masks[(size_t)tile * TPB + tid];
        const Min128Offs offs = min128_offs_load(p.lane_offs, tile, tid);
        const uint32_t in_wave = rank_begin(sh.wave_tot, tid, sel);  // barrier: the previous tile's codes and wave totals have been read
        stage_tile128<MIN128_NCHUNK>(p.km, sh.codes, sh.flags, tid, r0);
        const uint32_t in_tile = rank_end(sh.wave_tot, tid, in_wave);  // barrier: the codes and the wave totals are written
        min128_emit_thread(p.km, sh.codes, tid, r0, sel, offs, base + in_tile);
    }
}

hipError_t launch_minimizers128_count(const Min128Params& p, hipStream_t stream) { return launch_tiles128(min128_count_kernel, p, p.km.n_tiles, stream); }
hipError_t launch_minimizers128_emit(const Min128Params& p, hipStream_t stream) { return launch_tiles128(min128_emit_kernel, p, p.km.n_tiles, stream); }

}  // namespace bl
