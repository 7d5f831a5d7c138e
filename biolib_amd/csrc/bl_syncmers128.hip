// bl_syncmers128.hip — gfx950 kernels of bl_scan_syncmers128 (k <= 64, s <= 32, 16-byte s-mer keys) and their launchers.  The
// per-thread bodies are in bl_syncmers128_core.hpp; the tile layout is kmer_kernel's, the prefix scan between the two passes is
// launch_tile_scan (bl_launch.hpp).
#include <hip/hip_runtime.h>
#include "bl_scan128_launch.hpp"
#include "bl_tile128.hpp"

namespace bl {

namespace {

struct Sync128Shared {
    uint64_t hash[SYNC128_SLOTS];  // one strand's s-mer hashes at a time
    uint32_t codes[NCHUNK_POS];
    uint32_t flags[NCHUNK_POS];
    unsigned long long dig;
    uint32_t wave_tot[TPB / 64];
};

}  // namespace

// Pass 1: per lane the mask of its records, per tile their number; XOR of the records' positions.
__global__ __launch_bounds__(TPB) void sync128_count_kernel(const Sync128Params p)
{
    __shared__ Sync128Shared sh;
    const int tid = threadIdx.x;
    const bool canonical = p.km.canonical != 0;  // uniform
    Kmer128Acc acc{0, 0, 0, 0, 0};               // of the digest, only the positions' XOR is this scan's
    zero_digest128<DIG_POS>(&sh.dig, tid);
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.km.origin + (int64_t)tile * H;
        __syncthreads();  // the previous tile's hashes, codes and wave totals have been read
        stage_tile128<NCHUNK_POS>(p.km, sh.codes, sh.flags, tid, q0);
        __syncthreads();
        sync128_hash_thread(p, sh.codes, sh.hash, tid, false);
        uint32_t strand;
        const uint32_t ok = sync128_ok_strand(p.km, sh.codes, sh.flags, tid, q0, strand);
        __syncthreads();
        const uint32_t hit_fwd = sync128_window_thread<true>(sh.hash, tid, p.w, p.fwd_a, p.fwd_b);
        uint32_t hit_rev = 0;
        if (canonical) {
            __syncthreads();
            sync128_hash_thread(p, sh.codes, sh.hash, tid, true);
            __syncthreads();
            hit_rev = sync128_window_thread<false>(sh.hash, tid, p.w, p.rev_a, p.rev_b);
        }
        const uint32_t sel = sync128_select(p.km, tid, q0, ok, strand, hit_fwd, hit_rev, acc.sx);
        publish_tile_count(p.km, sh.wave_tot, tile, tid, sel);
    }
    fold_digest128<DIG_POS, 0>(p.km.shards, &sh.dig, tid, acc);
}

// Pass 2: every tile's records at the tile's offset, lanes in order.  Positions only: nothing is staged.
__global__ __launch_bounds__(TPB) void sync128_emit_kernel(const Sync128Params p)
{
    __shared__ uint32_t wave_tot[TPB / 64];
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const unsigned long long base = tile_emit_base(p.km, tile);
        if (base >= p.km.capacity) continue;
        const int64_t q0 = p.km.origin + (int64_t)tile * H;
        const uint32_t sel = p.km.lane_masks[(size_t)tile * TPB + tid];
        const uint32_t in_wave = rank_begin(wave_tot, tid, sel);  // barrier: the previous tile's wave totals have been read
        const uint32_t in_tile = rank_end(wave_tot, tid, in_wave);  // barrier: the wave totals are written
        sync128_emit_thread(p.km, tid, q0, sel, base + in_tile);
    }
}

hipError_t launch_syncmers128_count(const Sync128Params& p, hipStream_t stream) { return launch_tiles128(sync128_count_kernel, p, p.km.n_tiles, stream); }
hipError_t launch_syncmers128_emit(const Sync128Params& p, hipStream_t stream) { return launch_tiles128(sync128_emit_kernel, p, p.km.n_tiles, stream); }

}  // namespace bl
