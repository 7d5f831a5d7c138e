// bl_kmers128.hip — gfx950 kernels of the 128-bit k-mer scans (k <= 64) and their launchers: the dense scan of bl_scan_kmers128 and
// the two passes of bl_scan_hash_sample128.  The per-thread bodies are in bl_kmers128_core.hpp; the tile layout is kmer_kernel's.
#include <hip/hip_runtime.h>
#include "bl_scan128_launch.hpp"
#include "bl_tile128.hpp"

namespace bl {

namespace {

struct Kmer128Shared {
    uint32_t codes[NCHUNK_POS];
    uint32_t flags[NCHUNK_POS];
    unsigned long long dig[5];
    uint32_t wave_tot[TPB / 64];
};

// the sampler's count comes from its prefix scan; its slot 3 is an XOR (of positions), the dense scan's a wrapping sum (of hashes)
constexpr unsigned SAMPLE_SLOTS = DIG_LO | DIG_HASH | DIG_POS | DIG_HI, DENSE_SLOTS = DIG_COUNT | SAMPLE_SLOTS;

}  // namespace

// Dense scan: workgroups stride over the tiles, no compaction.
__global__ __launch_bounds__(TPB) void kmer128_kernel(const Kmer128Params p)
{
    __shared__ Kmer128Shared sh;
    const int tid = threadIdx.x;
    Kmer128Acc acc{0, 0, 0, 0, 0};
    zero_digest128<DENSE_SLOTS>(sh.dig, tid);
    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.origin + (int64_t)tile * H;
        __syncthreads();  // the previous tile's codes and flags have been read
        stage_tile128<NCHUNK_POS>(p, sh.codes, sh.flags, tid, q0);
        __syncthreads();
        kmer128_dense_thread(p, sh.codes, sh.flags, tid, q0, acc);
    }
    fold_digest128<DENSE_SLOTS, DIG_COUNT | DIG_POS>(p.shards, sh.dig, tid, acc);
}

// Sampler pass 1: per lane the mask of its records, per tile their number; the digest of the records.
__global__ __launch_bounds__(TPB) void kmer128_count_kernel(const Kmer128Params p)
{
    __shared__ Kmer128Shared sh;
    const int tid = threadIdx.x;
    Kmer128Acc acc{0, 0, 0, 0, 0};
    zero_digest128<SAMPLE_SLOTS>(sh.dig, tid);
    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.origin + (int64_t)tile * H;
        __syncthreads();  // the previous tile's codes, flags and wave totals have been read
        stage_tile128<NCHUNK_POS>(p, sh.codes, sh.flags, tid, q0);
        __syncthreads();
        const uint32_t sel = kmer128_count_thread(p, sh.codes, sh.flags, tid, q0, acc);
        publish_tile_count(p, sh.wave_tot, tile, tid, sel);
    }
    fold_digest128<SAMPLE_SLOTS, 0>(p.shards, sh.dig, tid, acc);
}

// Sampler pass 2: every tile's records at the tile's offset, lanes in order.
__global__ __launch_bounds__(TPB) void kmer128_emit_kernel(const Kmer128Params p)
{
    __shared__ Kmer128Shared sh;
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const unsigned long long base = tile_emit_base(p, tile);
        if (base >= p.capacity) continue;
        const int64_t q0 = p.origin + (int64_t)tile * H;
        const uint32_t sel = p.lane_masks[(size_t)tile * TPB + tid];
        const uint32_t in_wave = rank_begin(sh.wave_tot, tid, sel);  // barrier: the previous tile's codes and wave totals have been read
        stage_tile128<NCHUNK_POS>(p, sh.codes, sh.flags, tid, q0);
        const uint32_t in_tile = rank_end(sh.wave_tot, tid, in_wave);  // barrier: the codes and the wave totals are written
        kmer128_emit_thread(p, sh.codes, tid, q0, sel, base + in_tile);
    }
}

hipError_t launch_kmers128(const Kmer128Params& p, hipStream_t stream) { return launch_tiles128(kmer128_kernel, p, p.n_tiles, stream); }
hipError_t launch_kmers128_count(const Kmer128Params& p, hipStream_t stream) { return launch_tiles128(kmer128_count_kernel, p, p.n_tiles, stream); }
hipError_t launch_kmers128_emit(const Kmer128Params& p, hipStream_t stream) { return launch_tiles128(kmer128_emit_kernel, p, p.n_tiles, stream); }

}  // namespace bl
