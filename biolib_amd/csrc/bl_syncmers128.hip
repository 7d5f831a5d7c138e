// bl_syncmers128.hip — gfx950 kernels of bl_scan_syncmers128 (k <= 64, s <= 32, 16-byte s-mer keys) and their launchers.  The
// per-thread bodies are in bl_syncmers128_core.hpp; the tile layout is kmer_kernel's, the prefix scan between the two passes is
// launch_tile_scan (bl_launch.hpp).
#include <hip/hip_runtime.h>
#include "bl_syncmers128_launch.hpp"

namespace bl {

namespace {

struct Sync128Shared {
    uint64_t hash[SYNC128_SLOTS];  // one strand's s-mer hashes at a time
    uint32_t codes[NCHUNK_POS];
    uint32_t flags[NCHUNK_POS];
    unsigned long long dig;
    uint32_t wave_tot[TPB / 64];
};

__device__ __forceinline__ unsigned long long wave_xor_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace

// Pass 1: per lane the mask of its records, per tile their number; XOR of the records' positions.
__global__ __launch_bounds__(TPB) void sync128_count_kernel(const Sync128Params p)
{
    __shared__ Sync128Shared sh;
    const int tid = threadIdx.x;
    const bool canonical = p.km.canonical != 0;  // uniform
    unsigned long long xor_pos = 0;
    if (tid == 0) sh.dig = 0;
    ScanParams lp{};  // the staging code only looks at these three fields
    lp.bases = p.km.bases;
    lp.n_bases = p.km.n_bases;
    lp.start_bits = p.km.start_bits;
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.km.origin + (int64_t)tile * H;
        __syncthreads();  // the previous tile's hashes, codes and wave totals have been read
        stage_chunk(lp, sh.codes, sh.flags, tid, q0);
        if (tid < NCHUNK_POS - TPB) stage_chunk(lp, sh.codes, sh.flags, TPB + tid, q0);
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
        const uint32_t sel = sync128_select(p.km, tid, q0, ok, strand, hit_fwd, hit_rev, xor_pos);
        p.km.lane_masks[(size_t)tile * TPB + tid] = (uint16_t)sel;
        const uint32_t c = wave_sum_u32((uint32_t)__builtin_popcount(sel));
        if ((tid & 63) == 0) sh.wave_tot[tid >> 6] = c;
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int i = 0; i < TPB / 64; ++i) all += sh.wave_tot[i];
            p.km.tile_counts[tile] = all;  // the total reaches the digest through the prefix scan (tile_scan_top_kernel)
        }
    }
    __syncthreads();
    const unsigned long long x = wave_xor_u64(xor_pos);
    if ((tid & 63) == 0) atomicXor(&sh.dig, x);
    __syncthreads();
    if (tid == 0) atomicXor(&p.km.shards[8 * (blockIdx.x % NSHARD) + 3], sh.dig);
}

// Pass 2: every tile's records at the tile's offset, lanes in order.  Positions only: nothing is staged.
__global__ __launch_bounds__(TPB) void sync128_emit_kernel(const Sync128Params p)
{
    __shared__ uint32_t wave_tot[TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        if (p.km.tile_counts[tile] == 0) continue;  // uniform: the whole workgroup reads one word
        const unsigned long long base = p.km.tile_base[tile] + p.km.block_base[tile / SCAN_BLK];
        if (base >= p.km.capacity) continue;        // uniform as well
        const int64_t q0 = p.km.origin + (int64_t)tile * H;
        const uint32_t sel = p.km.lane_masks[(size_t)tile * TPB + tid];
        const uint32_t c = (uint32_t)__builtin_popcount(sel);
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        __syncthreads();  // the previous tile's wave totals have been read
        if (lane == 63) wave_tot[wv] = incl;
        __syncthreads();
        uint32_t before = 0;
#pragma unroll
        for (int i = 0; i < TPB / 64; ++i)
            if (i < wv) before += wave_tot[i];
        sync128_emit_thread(p.km, tid, q0, sel, base + before + incl - c);
    }
}

// 2,048 workgroups striding over the tiles, as the 128-bit k-mer kernels are launched
static int grid_for(int n_tiles) { return n_tiles < 256 * 8 ? n_tiles : 256 * 8; }

hipError_t launch_syncmers128_count(const Sync128Params& p, hipStream_t stream)
{
    if (p.km.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(sync128_count_kernel, dim3(grid_for(p.km.n_tiles)), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_syncmers128_emit(const Sync128Params& p, hipStream_t stream)
{
    if (p.km.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(sync128_emit_kernel, dim3(grid_for(p.km.n_tiles)), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

}  // namespace bl
