// bl_kmers128.hip — gfx950 kernels of the 128-bit k-mer scans (k <= 64) and their launchers: the dense scan of bl_scan_kmers128 and
// the two passes of bl_scan_hash_sample128.  The per-thread bodies are in bl_kmers128_core.hpp; the tile layout is kmer_kernel's.
#include <hip/hip_runtime.h>
#include "bl_kmers128_launch.hpp"

namespace bl {

namespace {

struct Kmer128Shared {
    uint32_t codes[NCHUNK_POS];
    uint32_t flags[NCHUNK_POS];
    unsigned long long dig[5];
    uint32_t wave_tot[TPB / 64];
};

__device__ __forceinline__ unsigned long long wave_xor_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ void stage_tile(const Kmer128Params& p, Kmer128Shared& sh, int tid, int64_t q0)
{
    ScanParams lp{};  // the staging code only looks at these three fields
    lp.bases = p.bases;
    lp.n_bases = p.n_bases;
    lp.start_bits = p.start_bits;
    stage_chunk(lp, sh.codes, sh.flags, tid, q0);
    if (tid < NCHUNK_POS - TPB) stage_chunk(lp, sh.codes, sh.flags, TPB + tid, q0);
}

// the workgroup's digest into one shard line.  COUNT: slot 0 is folded here (the sampler's count comes from its prefix scan instead);
// SUM3: slot 3 is a wrapping sum (of hashes), not an XOR (of positions)
template <bool COUNT, bool SUM3>
__device__ __forceinline__ void fold_digest(const Kmer128Params& p, Kmer128Shared& sh, int tid, const Kmer128Acc& acc)
{
    __syncthreads();
    const unsigned long long c = COUNT ? wave_sum_u64(acc.cnt) : 0ull, xlo = wave_xor_u64(acc.xlo), xhi = wave_xor_u64(acc.xhi), xh = wave_xor_u64(acc.xh);
    const unsigned long long sx = SUM3 ? wave_sum_u64(acc.sx) : wave_xor_u64(acc.sx);
    if ((tid & 63) == 0) {
        if (COUNT) atomicAdd(&sh.dig[0], c);
        atomicXor(&sh.dig[1], xlo);
        atomicXor(&sh.dig[2], xh);
        if (SUM3) atomicAdd(&sh.dig[3], sx);
        else atomicXor(&sh.dig[3], sx);
        atomicXor(&sh.dig[4], xhi);
    }
    __syncthreads();
    if (tid < 5 && (COUNT || tid != 0)) {
        unsigned long long* shard = p.shards + 8 * (blockIdx.x % NSHARD);
        if (tid == 0 || (SUM3 && tid == 3)) atomicAdd(&shard[tid], sh.dig[tid]);
        else atomicXor(&shard[tid], sh.dig[tid]);
    }
}

}  // namespace

// Dense scan: workgroups stride over the tiles, no compaction.
__global__ __launch_bounds__(TPB) void kmer128_kernel(const Kmer128Params p)
{
    __shared__ Kmer128Shared sh;
    const int tid = threadIdx.x;
    Kmer128Acc acc{0, 0, 0, 0, 0};
    if (tid < 5) sh.dig[tid] = 0;
    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.origin + (int64_t)tile * H;
        __syncthreads();
        stage_tile(p, sh, tid, q0);
        __syncthreads();
        kmer128_dense_thread(p, sh.codes, sh.flags, tid, q0, acc);
    }
    fold_digest<true, true>(p, sh, tid, acc);
}

// Sampler pass 1: per lane the mask of its records, per tile their number; the digest of the records.
__global__ __launch_bounds__(TPB) void kmer128_count_kernel(const Kmer128Params p)
{
    __shared__ Kmer128Shared sh;
    const int tid = threadIdx.x;
    Kmer128Acc acc{0, 0, 0, 0, 0};
    if (tid < 5) sh.dig[tid] = 0;
    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.origin + (int64_t)tile * H;
        __syncthreads();
        stage_tile(p, sh, tid, q0);
        __syncthreads();
        const uint32_t sel = kmer128_count_thread(p, sh.codes, sh.flags, tid, q0, acc);
        p.lane_masks[(size_t)tile * TPB + tid] = (uint16_t)sel;
        const unsigned long long c = wave_sum_u64((unsigned)__builtin_popcount(sel));
        if ((tid & 63) == 0) sh.wave_tot[tid >> 6] = (uint32_t)c;
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int i = 0; i < TPB / 64; ++i) all += sh.wave_tot[i];
            p.tile_counts[tile] = all;  // the total reaches the digest through the prefix scan (tile_scan_top_kernel)
        }
    }
    fold_digest<false, false>(p, sh, tid, acc);
}

// Sampler pass 2: every tile's records at the tile's offset, lanes in order.
__global__ __launch_bounds__(TPB) void kmer128_emit_kernel(const Kmer128Params p)
{
    __shared__ Kmer128Shared sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int tile = blockIdx.x; tile < p.n_tiles; tile += gridDim.x) {
        if (p.tile_counts[tile] == 0) continue;  // uniform: the whole workgroup reads one word
        const unsigned long long base = p.tile_base[tile] + p.block_base[tile / SCAN_BLK];
        if (base >= p.capacity) continue;        // uniform as well
        const int64_t q0 = p.origin + (int64_t)tile * H;
        const uint32_t sel = p.lane_masks[(size_t)tile * TPB + tid];
        const uint32_t c = (uint32_t)__builtin_popcount(sel);
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        __syncthreads();  // the previous tile's codes and wave totals have been read
        if (lane == 63) sh.wave_tot[wv] = incl;
        stage_tile(p, sh, tid, q0);
        __syncthreads();
        uint32_t before = 0;
#pragma unroll
        for (int i = 0; i < TPB / 64; ++i)
            if (i < wv) before += sh.wave_tot[i];
        kmer128_emit_thread(p, sh.codes, tid, q0, sel, base + before + incl - c);
    }
}

// 2,048 workgroups striding over the tiles, as bl_scan_kmers launches kmer_kernel
static int grid_for(int n_tiles) { return n_tiles < 256 * 8 ? n_tiles : 256 * 8; }

hipError_t launch_kmers128(const Kmer128Params& p, hipStream_t stream)
{
    if (p.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(kmer128_kernel, dim3(grid_for(p.n_tiles)), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_kmers128_count(const Kmer128Params& p, hipStream_t stream)
{
    if (p.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(kmer128_count_kernel, dim3(grid_for(p.n_tiles)), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_kmers128_emit(const Kmer128Params& p, hipStream_t stream)
{
    if (p.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(kmer128_emit_kernel, dim3(grid_for(p.n_tiles)), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

}  // namespace bl
