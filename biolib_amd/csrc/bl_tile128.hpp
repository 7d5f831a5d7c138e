// bl_tile128.hpp — what the gfx950 tile kernels of the 128-bit scans share as a workgroup (HIP only; bl_kmers128.hip, bl_syncmers128.hip,
// bl_minimizers128.hip): the wave reductions, the staging of a tile's chunks, the end of pass 1 (a tile's record count), the head and the
// rank of pass 2 (where a lane's records go), the digest fold into a shard line, and the launch over the tiles.  Every barrier these
// kernels have outside their own phases is in here.  The per-thread bodies are in the *_core.hpp files; the Shared structs stay with the
// kernels: their LDS sizes are part of each kernel's occupancy plan.
#pragma once
#include <hip/hip_runtime.h>
#include "bl_kmers128_core.hpp"

namespace bl {

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

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// NCHUNK chunks (TPB < NCHUNK <= 2 TPB) from position r0 on, one or two per lane.  The caller's barriers stand around it.
template <int NCHUNK>
__device__ __forceinline__ void stage_tile128(const Kmer128Params& km, uint32_t* codes, uint32_t* flags, int tid, int64_t r0)
{
    static_assert(NCHUNK > TPB && NCHUNK <= 2 * TPB, "one chunk per lane and a halo");
    const ScanParams lp = kmer128_staging_params(km);
    stage_chunk(lp, codes, flags, tid, r0);
    if (tid < NCHUNK - TPB) stage_chunk(lp, codes, flags, TPB + tid, r0);
}

// End of pass 1: the lane's record mask to pass 2, the tile's number of records to the prefix scan (a tile has at most H = 4,096).
// One barrier; wave_tot is free again after the next one (the one in front of the next tile's staging).
__device__ __forceinline__ void publish_tile_count(const Kmer128Params& km, uint32_t* wave_tot, int tile, int tid, uint32_t sel)
{
    if (km.lane_masks) km.lane_masks[(size_t)tile * TPB + tid] = (uint16_t)sel;  // uniform: a count-only call has no second pass
    const uint32_t c = wave_sum_u32((uint32_t)__builtin_popcount(sel));
    if ((tid & 63) == 0) wave_tot[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t all = 0;
#pragma unroll
        for (int i = 0; i < TPB / 64; ++i) all += wave_tot[i];
        km.tile_counts[tile] = all;  // the total reaches the digest through the prefix scan (tile_scan_top_kernel)
    }
}

// Head of pass 2: the record index from which the tile stores its records; at or beyond km.capacity (all ones: a tile without records) it
// stores none.  Uniform: the whole workgroup reads the same words.
__device__ __forceinline__ unsigned long long tile_emit_base(const Kmer128Params& km, int tile)
{
    if (km.tile_counts[tile] == 0) return ~0ull;
    return km.tile_base[tile] + km.block_base[tile / SCAN_BLK];
}

// Rank of pass 2, in two halves with a barrier each: what the caller stages into LDS for the tile goes between them.
// rank_begin: the number of records in the lanes of this wave in front of this one.  Its barrier: the previous tile's codes and wave
// totals have been read.
__device__ __forceinline__ uint32_t rank_begin(uint32_t* wave_tot, int tid, uint32_t sel)
{
    const int lane = tid & 63;
    const uint32_t c = (uint32_t)__builtin_popcount(sel);
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();
    if (lane == 63) wave_tot[tid >> 6] = incl;
    return incl - c;
}

// rank_end: the number of records of the tile in front of the lane's.  Its barrier: the wave totals (and the caller's staging) are written.
__device__ __forceinline__ uint32_t rank_end(const uint32_t* wave_tot, int tid, uint32_t in_wave)
{
    __syncthreads();
    const int wv = tid >> 6;
    uint32_t before = 0;
#pragma unroll
    for (int i = 0; i < TPB / 64; ++i)
        if (i < wv) before += wave_tot[i];
    return before + in_wave;
}

// The five words of a shard line, in the order of bl_result: count, XOR of low words, XOR of hashes, sum of hashes | XOR of positions,
// XOR of high words.
constexpr unsigned DIG_COUNT = 1u << 0, DIG_LO = 1u << 1, DIG_HASH = 1u << 2, DIG_POS = 1u << 3, DIG_HI = 1u << 4;

// dig: the kernel's LDS words of the fold, one per slot from the lowest live slot to the highest (digest_word: a slot's word).  Zeroed at
// the top of the kernel: any barrier orders that in front of the fold's atomics.
constexpr int digest_word(unsigned live, int slot) { return slot - __builtin_ctz(live); }
constexpr int digest_words(unsigned live) { return 32 - __builtin_clz(live) - __builtin_ctz(live); }

template <unsigned LIVE>
__device__ __forceinline__ void zero_digest128(unsigned long long* dig, int tid)
{
    if (tid < digest_words(LIVE)) dig[tid] = 0;
}

// The workgroup's digest into one shard line.  LIVE: the slots this kernel folds (a two-pass kernel's count comes from the prefix scan
// instead); SUMS: those of them that are wrapping sums, the others are XORs.  Nothing is reduced and no atomic is issued for a slot that
// is not live.  After the kernel's last tile, in every lane.
template <unsigned LIVE, unsigned SUMS>
__device__ __forceinline__ void fold_digest128(unsigned long long* shards, unsigned long long* dig, int tid, const Kmer128Acc& acc)
{
    static_assert(LIVE != 0 && LIVE < 32u && (SUMS & ~LIVE) == 0, "five slots; a sum is a live slot");
    const unsigned long long in[5] = {acc.cnt, acc.xlo, acc.xh, acc.sx, acc.xhi};  // in slot order
    unsigned long long red[5];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 5; ++s)
        if ((LIVE >> s) & 1u) red[s] = ((SUMS >> s) & 1u) ? wave_sum_u64(in[s]) : wave_xor_u64(in[s]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int s = 0; s < 5; ++s)
            if ((LIVE >> s) & 1u) {
                if ((SUMS >> s) & 1u) atomicAdd(&dig[digest_word(LIVE, s)], red[s]);
                else atomicXor(&dig[digest_word(LIVE, s)], red[s]);
            }
    }
    __syncthreads();
    const int slot = tid + __builtin_ctz(LIVE);  // one lane per word
    if (tid < digest_words(LIVE) && ((LIVE >> slot) & 1u)) {
        unsigned long long* word = shards + 8 * (blockIdx.x % NSHARD) + slot;
        if ((SUMS >> slot) & 1u) atomicAdd(word, dig[tid]);
        else atomicXor(word, dig[tid]);
    }
}

// 2,048 workgroups striding over the tiles, as bl_scan_kmers launches kmer_kernel
constexpr int TILE_GRID_MAX = 256 * 8;
inline int grid_for(int n_tiles) { return n_tiles < TILE_GRID_MAX ? n_tiles : TILE_GRID_MAX; }

// a kernel that takes one params struct, over n_tiles tiles
template <typename Params>
hipError_t launch_tiles128(void (*kernel)(const Params), const Params& p, int n_tiles, hipStream_t stream)
{
    if (n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(grid_for(n_tiles)), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

}  // namespace bl
