// bl_minimizers128.hip — gfx950 kernels of bl_scan_minimizers128 (window minimizers of k-mers up to k = 64, 16-byte keys) and their
// launchers.  The per-thread bodies are in bl_minimizers128_core.hpp; the prefix scan between the two passes is launch_tile_scan
// (bl_launch.hpp).
#include <hip/hip_runtime.h>
#include "bl_minimizers128_launch.hpp"

namespace bl {

namespace {

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

// MIN128_NCHUNK chunks from r0 = q0 - 16 on: the chunk in front of the tile is staged like any other (zeros before the batch)
__device__ __forceinline__ void stage_tile(const Kmer128Params& p, uint32_t* codes, uint32_t* flags, int tid, int64_t r0)
{
    ScanParams lp{};  // the staging code only looks at these three fields
    lp.bases = p.bases;
    lp.n_bases = p.n_bases;
    lp.start_bits = p.start_bits;
    stage_chunk(lp, codes, flags, tid, r0);
    if (tid < MIN128_NCHUNK - TPB) stage_chunk(lp, codes, flags, TPB + tid, r0);
}

}  // namespace

// Pass 1: per lane the mask of its records and their offsets, per tile their number; the digest of the records.
__global__ __launch_bounds__(TPB) void min128_count_kernel(const Min128Params p)
{
    __shared__ Min128Shared sh;
    const int tid = threadIdx.x;
    Kmer128Acc acc{0, 0, 0, 0, 0};
    if (tid < 5) sh.dig[tid] = 0;
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const int64_t r0 = p.km.origin + (int64_t)tile * H - 16;
        __syncthreads();  // the previous tile's hashes, codes and wave totals have been read
        stage_tile(p.km, sh.codes, sh.flags, tid, r0);
        __syncthreads();
        min128_hash_thread(p, sh.codes, sh.flags, sh.hash, sh.valid, tid, r0);
        __syncthreads();
        Min128Offs offs;
        const uint32_t sel = min128_window_thread(p, sh.hash, sh.valid, tid, r0, offs);
        min128_digest_thread(p.km, sh.codes, sh.hash, tid, r0, sel, offs, acc);
        if (p.km.lane_masks) {  // uniform: a count-only call has no second pass
            p.km.lane_masks[(size_t)tile * TPB + tid] = (uint16_t)sel;
            min128_offs_store(p.lane_offs, tile, tid, offs);
        }
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
    const unsigned long long xlo = wave_xor_u64(acc.xlo), xhi = wave_xor_u64(acc.xhi), xh = wave_xor_u64(acc.xh), sx = wave_xor_u64(acc.sx);
    if ((tid & 63) == 0) {
        atomicXor(&sh.dig[1], xlo);
        atomicXor(&sh.dig[2], xh);
        atomicXor(&sh.dig[3], sx);
        atomicXor(&sh.dig[4], xhi);
    }
    __syncthreads();
    if (tid >= 1 && tid < 5) atomicXor(&p.km.shards[8 * (blockIdx.x % NSHARD) + tid], sh.dig[tid]);
}

// Pass 2: every tile's records at the tile's offset, lanes in order.
__global__ __launch_bounds__(TPB) void min128_emit_kernel(const Min128Params p)
{
    __shared__ Min128EmitShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        if (p.km.tile_counts[tile] == 0) continue;  // uniform: the whole workgroup reads one word
        const unsigned long long base = p.km.tile_base[tile] + p.km.block_base[tile / SCAN_BLK];
        if (base >= p.km.capacity) continue;        // uniform as well
        const int64_t r0 = p.km.origin + (int64_t)tile * H - 16;
        const uint32_t sel = p.km.lane_masks[(size_t)tile * TPB + tid];
        const Min128Offs offs = min128_offs_load(p.lane_offs, tile, tid);
        const uint32_t c = (uint32_t)__builtin_popcount(sel);
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        __syncthreads();  // the previous tile's codes and wave totals have been read
        if (lane == 63) sh.wave_tot[wv] = incl;
        stage_tile(p.km, sh.codes, sh.flags, tid, r0);
        __syncthreads();
        uint32_t before = 0;
#pragma unroll
        for (int i = 0; i < TPB / 64; ++i)
            if (i < wv) before += sh.wave_tot[i];
        min128_emit_thread(p.km, sh.codes, tid, r0, sel, offs, base + before + incl - c);
    }
}

// 2,048 workgroups striding over the tiles, as the 128-bit k-mer kernels are launched
static int grid_for(int n_tiles) { return n_tiles < 256 * 8 ? n_tiles : 256 * 8; }

hipError_t launch_minimizers128_count(const Min128Params& p, hipStream_t stream)
{
    if (p.km.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(min128_count_kernel, dim3(grid_for(p.km.n_tiles)), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_minimizers128_emit(const Min128Params& p, hipStream_t stream)
{
    if (p.km.n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(min128_emit_kernel, dim3(grid_for(p.km.n_tiles)), dim3(TPB), 0, stream, p);
    return hipGetLastError();
}

}  // namespace bl
