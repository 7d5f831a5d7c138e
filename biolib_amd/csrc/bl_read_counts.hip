// bl_read_counts.hip — bl_scan_read_counts (entry in bl_capi.hip): the fused scan of bl_lookup.hip with the looked-up counts reduced per
// sequence on the chip, one 48-byte record per read.  Two kernels: the identity fill of the records a call touches (INIT) and the scan.
// The scan keeps scan_counts_kernel's position tiling (bl_tile128.hpp); the per-thread bodies, the segment rules and the index search
// are in bl_read_counts_core.hpp.  The reduction is per wave, through shuffles: no LDS and no barrier beyond the tile's two.
#include <hip/hip_runtime.h>

#include "bl_read_counts_launch.hpp"
#include "bl_tile128.hpp"

namespace blrc {

namespace {

struct ReadCountShared {
    uint32_t codes[bl::NCHUNK_POS];
    uint32_t flags[bl::NCHUNK_POS];
    unsigned long long dig[5];
};

constexpr unsigned SCAN_SLOTS = bl::DIG_COUNT | bl::DIG_LO | bl::DIG_HASH | bl::DIG_POS | bl::DIG_HI;

// the part of lane - d (its own for the lanes below d)
__device__ __forceinline__ Part shfl_up_part(const Part& a, int d)
{
    Part r;
    r.n = __shfl_up(a.n, d, 64);
    r.found = __shfl_up(a.found, d, 64);
    r.solid = __shfl_up(a.solid, d, 64);
    r.mn = __shfl_up(a.mn, d, 64);
    r.mx = __shfl_up(a.mx, d, 64);
    r.wb = __shfl_up(a.wb, d, 64);
    r.we = __shfl_up(a.we, d, 64);
    r.sum = __shfl_up((unsigned long long)a.sum, d, 64);
    return r;
}

}  // namespace

// one thread per touched record; thread 0 of every workgroup finds the span
__global__ __launch_bounds__(ITPB) void read_counts_init_kernel(const ReadCountParams p)
{
    __shared__ uint64_t span[2];
    if (threadIdx.x == 0) touched_span(p, span[0], span[1]);
    __syncthreads();
    const uint64_t lo = span[0], hi = span[1];  // both below n_seqs
    if (lo > hi) return;                        // (only a wrong offsets array does that)
    for (uint64_t i = (uint64_t)blockIdx.x * ITPB + threadIdx.x; i <= hi - lo; i += (uint64_t)gridDim.x * ITPB) p.records[lo + i] = identity_record();
}

__global__ __launch_bounds__(bl::TPB) void read_counts_kernel(const ReadCountParams p)
{
    __shared__ ReadCountShared sh;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = bl::wave_index(tid);
    bl::Kmer128Acc acc{0, 0, 0, 0, 0};
    bl::zero_digest128<SCAN_SLOTS>(sh.dig, tid);
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.km.origin + (int64_t)tile * bl::H;
        __syncthreads();  // the previous tile's codes and flags have been read
        bl::stage_tile128<bl::NCHUNK_POS>(p.km, sh.codes, sh.flags, tid, q0);
        // the wave's first and last sequence: lanes 0 and 1 bisect side by side (nothing to find without offsets)
        uint64_t bound = 0;
        if (p.offsets && lane < 2) bound = seq_of(p.offsets, wave_bound_position(p, q0, wv, lane), 0, p.n_seqs - 1);
        const uint64_t lo_seq = __shfl((unsigned long long)bound, 0, 64), hi_seq = __shfl((unsigned long long)bound, 1, 64);
        __syncthreads();
        uint32_t start16;
        Part head, run;
        read_counts_lane(p, sh.codes, sh.flags, tid, q0, lo_seq, hi_seq, acc, start16, head, run);
        const int seg = wave_seg_head(__ballot(start16 != 0), lane);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Part theirs = shfl_up_part(run, d);
            if (wave_scan_takes(lane, d, seg)) run = merge(theirs, run);
        }
        Part below = shfl_up_part(run, 1);
        if (lane == 0) below = identity_part();
        wave_close(p, tid, q0, start16, head, run, below, lo_seq, hi_seq);
    }
    bl::fold_digest128<SCAN_SLOTS, bl::DIG_COUNT | bl::DIG_HASH | bl::DIG_POS>(p.km.shards, sh.dig, tid, acc);
}

hipError_t launch_read_counts_init(const ReadCountParams& p, hipStream_t stream)
{
    const uint64_t wg = (p.n_seqs + ITPB - 1) / ITPB;
    hipLaunchKernelGGL(read_counts_init_kernel, dim3((unsigned)(wg < (uint64_t)INIT_GRID_MAX ? wg : (uint64_t)INIT_GRID_MAX)), dim3(ITPB), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_read_counts(const ReadCountParams& p, hipStream_t stream) { return bl::launch_tiles128(read_counts_kernel, p, p.km.n_tiles, stream); }

}  // namespace blrc
