// bl_read_quantiles.hip — bl_select_read_counts: per-sequence quantiles (the median among them) of the counts bl_scan_kmer_counts wrote,
// by exact radix selection on the device.  Two kernels, both handing out work per sequence (bl_read_quantiles_core.hpp):
//   select_wave_kernel   one wave per sequence of at most WAVE_MAX positions, values in registers, a step is compares and ballots: no LDS,
//                        no barrier.  A longer sequence is appended to a list (the one atomic of the call: it hands out work, no value
//                        depends on the order of the list).
//   select_wg_kernel     one workgroup per listed sequence: a census pass, then one 256-bin histogram pass per 8-bit digit and quantile.
// The histograms are integer counts in LDS: their sums do not depend on the order of the adds, so the results are bit-reproducible.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"
#include "bl_read_quantiles_core.hpp"

namespace blrq {

namespace {

constexpr int WAVES = WG_TPB / 64;

__device__ __forceinline__ uint32_t wave_or(uint32_t x)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x |= __shfl_xor(x, d, 64);
    return x;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// the sequences [lo, hi) of the call's range: lanes 0 and 1 of the wave search side by side
__device__ __forceinline__ void wave_work_span(const SelectParams& p, int lane, uint64_t& lo, uint64_t& hi)
{
    unsigned long long bound = 0;
    if (lane < 2) bound = work_bound(p, lane);
    lo = __shfl(bound, 0, 64);
    hi = __shfl(bound, 1, 64);
}

__device__ __forceinline__ void write_answers(const SelectParams& p, uint64_t seq, uint32_t m, const uint32_t* answers)
{
#pragma unroll
    for (int j = 0; j < MAX_Q; ++j)  // (unrolled: the answers stay in registers)
        if ((uint32_t)j < p.n_q) p.quantiles[seq * p.n_q + j] = answers[j];
    if (p.n_kmers) p.n_kmers[seq] = m;
}

// one sequence of at most 64 * NS positions; wave-uniform control flow throughout
template <int NS>
__device__ __forceinline__ void select_in_wave(const SelectParams& p, uint64_t seq, uint64_t r0, uint32_t len, int lane)
{
    LaneVals<NS> L;
    wave_load_lane<NS>(p, r0, len, lane, L);
    uint32_t m = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) m += (uint32_t)__popcll(__ballot((L.ok >> s) & 1u));
    const uint32_t ors = wave_or(lane_or<NS>(L));
    uint32_t answers[MAX_Q] = {0, 0, 0, 0};
    if (ors) {  // (m >= 1)
        const int hb = highest_bit(ors);
#pragma unroll
        for (int j = 0; j < MAX_Q; ++j) {
            if ((uint32_t)j < p.n_q) {
                uint64_t k = rank_of(m, p.q_num[j], p.q_den[j]);
                uint32_t prefix = 0;
                for (int bit = hb; bit >= 0; --bit) {
                    uint32_t zeros = 0;
#pragma unroll
                    for (int s = 0; s < NS; ++s) zeros += (uint32_t)__popcll(__ballot(slot_in_zero_half<NS>(L, s, prefix, bit)));
                    narrow_bit(k, prefix, bit, zeros);
                }
                answers[j] = prefix;
            }
        }
    }
    if (lane == 0) write_answers(p, seq, m, answers);
}

}  // namespace

__global__ __launch_bounds__(WG_TPB) void select_wave_kernel(const SelectParams p)
{
    const int lane = threadIdx.x & 63;
    uint64_t lo, hi;
    wave_work_span(p, lane, lo, hi);
    const uint64_t wave = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    for (uint64_t seq = lo + wave; seq < hi; seq += (uint64_t)gridDim.x * WAVES) {
        uint64_t r0, len;
        if (!sequence_span(p, seq, r0, len)) continue;  // (wave-uniform: only wrong offsets get here)
        if (len > (uint64_t)WAVE_MAX) {
            if (lane == 0) {
                const unsigned long long slot = atomicAdd(p.long_count, 1ull);
                if (slot < p.long_cap) p.long_list[slot] = seq;
            }
        } else if (len <= 64u * WAVE_SLOTS_SHORT) {
            select_in_wave<WAVE_SLOTS_SHORT>(p, seq, r0, (uint32_t)len, lane);
        } else {
            select_in_wave<WAVE_SLOTS>(p, seq, r0, (uint32_t)len, lane);
        }
    }
}

namespace {

struct WgShared {
    uint32_t hist[MAX_Q][256];
    uint32_t red[2][WAVES];
    uint32_t prefix[MAX_Q];
    unsigned long long k[MAX_Q];
};

// One position of a digit pass.  Where the whole wave adds to one bin — the upper digits of real counts — one lane adds for all.
__device__ __forceinline__ void hist_add(uint32_t* hist, bool live, uint32_t digit)
{
    const unsigned long long mask = __ballot(live);
    if (mask == 0) return;
    const int leader = __builtin_ctzll(mask);
    const uint32_t lead = __shfl(digit, leader, 64);
    if (__ballot(live && digit == lead) == mask) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lead], (uint32_t)__popcll(mask));
    } else if (live) {
        atomicAdd(&hist[digit], 1u);
    }
}

__device__ __forceinline__ void digit_step(const SelectParams& p, WgShared& sh, uint64_t r0, uint64_t j, bool inside, const uint32_t* prefix, int shift)
{
    uint32_t v;
    bool ok;
    wg_fetch(p, r0, j, inside, v, ok);
    const uint32_t digit = digit_of(v, shift);
#pragma unroll
    for (int q = 0; q < MAX_Q; ++q)
        if ((uint32_t)q < p.n_q) hist_add(sh.hist[q], ok && digit_candidate(v, prefix[q], shift), digit);
}

}  // namespace

__global__ __launch_bounds__(WG_TPB) void select_wg_kernel(const SelectParams p)
{
    __shared__ WgShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long listed = *p.long_count;
    const uint64_t n_long = listed < p.long_cap ? listed : p.long_cap;
    for (uint64_t t = blockIdx.x; t < n_long; t += gridDim.x) {
        const uint64_t seq = p.long_list[t];
        uint64_t r0, len;
        if (seq >= p.n_seqs || !sequence_span(p, seq, r0, len)) continue;  // (the list is the wave kernel's: it holds what passed this test)
        const uint64_t n_steps = wg_steps(len);

        // census: the valid positions and the OR of their counts
        uint32_t m = 0, ors = 0;
        for (uint64_t step = 0; step < n_steps; ++step) {
#pragma unroll
            for (int u = 0; u < WG_UNROLL; ++u) {
                uint64_t j;
                const bool inside = wg_position(len, step, u, tid, j);
                wg_census(p, r0, j, inside, m, ors);
            }
        }
        m = wave_sum(m);
        ors = wave_or(ors);
        __syncthreads();  // the previous sequence's words have been read
        if (lane == 0) {
            sh.red[0][wv] = m;
            sh.red[1][wv] = ors;
        }
        __syncthreads();
        m = 0;
        ors = 0;
        for (int w = 0; w < WAVES; ++w) {
            m += sh.red[0][w];
            ors |= sh.red[1][w];
        }
        if ((uint32_t)tid < p.n_q) {
            sh.prefix[tid] = 0;
            sh.k[tid] = m ? rank_of(m, p.q_num[tid], p.q_den[tid]) : 0;
        }
        if (ors) {  // (uniform over the workgroup)
            for (int shift = top_shift(ors); shift >= 0; shift -= 8) {
                for (int i = tid; i < MAX_Q * 256; i += WG_TPB) (&sh.hist[0][0])[i] = 0;
                __syncthreads();
                uint32_t prefix[MAX_Q];
#pragma unroll
                for (int q = 0; q < MAX_Q; ++q) prefix[q] = sh.prefix[q < (int)p.n_q ? q : 0];
                for (uint64_t step = 0; step < n_steps; ++step) {
#pragma unroll
                    for (int u = 0; u < WG_UNROLL; ++u) {
                        uint64_t j;
                        const bool inside = wg_position(len, step, u, tid, j);
                        digit_step(p, sh, r0, j, inside, prefix, shift);
                    }
                }
                __syncthreads();
                if ((uint32_t)wv < p.n_q) {  // wave j: quantile j
                    uint32_t h[4];
#pragma unroll
                    for (int d = 0; d < 4; ++d) h[d] = sh.hist[wv][4 * lane + d];
                    const uint32_t mine = h[0] + h[1] + h[2] + h[3];  // (at most m <= 2^31)
                    uint32_t incl = mine;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const uint32_t up = __shfl_up(incl, d, 64);
                        if (lane >= d) incl += up;
                    }
                    uint64_t k = sh.k[wv];
                    uint32_t pre = sh.prefix[wv];
                    if (narrow_digit(h, incl - mine, lane, shift, k, pre)) {
                        sh.k[wv] = k;
                        sh.prefix[wv] = pre;
                    }
                }
                __syncthreads();
            }
        } else {
            __syncthreads();
        }
        if (tid == 0) {
            uint32_t answers[MAX_Q];
#pragma unroll
            for (int q = 0; q < MAX_Q; ++q) answers[q] = sh.prefix[q < (int)p.n_q ? q : 0];
            write_answers(p, seq, m, answers);
        }
    }
}

namespace {

using blh::invalid;

}  // namespace

}  // namespace blrq

extern "C" int bl_select_read_counts(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, const uint32_t* d_counts, const uint8_t* d_valid,
                                     const uint64_t* d_offsets, const uint32_t* q_num, const uint32_t* q_den, uint32_t n_q, uint32_t* d_quantiles,
                                     uint32_t* d_n_kmers)
{
    using namespace blrq;
    if (!ctx || !batch) return invalid("ctx or batch is NULL");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    const uint64_t n_bases = view.n_bases, n_seqs = view.n_seqs, read_len = view.read_len;
    if (!d_counts || !d_valid) return invalid("d_counts and d_valid are both required: what bl_scan_kmer_counts wrote for the range");
    if (!d_quantiles) return invalid("d_quantiles is NULL");
    if (!q_num || !q_den) return invalid("q_num or q_den is NULL");
    if (n_q < 1 || n_q > (uint32_t)MAX_Q) return invalid("n_q must be 1 .. 4");
    for (uint32_t j = 0; j < n_q; ++j) {
        if (q_den[j] == 0) return invalid("a quantile's q_den is 0");
        if (q_num[j] > q_den[j]) return invalid("a quantile's q_num exceeds its q_den");
    }
    uint64_t end = 0;
    BLH_OK(blh::range_end(n_bases, first, n, "a range", end));
    BLH_OK(blh::offsets_needed(d_offsets, n_seqs, read_len));
    if (end <= first) return BL_OK;  // (n_seqs >= 1 from here on)

    SelectParams p{};
    p.counts = d_counts;
    p.valid = d_valid;
    p.offsets = d_offsets;
    p.first = first;
    p.end = end;
    p.n_bases = n_bases;
    p.n_seqs = n_seqs;
    p.read_len = d_offsets ? 0 : (read_len ? read_len : n_bases);
    p.n_q = n_q;
    for (uint32_t j = 0; j < n_q; ++j) {
        p.q_num[j] = q_num[j];
        p.q_den[j] = q_den[j];
    }
    p.quantiles = d_quantiles;
    p.n_kmers = d_n_kmers;

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the context's scans in flight
    // the long sequences of a range are disjoint and each longer than WAVE_MAX
    const uint64_t by_length = (end - first) / ((uint64_t)WAVE_MAX + 1);
    p.long_cap = by_length < n_seqs ? by_length : n_seqs;
    p.long_count = static_cast<unsigned long long*>(bl_ctx_scratch(ctx, 6, 128));
    p.long_list = static_cast<uint64_t*>(bl_ctx_scratch(ctx, 4, (size_t)(p.long_cap + 1) * sizeof(uint64_t)));
    if (!p.long_count || !p.long_list) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    BLH_TRY(hipMemsetAsync(p.long_count, 0, sizeof(unsigned long long), s));
    const uint64_t wave_wgs = (n_seqs + WG_TPB / 64 - 1) / (WG_TPB / 64);
    hipLaunchKernelGGL(select_wave_kernel, dim3((unsigned)(wave_wgs < (uint64_t)WAVE_GRID_MAX ? wave_wgs : (uint64_t)WAVE_GRID_MAX)), dim3(WG_TPB), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bl_set_error(BL_ERR_HIP, (std::string("select_wave_kernel: ") + hipGetErrorString(e)).c_str());
    if (p.long_cap) {
        hipLaunchKernelGGL(select_wg_kernel, dim3((unsigned)(p.long_cap < (uint64_t)WG_GRID_MAX ? p.long_cap : (uint64_t)WG_GRID_MAX)), dim3(WG_TPB), 0, s, p);
        e = hipGetLastError();
        if (e != hipSuccess) return bl_set_error(BL_ERR_HIP, (std::string("select_wg_kernel: ") + hipGetErrorString(e)).c_str());
    }
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}
