// bl_adapters.hip — bl_scan_read_adapters: poly tails, read-through between mates and 3' adapters cut from every read of a batch (what
// fastp, cutadapt -a --no-indels and Trimmomatic do besides quality trimming).  The per-lane bodies are in bl_adapters_core.hpp.
// One kernel; a wave takes a read at a time, or a pair of mates under BL_ADAPTERS_PAIRED:
//   stage    the wave puts a block of 1,024 positions of its read into its own LDS as 16-base chunks of 2-bit codes and invalid bits, from
//            the batch's packed copy (ASCII where a chunk is bad or there is no copy); a read of up to 1,024 bases is staged once
//   poly     a lane per base from the 3' end, 64 at a time: the suffix count is a ballot and a popcount, the stop the ballot's top bit
//   pair     both mates' heads (<= 512 bases) and the reverse complement of the second staged; a lane per insert size I, 64 sizes at
//            a time from the largest down, the answer the first lane of a ballot
//   adapter  a lane per position p, all adapters at it (scalar words of the kernel's arguments); the best (matches, p, adapter) is a
//            packed key, the maximum over the wave by shuffles
// LDS holds staged bases and lane 0's statistics, each wave its own; the only atomics are the integer sums of the statistics on striped
// counters: no atomic and no LDS decides a value or a place.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/biolib_amd.h"
#include "bl_adapters_core.hpp"
#include "bl_host.hpp"

static_assert(sizeof(bla::Rule) == sizeof(bl_adapter_rule) && sizeof(bla::Record) == sizeof(bl_read_adapters) && sizeof(bl_read_adapters) == 32,
              "the header's structs");
static_assert(offsetof(bla::Rule, min_len) == offsetof(bl_adapter_rule, min_len) && offsetof(bla::Rule, min_overlap) == offsetof(bl_adapter_rule, min_overlap) &&
                  offsetof(bla::Record, cut) == offsetof(bl_read_adapters, cut),
              "the header's layouts");
static_assert(BL_MAX_ADAPTERS == bla::MAX_ADAPTERS && BL_ADAPTER_MAX_LEN == bla::ADAPTER_MAX && BL_ADAPTER_PAIR_MAX_LEN == bla::PAIR_MAX &&
                  BL_ADAPT_POLY_BEFORE == bla::CUT_POLY_BEFORE && BL_ADAPT_PAIR == bla::CUT_PAIR && BL_ADAPT_ADAPTER == bla::CUT_ADAPTER &&
                  BL_ADAPT_POLY_AFTER == bla::CUT_POLY_AFTER && BL_ADAPT_TOO_SHORT == bla::CUT_TOO_SHORT && BL_ADAPT_PAIR_SKIPPED == bla::CUT_PAIR_SKIPPED &&
                  (uint32_t)BL_ADAPTERS_PAIRED == bla::FLAG_PAIRED,
              "the header's constants");
static_assert(sizeof(bl_adapter_stats) == 24 * sizeof(uint64_t), "bl_adapter_stats is 24 words");

namespace bla {

namespace {

// what a wave keeps in LDS
struct WaveStage {
    uint32_t codes[STAGE_CHUNKS], inv[STAGE_CHUNKS];                                              // the block of the read
    uint32_t r1_codes[PAIR_CHUNKS], r1_inv[PAIR_CHUNKS], r2_codes[PAIR_CHUNKS], r2_inv[PAIR_CHUNKS];  // step 2: the mates' heads
    uint32_t rc_codes[PAIR_CHUNKS], rc_inv[PAIR_CHUNKS];                                          // and the second's reverse complement
    unsigned long long counts[N_COUNTERS];  // the wave's part of the statistics, lane 0's to add to (19 counters in registers cost a wave per SIMD)
};

// the wave's lanes have written its LDS / are about to overwrite what others still read
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One read by one wave.  Everything but the lane's own position is uniform over the wave.
struct ReadPass {
    const AdapterParams& p;
    WaveStage& s;
    const int lane;
    uint64_t first, L;
    uint64_t staged;  // the block in s.codes / s.inv, ~0: none

    __device__ __forceinline__ ReadPass(const AdapterParams& p_, WaveStage& s_, int lane_, uint64_t i) : p(p_), s(s_), lane(lane_), staged(~0ull)
    {
        blsel::read_extent(p.offsets, p.read_len, p.n_bases, i, first, L);
    }

    __device__ __forceinline__ void stage(uint64_t block)
    {
        if (block == staged) return;
        wave_sync();
        for (int c = lane; c < STAGE_CHUNKS; c += 64) {
            uint32_t code, inv;
            stage_chunk(p, first, L, block * BLOCK_CHUNKS + (uint64_t)c, code, inv);
            s.codes[c] = code;
            s.inv[c] = inv;
        }
        wave_sync();
        staged = block;
    }

    // steps 1 and 4 on [b, e), e > b: the new end
    __device__ __forceinline__ uint64_t poly(uint64_t b, uint64_t e, uint32_t mask)
    {
        const KRule& r = p.rule;
        uint64_t best = e;
        for (uint32_t X = 0; X < 4; ++X) {
            if (!((mask >> X) & 1u)) continue;
            uint64_t carry = 0, n = e - b, left = e;
            for (uint64_t q0 = (e - 1) & ~63ull;; q0 -= 64) {
                stage(q0 / BLOCK);
                const uint64_t pos = q0 + (uint64_t)lane;
                const bool active = pos >= b && pos < e;
                const uint32_t code = active ? base_at(s.codes, s.inv, (uint32_t)(pos % BLOCK)) : 4u;
                const uint64_t not_x = __ballot(active && code != X);
                const uint64_t stops = __ballot(active && poly_stops(r, e - pos, poly_count(carry, not_x, lane)));
                const uint64_t is_x = __ballot(active && code == X);
                if (poly_join(stops, is_x, q0, e, n, left) || q0 <= b) break;
                carry += (uint64_t)__builtin_popcountll(not_x);
            }
            if (n >= r.poly_min_len && left < best) best = left;
        }
        return best;
    }

    // step 3 on [b, e): the best candidate's key, 0 for none
    __device__ __forceinline__ uint64_t adapters(uint64_t b, uint64_t e)
    {
        const KRule& r = p.rule;
        uint64_t key = 0;
        if (e <= b) return 0;
        for (uint64_t block = b / BLOCK; block <= (e - 1) / BLOCK; ++block) {
            stage(block);
            const uint64_t lo = b > block * BLOCK ? b : block * BLOCK, hi = e < (block + 1) * BLOCK ? e : (block + 1) * BLOCK;
            for (uint64_t pos = lo + (uint64_t)lane; pos < hi; pos += 64) {
                for (uint32_t a = 0; a < r.n_adapters; ++a) {
                    const uint32_t O = r.min_overlap < r.adapter_len[a] ? r.min_overlap : r.adapter_len[a];
                    if (pos + O > e) continue;
                    int o, m;
                    const uint64_t k = adapter_key(r, (int)a, s.codes, s.inv, (uint32_t)(pos - block * BLOCK), pos, e, o, m);
                    key = k > key ? k : key;
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)key, d, 64);
            key = other > key ? other : key;
        }
        return key;
    }

    // the four steps; insert, pair_mismatches and skipped are step 2's answer for the pair
    __device__ __forceinline__ void run(uint64_t i, bool paired, uint32_t insert, uint32_t pair_mismatches, bool skipped, unsigned long long* counts)
    {
        bool input_empty;
        Outcome o = read_steps(*this, p, i, L, paired, insert, pair_mismatches, skipped, input_empty);
        if (lane != 0) return;
        uint64_t sb, se;
        finish_read(p.rule, o, input_empty, L, sb, se, counts);
        if (p.out_records) {
            const Record rec = make_record(o);
            const uint4* w = reinterpret_cast<const uint4*>(&rec);
            uint4* out = reinterpret_cast<uint4*>(p.out_records + i);
            out[0] = w[0];
            out[1] = w[1];
        }
        if (p.out_spans) *reinterpret_cast<uint4*>(p.out_spans + 2 * i) = make_uint4((uint32_t)sb, (uint32_t)(sb >> 32), (uint32_t)se, (uint32_t)(se >> 32));
    }
};

// step 2 for the mates i and i + 1: the insert size (0: none) and its mismatches; skipped: the pair is too long to be tested
__device__ __forceinline__ void pair_step(const AdapterParams& p, WaveStage& s, int lane, uint64_t i, uint32_t& insert, uint32_t& mismatches, bool& skipped)
{
    const KRule& r = p.rule;
    insert = mismatches = 0;
    uint64_t f1, L1, f2, L2;
    blsel::read_extent(p.offsets, p.read_len, p.n_bases, i, f1, L1);
    blsel::read_extent(p.offsets, p.read_len, p.n_bases, i + 1, f2, L2);
    const uint64_t shorter = L1 < L2 ? L1 : L2;
    skipped = shorter > (uint64_t)PAIR_MAX;
    if (skipped || shorter < r.pair_min_overlap) return;
    const int M = (int)shorter, least = (int)r.pair_min_overlap;
    wave_sync();
    if (lane < PAIR_CHUNKS) {
        uint32_t code, inv;
        stage_chunk(p, f1, L1, (uint64_t)lane, code, inv);
        s.r1_codes[lane] = code;
        s.r1_inv[lane] = inv;
        stage_chunk(p, f2, L2, (uint64_t)lane, code, inv);
        s.r2_codes[lane] = code;
        s.r2_inv[lane] = inv;
    }
    wave_sync();
    if (lane < PAIR_CHUNKS) {
        uint32_t code, inv;
        reverse_chunk(s.r2_codes, s.r2_inv, M, lane, code, inv);
        s.rc_codes[lane] = code;
        s.rc_inv[lane] = inv;
    }
    wave_sync();
    for (int top = M; top >= least; top -= 64) {  // lane l asks for I = top - l
        const int I = top - lane;
        const bool asked = I >= least;
        const uint32_t d = asked ? pair_diff(s.r1_codes, s.r1_inv, s.rc_codes, s.rc_inv, M, I, r.pair_max_diff) : 0u;
        const uint64_t yes = __ballot(asked && pair_qualifies(r, I, d));
        if (yes) {
            const int src = __builtin_ctzll(yes);
            insert = (uint32_t)(top - src);
            mismatches = __shfl(d, src, 64);
            return;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(TPB) void adapters_kernel(const AdapterParams p)
{
    __shared__ WaveStage stages[TPB / 64];
    WaveStage& s = stages[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const bool paired = (p.rule.flags & FLAG_PAIRED) != 0;
    const uint64_t per = paired ? 2 : 1, n_units = p.n_seqs / per, n_waves = (uint64_t)gridDim.x * (TPB / 64);
    unsigned long long* counts = p.counters ? s.counts : nullptr;  // lane 0's
    if (counts) {
        if (lane < N_COUNTERS) counts[lane] = 0;
        wave_sync();
    }
    for (uint64_t u = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); u < n_units; u += n_waves) {
        uint32_t insert = 0, mismatches = 0;
        bool skipped = false;
        if (paired) pair_step(p, s, lane, 2 * u, insert, mismatches, skipped);
        for (uint64_t i = per * u; i < per * u + per; ++i) {
            ReadPass pass(p, s, lane, i);
            pass.run(i, paired, insert, mismatches, skipped, counts);
        }
    }
    if (counts) {  // integer sums: the order of the adds does not matter
        wave_sync();
        if (lane < N_COUNTERS && counts[lane]) atomicAdd(&p.counters[(blockIdx.x % STRIPES) * STRIPE_WORDS + lane], counts[lane]);
    }
}

namespace {

using blh::invalid;

constexpr uint64_t GRID_MAX = 1u << 16;  // workgroups: a wave then walks its reads in steps of 2^18

}  // namespace

}  // namespace bla

extern "C" int bl_scan_read_adapters(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const uint64_t* d_spans_in, const bl_adapter_rule* rule,
                                     bl_read_adapters* d_records, uint64_t* d_spans, bl_adapter_stats* stats)
{
    using namespace bla;
    if (!ctx || !batch || !rule) return invalid("ctx, batch or rule is NULL");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    BLH_OK(blh::offsets_needed(d_offsets, view.n_seqs, view.read_len));
    Rule r;
    static_assert(sizeof(r) == sizeof(*rule), "one layout");
    std::memcpy(&r, rule, sizeof(r));
    if (const char* what = rule_error(r, view.n_seqs)) return invalid(what);
    if (blh::misaligned16(d_records) || blh::misaligned16(d_spans) || blh::misaligned16(d_spans_in))
        return invalid("d_records, d_spans and d_spans_in must be 16-byte aligned");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (view.n_seqs == 0) return BL_OK;

    AdapterParams p{};
    pack_rule(r, p.rule);
    p.bases = view.bases;
    p.n_bases = view.n_bases;
    p.offsets = d_offsets;
    p.read_len = d_offsets ? 0 : (view.read_len ? view.read_len : (view.n_bases ? view.n_bases : 1));
    p.n_seqs = view.n_seqs;
    BLH_OK(bl_batch_packed_view(ctx, batch, &p.codes_packed, &p.chunk_bad));
    p.spans_in = d_spans_in;
    p.out_records = reinterpret_cast<Record*>(d_records);
    p.out_spans = d_spans;

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the context's scans in flight and the calls that write the input spans
    unsigned long long stripes[STRIPES * STRIPE_WORDS] = {};
    if (stats) {
        p.counters = static_cast<unsigned long long*>(bl_ctx_scratch(ctx, 6, sizeof(stripes)));
        if (!p.counters) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        BLH_TRY(hipMemsetAsync(p.counters, 0, sizeof(stripes), s));
    }
    const uint64_t n_units = (r.flags & FLAG_PAIRED) ? p.n_seqs / 2 : p.n_seqs, wgs = (n_units + TPB / 64 - 1) / (TPB / 64);
    hipLaunchKernelGGL(adapters_kernel, dim3((unsigned)(wgs < GRID_MAX ? wgs : GRID_MAX)), dim3(TPB), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bl_set_error(BL_ERR_HIP, (std::string("adapters_kernel: ") + hipGetErrorString(e)).c_str());
    if (!stats) return BL_OK;
    BLH_TRY(hipMemcpyAsync(stripes, p.counters, sizeof(stripes), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    uint64_t host[N_COUNTERS] = {};
    for (int i = 0; i < STRIPES; ++i)
        for (int k = 0; k < N_COUNTERS; ++k) host[k] += stripes[i * STRIPE_WORDS + k];
    stats->n_reads = host[C_READS];
    stats->n_reads_cut = host[C_CUT];
    stats->n_reads_kept = host[C_KEPT];
    stats->n_bases = host[C_BASES_IN];
    stats->n_bases_kept = host[C_BASES_KEPT];
    stats->n_poly_before = host[C_BIT0];
    stats->n_pair = host[C_BIT0 + 1];
    stats->n_adapter = host[C_BIT0 + 2];
    stats->n_poly_after = host[C_BIT0 + 3];
    stats->n_too_short = host[C_BIT0 + 4];
    stats->n_pair_skipped = host[C_BIT0 + 5];
    for (int a = 0; a < MAX_ADAPTERS; ++a) stats->per_adapter[a] = host[C_ADAPTER0 + a];
    return BL_OK;
}
