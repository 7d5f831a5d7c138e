// bl_quality.hip — bl_scan_read_quality: per-read trimming and filtering by the quality values of an indexed FASTQ text (the step fastp,
// Trimmomatic and cutadapt -q do first), and bl_spans_intersect, which joins its spans with others and with mate pairing.  The per-lane
// bodies are in bl_quality_core.hpp.  One kernel hands out reads four at a time to a wave and has three bodies:
//   short   the four reads hold at most SHORT_MAX positions each: a group of 16 lanes per read, 16 positions per lane, in registers
//   wave    one read of at most WAVE_MAX positions at a time over the 64 lanes, in registers
//   sweep   a longer read chunk by chunk of WAVE_MAX positions with a carry; every step is one sweep (the span is decided, then the
//           statistics are taken), stopped where it is decided
// A step is a scan: within a lane over its 16 values, across the lanes of the group by ballots (first, last) and shuffle scans
// (sums in front or behind, the maximum with its tie rule).  No LDS but the 94-word error table, no barrier but the one behind its
// fill, no atomic but the integer sums of the statistics on striped counters: no atomic decides a value or a place.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"
#include "bl_quality_core.hpp"

static_assert(sizeof(blq::Rule) == sizeof(bl_quality_rule) && sizeof(blq::Record) == sizeof(bl_read_quality) && sizeof(bl_read_quality) == 48,
              "the header's structs");
static_assert((uint32_t)BL_SPANS_PAIRED == blq::SPANS_PAIRED && BL_QFAIL_MIN_LEN == blq::FAIL_MIN_LEN && BL_QFAIL_MAX_LEN == blq::FAIL_MAX_LEN &&
                  BL_QFAIL_AMBIGUOUS == blq::FAIL_AMBIGUOUS && BL_QFAIL_LOW == blq::FAIL_LOW && BL_QFAIL_MEAN == blq::FAIL_MEAN && BL_QFAIL_EE == blq::FAIL_EE,
              "the header's constants");
static_assert(sizeof(bl_quality_stats) == 12 * sizeof(uint64_t), "bl_quality_stats is 12 words");

namespace blq {

namespace {

// the G lanes of a group: ballots, shuffles and scans among them.  Control flow is uniform over a group, not over the wave.
template <int G>
struct Group {
    int gl;     // the lane's place in its group
    int first;  // the group's first lane of the wave

    __device__ __forceinline__ explicit Group(int lane) : gl(lane & (G - 1)), first(lane & ~(G - 1)) {}
    __device__ __forceinline__ uint64_t ballot(bool x) const
    {
        const uint64_t b = __ballot(x);
        return G == 64 ? b : (b >> first) & ((1ull << (G & 63)) - 1ull);
    }
    template <typename T>
    __device__ __forceinline__ T shfl(T x, int src) const
    {
        return __shfl(x, src, G);
    }
    // the sum of x over the lanes in front of this one / behind it
    __device__ __forceinline__ int32_t sum_in_front(int32_t x) const
    {
        int32_t incl = x;
#pragma unroll
        for (int d = 1; d < G; d <<= 1) {
            const int32_t up = __shfl_up(incl, d, G);
            if (gl >= d) incl += up;
        }
        return incl - x;
    }
    __device__ __forceinline__ int32_t sum_behind(int32_t x) const
    {
        int32_t incl = x;
#pragma unroll
        for (int d = 1; d < G; d <<= 1) {
            const int32_t down = __shfl_down(incl, d, G);
            if (gl + d < G) incl += down;
        }
        return incl - x;
    }
    template <typename T>
    __device__ __forceinline__ T sum(T x) const
    {
#pragma unroll
        for (int d = G / 2; d >= 1; d >>= 1) x += __shfl_xor(x, d, G);
        return x;
    }
    __device__ __forceinline__ long long max(long long x) const
    {
#pragma unroll
        for (int d = G / 2; d >= 1; d >>= 1) {
            const long long y = __shfl_xor(x, d, G);
            x = y > x ? y : x;
        }
        return x;
    }
    __device__ __forceinline__ uint32_t min(uint32_t x) const
    {
#pragma unroll
        for (int d = G / 2; d >= 1; d >>= 1) {
            const uint32_t y = __shfl_xor(x, d, G);
            x = y < x ? y : x;
        }
        return x;
    }
    __device__ __forceinline__ uint32_t max(uint32_t x) const
    {
#pragma unroll
        for (int d = G / 2; d >= 1; d >>= 1) {
            const uint32_t y = __shfl_xor(x, d, G);
            x = y > x ? y : x;
        }
        return x;
    }
};

// One read by one group.  RESIDENT: the read fits the group's G * 16 positions; every lane loads its values once and every sweep
// below is one step.  Otherwise the sweeps walk the read's chunks of G * 16 positions and load as they go.
template <int G, bool RESIDENT>
struct ReadPass {
    static constexpr uint64_t CH = (uint64_t)G * LANE;
    const QualityParams& p;
    const Group<G> g;
    Place d;
    uint32_t held[LANE];

    // d: the read's place (all zeros for a group without a read)
    __device__ __forceinline__ ReadPass(const QualityParams& p_, int lane, const Place& d_) : p(p_), g(lane), d(d_)
    {
        if (RESIDENT) fetch_values(p, d, (uint64_t)g.gl * LANE, held);
    }
    __device__ __forceinline__ uint64_t chunk_of(uint64_t pos) const { return RESIDENT ? 0 : pos / CH; }
    __device__ __forceinline__ uint64_t lane_pos(uint64_t c) const { return c * CH + (uint64_t)g.gl * LANE; }
    __device__ __forceinline__ void values(uint64_t c, uint32_t v[LANE]) const
    {
        if (RESIDENT) {
#pragma unroll
            for (int t = 0; t < LANE; ++t) v[t] = held[t];
        } else {
            fetch_values(p, d, lane_pos(c), v);
        }
    }

    // the first position of [lo, hi) whose value is at least `threshold`; hi where there is none
    __device__ __forceinline__ uint64_t first_at_least(uint64_t lo, uint64_t hi, uint32_t threshold) const
    {
        if (hi <= lo) return hi;
        const uint64_t c_last = chunk_of(hi - 1);
        for (uint64_t c = chunk_of(lo);; ++c) {
            uint32_t v[LANE];
            values(c, v);
            const uint32_t m = ge_mask(v, threshold) & range_mask(lane_pos(c), lo, hi);
            const uint64_t lanes = g.ballot(m != 0);
            if (lanes) {
                const int src = __builtin_ctzll(lanes);
                return c * CH + (uint64_t)(src * LANE + lowest_bit(g.shfl(m, src)));
            }
            if (c == c_last) return hi;
        }
    }
    // one past the last position of [lo, hi) whose value is at least `threshold`; lo where there is none
    __device__ __forceinline__ uint64_t behind_last_at_least(uint64_t lo, uint64_t hi, uint32_t threshold) const
    {
        if (hi <= lo) return lo;
        const uint64_t c_first = chunk_of(lo);
        for (uint64_t c = chunk_of(hi - 1);; --c) {
            uint32_t v[LANE];
            values(c, v);
            const uint32_t m = ge_mask(v, threshold) & range_mask(lane_pos(c), lo, hi);
            const uint64_t lanes = g.ballot(m != 0);
            if (lanes) {
                const int src = 63 - __builtin_clzll(lanes);
                return c * CH + (uint64_t)(src * LANE + highest_bit(g.shfl(m, src))) + 1;
            }
            if (c == c_first) return lo;
        }
    }

    // step B from the back of [lo, hi): the new end
    __device__ __forceinline__ uint64_t maxsum_back(uint64_t lo, uint64_t hi, uint32_t cutoff) const
    {
        if (hi <= lo) return hi;
        const uint64_t c_first = chunk_of(lo);
        long long carry = 0, best = 0;
        uint64_t best_at = hi;
        for (uint64_t c = chunk_of(hi - 1);; --c) {
            uint32_t v[LANE];
            int32_t s[LANE];
            values(c, v);
            const uint32_t mask = range_mask(lane_pos(c), lo, hi);
            const int32_t total = sums_behind(v, mask, cutoff, s);
            const int32_t behind = g.sum_behind(total);
            const long long base = carry + behind;
            const uint32_t neg = negative_mask(s, base, mask);
            const uint64_t lanes = g.ballot(neg != 0);
            uint32_t candidates = mask;
            if (lanes) {  // the walk stops in this chunk: only what lies behind the stop counts
                const int src = 63 - __builtin_clzll(lanes);
                const int bit = highest_bit(g.shfl(neg, src));
                candidates = g.gl > src ? mask : (g.gl == src ? mask & ~((2u << bit) - 1u) : 0u);
            }
            int at;
            const long long mine = best_sum(s, base, candidates, true, at);
            const long long top = g.max(mine);
            if (top > best) {  // (strictly: the chunks swept before lie behind this one and win a tie)
                const int src = 63 - __builtin_clzll(g.ballot(at >= 0 && mine == top));
                best = top;
                best_at = c * CH + (uint64_t)(src * LANE + g.shfl(at, src));
            }
            if (lanes || c == c_first) return best_at;
            carry += g.shfl(behind + total, 0);
        }
    }
    // step B from the front of [lo, hi): the new begin
    __device__ __forceinline__ uint64_t maxsum_front(uint64_t lo, uint64_t hi, uint32_t cutoff) const
    {
        if (hi <= lo) return lo;
        const uint64_t c_last = chunk_of(hi - 1);
        long long carry = 0, best = 0;
        uint64_t best_begin = lo;
        for (uint64_t c = chunk_of(lo);; ++c) {
            uint32_t v[LANE];
            int32_t s[LANE];
            values(c, v);
            const uint32_t mask = range_mask(lane_pos(c), lo, hi);
            const int32_t total = sums_in_front(v, mask, cutoff, s);
            const int32_t front = g.sum_in_front(total);
            const long long base = carry + front;
            const uint32_t neg = negative_mask(s, base, mask);
            const uint64_t lanes = g.ballot(neg != 0);
            uint32_t candidates = mask;
            if (lanes) {
                const int src = __builtin_ctzll(lanes);
                const int bit = lowest_bit(g.shfl(neg, src));
                candidates = g.gl < src ? mask : (g.gl == src ? mask & ((1u << bit) - 1u) : 0u);
            }
            int at;
            const long long mine = best_sum(s, base, candidates, false, at);
            const long long top = g.max(mine);
            if (top > best) {  // (strictly: the chunks swept before lie in front of this one and win a tie)
                const int src = __builtin_ctzll(g.ballot(at >= 0 && mine == top));
                best = top;
                best_begin = c * CH + (uint64_t)(src * LANE + g.shfl(at, src)) + 1;
            }
            if (lanes || c == c_last) return best_begin;
            carry += g.shfl(front + total, G - 1);
        }
    }

    // step C on [lo, hi): the new end
    __device__ __forceinline__ uint64_t window_cut(uint64_t lo, uint64_t hi, uint32_t W, uint32_t window_q) const
    {
        if (hi <= lo || hi - lo < W) return hi;
        // the first window's sum
        int32_t first_sum = 0;
        {
            const uint64_t c_last = chunk_of(lo + W - 1);
            for (uint64_t c = chunk_of(lo);; ++c) {
                uint32_t v[LANE];
                values(c, v);
                first_sum += (int32_t)g.sum(masked_sum(v, range_mask(lane_pos(c), lo, lo + W)));
                if (c == c_last) break;
            }
        }
        // every other window's is the first plus what it has gained: the values W positions on come from the text a second time
        const int32_t limit = (int32_t)(W * window_q);
        const uint64_t last = hi - W, c_last = chunk_of(last);
        int32_t carry = first_sum;
        for (uint64_t c = chunk_of(lo);; ++c) {
            uint32_t v[LANE], u[LANE];
            int32_t x[LANE];
            values(c, v);
            fetch_values(p, d, lane_pos(c) + W, u);
            const int32_t total = window_gains(v, u, range_mask(lane_pos(c), lo, last), x);
            const int32_t front = g.sum_in_front(total);
            const uint32_t fails = below_mask(x, carry + front, range_mask(lane_pos(c), lo, last + 1), limit);
            const uint64_t lanes = g.ballot(fails != 0);
            if (lanes) {
                const int src = __builtin_ctzll(lanes);
                const uint64_t j = c * CH + (uint64_t)(src * LANE + lowest_bit(g.shfl(fails, src)));
                return behind_last_at_least(lo, j, window_q);  // the trailing values below window_q go too
            }
            if (c == c_last) return hi;
            carry += g.shfl(front + total, G - 1);
        }
    }

    __device__ __forceinline__ Stats span_stats(uint64_t b, uint64_t e, const uint32_t* err) const
    {
        Stats st = stats_zero();
        const uint32_t need = p.need;
        if (need == 0) return st;  // (uniform over the grid)
        if (e > b) {
            const uint64_t c_last = chunk_of(e - 1);
            for (uint64_t c = chunk_of(b);; ++c) {
                uint32_t v[LANE];
                values(c, v);
                const uint32_t mask = range_mask(lane_pos(c), b, e);
                stats_add(st, v, mask, p.rule.low_q, need, err);
                if (need & NEED_AMBIGUOUS) st.n_ambiguous += (uint64_t)__builtin_popcount(ambiguous_mask(p, d, lane_pos(c)) & mask);
                if (c == c_last) break;
            }
        }
        if (need & NEED_SUM) st.sum = g.sum((unsigned long long)st.sum);
        if (need & NEED_EE) st.ee = g.sum((unsigned long long)st.ee);
        if (need & NEED_LOW) st.n_low = g.sum((unsigned long long)st.n_low);
        if (need & NEED_AMBIGUOUS) st.n_ambiguous = g.sum((unsigned long long)st.n_ambiguous);
        if (need & NEED_MINMAX) {
            st.q_min = g.min(st.q_min);
            st.q_max = g.max(st.q_max);
        }
        return st;
    }

    // the whole rule; the group's first lane writes read i's outputs and adds it to its counts
    __device__ __forceinline__ void run(uint64_t i, bool live, const uint32_t* err, unsigned long long* counts) const
    {
        const Rule& r = p.rule;
        uint64_t b = 0, e = d.L;
        if (r.front_q) b = first_at_least(b, e, r.front_q);
        if (r.back_q) e = behind_last_at_least(b, e, r.back_q);
        if (r.maxsum_front_q || r.maxsum_back_q) {
            const uint64_t e2 = r.maxsum_back_q ? maxsum_back(b, e, r.maxsum_back_q) : e;
            const uint64_t b2 = r.maxsum_front_q ? maxsum_front(b, e, r.maxsum_front_q) : b;
            b = b2;
            e = e2 > b2 ? e2 : b2;
        }
        if (r.window_len) e = window_cut(b, e, r.window_len, r.window_q);
        const Stats st = span_stats(b, e, err);
        if (!live || g.gl != 0) return;
        const uint64_t n = e - b;
        const uint32_t failed = failed_bits(r, n, st);
        if (p.out_records) {
            const Record rec = make_record(b, e, st, failed);
            const uint4* w = reinterpret_cast<const uint4*>(&rec);
            uint4* out = reinterpret_cast<uint4*>(p.out_records + i);
            out[0] = w[0];
            out[1] = w[1];
            out[2] = w[2];
        }
        if (p.out_spans) {
            const uint64_t sb = failed ? 0 : b, se = failed ? 0 : e;
            *reinterpret_cast<uint4*>(p.out_spans + 2 * i) = make_uint4((uint32_t)sb, (uint32_t)(sb >> 32), (uint32_t)se, (uint32_t)(se >> 32));
        }
        const bool kept = failed == 0 && n > 0;
        counts[C_READS] += 1;
        counts[C_KEPT] += kept ? 1 : 0;
        counts[C_BASES_IN] += d.L;
        counts[C_BASES_KEPT] += kept ? n : 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) counts[C_FAIL0 + k] += (failed >> k) & 1u;
    }
};

}  // namespace

__global__ __launch_bounds__(TPB) void quality_kernel(const QualityParams p)
{
    __shared__ uint32_t err_table[96];
    if (threadIdx.x < 94) err_table[threadIdx.x] = BL_PHRED_ERR[threadIdx.x];
    __syncthreads();
    const uint32_t* err = err_table;
    const int lane = threadIdx.x & 63;
    const uint64_t n_fours = (p.n_seqs + READS_PER_WAVE - 1) / READS_PER_WAVE, n_waves = (uint64_t)gridDim.x * (TPB / 64);
    unsigned long long counts[N_COUNTERS];
#pragma unroll
    for (int k = 0; k < N_COUNTERS; ++k) counts[k] = 0;
    // A lane's read of a four is four * 4 + lane / 16.  Its place (two offsets, then the index's record) is loaded one round ahead, so
    // that the only load a round waits for is the one of its quality bytes.
    auto place_of = [&](uint64_t four, uint64_t& i, bool& live) {
        i = four * READS_PER_WAVE + (uint64_t)(lane / SHORT_LANES);
        live = four < n_fours && i < p.n_seqs;
        Place d;
        d.first = d.L = d.q_src = d.qn = 0;
        if (live) d = place_read(p, i);
        return d;
    };
    uint64_t four = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), mine;
    bool live;
    Place here = place_of(four, mine, live);
    for (; four < n_fours; four += n_waves) {
        uint64_t next_mine;
        bool next_live;
        const Place next = place_of(four + n_waves, next_mine, next_live);
        if (__ballot(here.L > (uint64_t)SHORT_MAX) == 0) {
            const ReadPass<SHORT_LANES, true> pass(p, lane, here);
            pass.run(mine, live, err, counts);
        } else {
            for (int k = 0; k < READS_PER_WAVE; ++k) {  // (wave-uniform)
                const uint64_t i = four * READS_PER_WAVE + (uint64_t)k;
                if (i >= p.n_seqs) break;
                if (__shfl(here.L, k * SHORT_LANES, 64) <= (uint64_t)WAVE_MAX) {
                    const ReadPass<64, true> pass(p, lane, place_read(p, i));
                    pass.run(i, true, err, counts);
                } else {
                    const ReadPass<64, false> pass(p, lane, place_read(p, i));
                    pass.run(i, true, err, counts);
                }
            }
        }
        here = next;
        mine = next_mine;
        live = next_live;
    }
    if (p.counters) {  // integer sums: the order of the adds does not matter
#pragma unroll
        for (int k = 0; k < N_COUNTERS; ++k) {
            unsigned long long x = counts[k];
#pragma unroll
            for (int dd = 32; dd >= 1; dd >>= 1) x += __shfl_xor(x, dd, 64);
            if (lane == 0 && x) atomicAdd(&p.counters[(blockIdx.x % STRIPES) * STRIPE_WORDS + k], x);
        }
    }
}

__global__ __launch_bounds__(TPB) void intersect_kernel(const IntersectParams p) { intersect_spans(p, (uint64_t)blockIdx.x * TPB + threadIdx.x); }

namespace {

using blh::blocks_for;
using blh::invalid;

constexpr uint64_t GRID_MAX = 1u << 16;  // workgroups: a wave then walks the reads in steps of 2^20

}  // namespace

}  // namespace blq

extern "C" int bl_scan_read_quality(bl_ctx* ctx, const bl_batch* batch, const bl_text_index* index, const bl_quality_rule* rule, bl_read_quality* d_records,
                                    uint64_t* d_spans, bl_quality_stats* stats)
{
    using namespace blq;
    if (!ctx || !batch || !index || !rule) return invalid("ctx, batch, index or rule is NULL");
    QualityParams p{};
    static_assert(sizeof(p.rule) == sizeof(*rule), "one layout");
    std::memcpy(&p.rule, rule, sizeof(p.rule));
    const Rule& r = p.rule;
    if (r.phred_base != 33 && r.phred_base != 64) return invalid("bl_quality_rule: phred_base is 33 or 64");
    if (r.quality_fill < 33 || r.quality_fill > 126) return invalid("bl_quality_rule: quality_fill is a byte 33 .. 126");
    if (r.front_q > THRESHOLD_MAX || r.back_q > THRESHOLD_MAX || r.maxsum_front_q > THRESHOLD_MAX || r.maxsum_back_q > THRESHOLD_MAX ||
        r.window_q > THRESHOLD_MAX || r.low_q > THRESHOLD_MAX || r.mean_q > THRESHOLD_MAX)
        return invalid("bl_quality_rule: a quality threshold is at most 94");
    if (r.window_len > WINDOW_MAX) return invalid("bl_quality_rule: window_len is at most 65535");
    if (r.low_max_den == 0 || r.low_max_num > r.low_max_den) return invalid("bl_quality_rule: low_max_den is at least 1 and low_max_num at most low_max_den");
    if (r.reserved != 0) return invalid("bl_quality_rule: reserved must be 0");
    if (!rule_valid(r)) return invalid("bl_quality_rule: invalid");  // (never: the tests above are its parts)
    if (blh::misaligned16(d_records) || blh::misaligned16(d_spans)) return invalid("d_records and d_spans must be 16-byte aligned");
    bl_ctx* index_ctx = nullptr;
    uint64_t index_bases = 0, n_records = 0, n_text = 0;
    int fastq = 0;
    const uint8_t* d_text = nullptr;
    const void* d_index_records = nullptr;
    BLH_OK(bl_text_index_describe(index, &index_ctx, &index_bases));
    BLH_OK(bl_text_index_info(index, &n_records, &fastq, &d_text, &n_text, &d_index_records));
    if (index_ctx != ctx) return invalid("the index belongs to another context");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    if (view.n_seqs != n_records || view.n_bases != index_bases) return invalid("the batch is not the one the index was built with");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (view.n_seqs == 0) return BL_OK;

    p.bases = view.bases;
    p.n_bases = view.n_bases;
    p.offsets = bl_text_index_offsets(index);
    p.n_seqs = view.n_seqs;
    p.text = d_text;
    p.n_text = n_text;
    p.records = static_cast<const blfmt::TextRecord*>(d_index_records);
    p.fastq = fastq && d_text ? 1u : 0u;
    p.need = stats_needed(r, d_records != nullptr);
    p.out_records = reinterpret_cast<Record*>(d_records);
    p.out_spans = d_spans;

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the context's scans in flight
    unsigned long long stripes[STRIPES * STRIPE_WORDS] = {};
    if (stats) {
        p.counters = static_cast<unsigned long long*>(bl_ctx_scratch(ctx, 6, sizeof(stripes)));
        if (!p.counters) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        BLH_TRY(hipMemsetAsync(p.counters, 0, sizeof(stripes), s));
    }
    const uint64_t wgs = (p.n_seqs + READS_PER_WAVE * (TPB / 64) - 1) / (READS_PER_WAVE * (TPB / 64));
    hipLaunchKernelGGL(quality_kernel, dim3((unsigned)(wgs < GRID_MAX ? wgs : GRID_MAX)), dim3(TPB), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bl_set_error(BL_ERR_HIP, (std::string("quality_kernel: ") + hipGetErrorString(e)).c_str());
    if (!stats) return BL_OK;
    BLH_TRY(hipMemcpyAsync(stripes, p.counters, sizeof(stripes), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    uint64_t host[N_COUNTERS] = {};
    for (int i = 0; i < STRIPES; ++i)
        for (int k = 0; k < N_COUNTERS; ++k) host[k] += stripes[i * STRIPE_WORDS + k];
    stats->n_reads = host[C_READS];
    stats->n_reads_kept = host[C_KEPT];
    stats->n_bases = host[C_BASES_IN];
    stats->n_bases_kept = host[C_BASES_KEPT];
    stats->n_too_short = host[C_FAIL0];
    stats->n_too_long = host[C_FAIL0 + 1];
    stats->n_ambiguous = host[C_FAIL0 + 2];
    stats->n_low = host[C_FAIL0 + 3];
    stats->n_mean = host[C_FAIL0 + 4];
    stats->n_ee = host[C_FAIL0 + 5];
    return BL_OK;
}

extern "C" int bl_spans_intersect(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const uint64_t* d_a, const uint64_t* d_b, uint32_t flags,
                                  uint64_t* d_out)
{
    using namespace blq;
    if (!ctx || !batch) return invalid("ctx or batch is NULL");
    if (!d_a || !d_out) return invalid("d_a or d_out is NULL");
    if (blh::misaligned16(d_a) || blh::misaligned16(d_b) || blh::misaligned16(d_out)) return invalid("d_a, d_b and d_out must be 16-byte aligned");
    if (flags & ~(uint32_t)BL_SPANS_PAIRED) return invalid("unknown flag bits");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    BLH_OK(blh::offsets_needed(d_offsets, view.n_seqs, view.read_len));
    if ((flags & BL_SPANS_PAIRED) && (view.n_seqs & 1)) return invalid("BL_SPANS_PAIRED needs an even number of sequences: reads 2j and 2j + 1 are mates");
    IntersectParams p{};
    p.offsets = d_offsets;
    p.n_seqs = view.n_seqs;
    p.n_bases = view.n_bases;
    p.read_len = d_offsets ? 0 : (view.read_len ? view.read_len : (view.n_bases ? view.n_bases : 1));
    p.a = d_a;
    p.b = d_b;
    p.flags = flags;
    p.out = d_out;
    if (p.n_seqs == 0) return BL_OK;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the calls that write the spans
    hipLaunchKernelGGL(intersect_kernel, dim3(blocks_for(p.n_seqs, TPB)), dim3(TPB), 0, s, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BL_OK : bl_set_error(BL_ERR_HIP, (std::string("intersect_kernel: ") + hipGetErrorString(e)).c_str());
}
