// bl_quality_core.hpp — per-lane bodies of bl_scan_read_quality (trimming and filtering of reads by their quality values) and
// bl_spans_intersect.  Compiled two ways like bl_select_core.hpp: by hipcc for gfx950 (bl_quality.hip) and by a host compiler under
// BL_CPU_EMU for tests/emu/emu_quality.cpp, which runs the lanes as loops over arrays of exactly their sizes.
//
// A lane owns LANE positions of a read: [pos0, pos0 + 16).  It takes their quality bytes as the aligned dwords of the text that cover
// them, funnel-shifted to the quality line's odd start (blsel::window_load / window_shift), or byte by byte where that window would
// leave the text; positions at or behind the quality line's end take the rule's fill.  Everything a lane then does is a loop over its
// 16 values with compile-time indices: 16-bit masks of a predicate, sums in front of or behind every position, the best position of
// a running sum, the statistics.  The kernel (and the emulation) join the lanes of a group — 16 lanes for a short read, the 64 of a
// wave otherwise — with ballots and shuffle scans; a read longer than a group's positions is swept chunk by chunk with a carry.
//
// Safety.  Offsets and index records are trusted for content only: read boundaries are clamped to [0, n_bases] (blsel::read_extent),
// the quality line to the text.  No byte at or behind n_text of the text or n_bases of the batch is read.
#pragma once
#include "bl_format_core.hpp"

#if defined(__HIPCC__) && !defined(BL_CPU_EMU)
#define BLQ_TABLE static __constant__ const
#else
#define BLQ_TABLE static const
#endif

namespace blq {

constexpr int TPB = 256;                // threads of a workgroup
constexpr int LANE = 16;                // positions a lane owns per chunk: one 16-byte window
constexpr int SHORT_LANES = 16;         // lanes of a group of the short body: four reads per wave
constexpr int SHORT_MAX = SHORT_LANES * LANE;  // 256: the longest read of the short body
constexpr int WAVE_MAX = 64 * LANE;     // 1,024: the longest read a wave keeps in registers; a longer one is swept
constexpr int READS_PER_WAVE = 64 / SHORT_LANES;
constexpr uint32_t Q_TOP = 93;          // the largest Phred value
constexpr uint32_t THRESHOLD_MAX = 94;  // a threshold no value reaches
constexpr uint32_t WINDOW_MAX = 65535;
constexpr int STRIPES = 64, STRIPE_WORDS = 16;  // the statistics: STRIPES copies of 10 counters, a 128-byte line each
enum { C_READS = 0, C_KEPT = 1, C_BASES_IN = 2, C_BASES_KEPT = 3, C_FAIL0 = 4, N_COUNTERS = 10 };
// include/biolib_amd.h: BL_QFAIL_*
enum { FAIL_MIN_LEN = 1, FAIL_MAX_LEN = 2, FAIL_AMBIGUOUS = 4, FAIL_LOW = 8, FAIL_MEAN = 16, FAIL_EE = 32 };

// BL_PHRED_ERR[q] = floor(2^31 * 10^(-q/10) + 1/2): the error probability of Phred value q in units of 2^-31
BLQ_TABLE uint32_t BL_PHRED_ERR[94] = {
    2147483648u, 1705806895u, 1354970580u, 1076291389u, 854928639u, 679093957u, 539423504u, 428479319u,
    340353221u, 270352174u, 214748365u, 170580690u, 135497058u, 107629139u, 85492864u, 67909396u,
    53942350u, 42847932u, 34035322u, 27035217u, 21474836u, 17058069u, 13549706u, 10762914u,
    8549286u, 6790940u, 5394235u, 4284793u, 3403532u, 2703522u, 2147484u, 1705807u,
    1354971u, 1076291u, 854929u, 679094u, 539424u, 428479u, 340353u, 270352u,
    214748u, 170581u, 135497u, 107629u, 85493u, 67909u, 53942u, 42848u,
    34035u, 27035u, 21475u, 17058u, 13550u, 10763u, 8549u, 6791u,
    5394u, 4285u, 3404u, 2704u, 2147u, 1706u, 1355u, 1076u,
    855u, 679u, 539u, 428u, 340u, 270u, 215u, 171u,
    135u, 108u, 85u, 68u, 54u, 43u, 34u, 27u,
    21u, 17u, 14u, 11u, 9u, 7u, 5u, 4u,
    3u, 3u, 2u, 2u, 1u, 1u,
};

// include/biolib_amd.h: bl_quality_rule, bl_read_quality
struct Rule {
    uint32_t phred_base, quality_fill;
    uint32_t front_q, back_q, maxsum_front_q, maxsum_back_q;
    uint32_t window_len, window_q;
    uint32_t low_q, low_max_num, low_max_den, mean_q;
    uint32_t max_ambiguous, reserved;
    uint64_t min_len, max_len, max_ee;
};
struct alignas(16) Record {
    uint64_t begin, end, sum, ee;
    uint32_t n_low, n_ambiguous;
    uint8_t q_min, q_max;
    uint16_t failed;
    uint32_t reserved;
};

BL_DEV bool rule_valid(const Rule& r)
{
    return (r.phred_base == 33 || r.phred_base == 64) && r.quality_fill >= 33 && r.quality_fill <= 126 && r.front_q <= THRESHOLD_MAX &&
           r.back_q <= THRESHOLD_MAX && r.maxsum_front_q <= THRESHOLD_MAX && r.maxsum_back_q <= THRESHOLD_MAX && r.window_q <= THRESHOLD_MAX &&
           r.low_q <= THRESHOLD_MAX && r.mean_q <= THRESHOLD_MAX && r.window_len <= WINDOW_MAX && r.low_max_den >= 1 && r.low_max_num <= r.low_max_den &&
           r.reserved == 0;
}

struct QualityParams {
    // the batch; its offsets are the index's own
    const uint8_t* bases;     // [n_bases], 16-byte aligned, nothing behind it
    uint64_t n_bases;
    const uint64_t* offsets;  // [n_seqs + 1]
    uint64_t n_seqs;
    // the index
    const uint8_t* text;      // [n_text], 16-byte aligned
    uint64_t n_text;
    const blfmt::TextRecord* records;  // [n_seqs]
    uint32_t fastq;           // 0: every quality byte is the fill
    Rule rule;
    uint32_t need;            // NEED_*: the statistics the outputs and the filters ask for (stats_needed)
    // outputs, each nullable
    Record* out_records;            // [n_seqs]
    uint64_t* out_spans;            // [n_seqs][2]
    unsigned long long* counters;   // [STRIPES][STRIPE_WORDS]
};

// read i < n_seqs: its bases are [first, first + L) of the batch; its quality bytes [0, qn) are text[q_src ...], [qn, L) the fill.
// (blfmt::describe's rule for a sequence that is its own source read, without spans.)
struct Place {
    uint64_t first, L, q_src, qn;
};
BL_DEV Place place_read(const QualityParams& p, uint64_t i)
{
    Place d;
    blsel::read_extent(p.offsets, 0, p.n_bases, i, d.first, d.L);
    d.q_src = 0;
    d.qn = 0;
    if (p.fastq) {
        const blfmt::TextRecord r = p.records[i];
        const uint64_t q = r.name_begin + r.qual_delta;
        if (q < p.n_text) {
            const uint64_t room = p.n_text - q;
            d.q_src = q;
            d.qn = d.L < room ? d.L : room;
        }
    }
    return d;
}

// the 16 bytes src[at + t], t < 16, of which the first n (0 .. 16) are wanted and lie inside [0, n_src); the others are unspecified
BL_DEV void load16(const uint8_t* src, uint64_t n_src, uint64_t at, int n, uint32_t w[4])
{
    w[0] = w[1] = w[2] = w[3] = 0;
    if (n <= 0) return;
    if (blsel::window_loadable(n_src, (int64_t)at)) {
        uint32_t v[5];
        blsel::window_load(src, at, v);
        blsel::window_shift(v, at, w);
    } else {
        for (int t = 0; t < n; ++t) {
            const uint64_t b = at + (uint64_t)t;
            const uint32_t byte = b < n_src ? src[b] : 0u;  // (always inside)
            w[t >> 2] |= byte << (8 * (t & 3));
        }
    }
}

// how many of the positions [pos0, pos0 + 16) lie in front of `end`
BL_DEV int count_before(uint64_t pos0, uint64_t end) { return end <= pos0 ? 0 : (end - pos0 < (uint64_t)LANE ? (int)(end - pos0) : LANE); }

// bit t: lo <= pos0 + t < hi
BL_DEV uint32_t range_mask(uint64_t pos0, uint64_t lo, uint64_t hi)
{
    const int a = count_before(pos0, lo), z = count_before(pos0, hi);
    return z > a ? ((1u << z) - 1u) & ~((1u << a) - 1u) : 0u;
}

// the Phred values of positions [pos0, pos0 + 16) of the read; positions at or behind L give the fill's value (callers mask them)
BL_DEV void fetch_values(const QualityParams& p, const Place& d, uint64_t pos0, uint32_t v[LANE])
{
    uint32_t w[4];
    const int n = count_before(pos0, d.qn);
    load16(p.text, p.n_text, d.q_src + pos0, n, w);
    BL_UNROLL
    for (int t = 0; t < LANE; ++t) {
        const uint32_t byte = t < n ? (w[t >> 2] >> (8 * (t & 3))) & 0xffu : p.rule.quality_fill;
        const uint32_t x = byte > p.rule.phred_base ? byte - p.rule.phred_base : 0u;
        v[t] = x < Q_TOP ? x : Q_TOP;
    }
}

// bit t: the base at position pos0 + t (inside [0, L)) is one the scans' encoder takes as invalid (bl::encode4's rule)
BL_DEV uint32_t ambiguous_mask(const QualityParams& p, const Place& d, uint64_t pos0)
{
    uint32_t w[4];
    const int n = count_before(pos0, d.L);
    load16(p.bases, p.n_bases, d.first + pos0, n, w);
    uint32_t bad = 0;
    BL_UNROLL
    for (int i = 0; i < 4; ++i) {
        uint32_t code, diff;
        bl::encode4(w[i], code, diff);
        bad |= bl::bad_bits4(diff) << (4 * i);
    }
    return n > 0 ? bad & ((1u << n) - 1u) : 0u;
}

BL_DEV uint32_t ge_mask(const uint32_t v[LANE], uint32_t threshold)
{
    uint32_t m = 0;
    BL_UNROLL
    for (int t = 0; t < LANE; ++t) m |= (v[t] >= threshold ? 1u : 0u) << t;
    return m;
}
BL_DEV int lowest_bit(uint32_t m) { return __builtin_ctz(m); }        // m != 0
BL_DEV int highest_bit(uint32_t m) { return 31 - __builtin_clz(m); }  // m != 0

// ---- step B, the running sum.  d[t] = cutoff - v[t] at the positions of `mask`, 0 elsewhere.
// back: s[t] = the sum of d[t ..]; front: s[t] = the sum of d[.. t].  Returns the lane's total.
BL_DEV int32_t sums_behind(const uint32_t v[LANE], uint32_t mask, uint32_t cutoff, int32_t s[LANE])
{
    int32_t acc = 0;
    BL_UNROLL
    for (int t = LANE - 1; t >= 0; --t) {
        acc += ((mask >> t) & 1u) ? (int32_t)cutoff - (int32_t)v[t] : 0;
        s[t] = acc;
    }
    return acc;
}
BL_DEV int32_t sums_in_front(const uint32_t v[LANE], uint32_t mask, uint32_t cutoff, int32_t s[LANE])
{
    int32_t acc = 0;
    BL_UNROLL
    for (int t = 0; t < LANE; ++t) {
        acc += ((mask >> t) & 1u) ? (int32_t)cutoff - (int32_t)v[t] : 0;
        s[t] = acc;
    }
    return acc;
}
// base + s[t] compared with 0 in 32 bits: |s[t]| <= 16 * 94, so -base may be clamped to +-2^20 without changing any comparison
BL_DEV int32_t minus_base(int64_t base)
{
    const int64_t lim = 1 << 20;
    return (int32_t)(-base > lim ? lim : (-base < -lim ? -lim : -base));
}
// bit t of `mask`: base + s[t] < 0
BL_DEV uint32_t negative_mask(const int32_t s[LANE], int64_t base, uint32_t mask)
{
    const int32_t nb = minus_base(base);
    uint32_t m = 0;
    BL_UNROLL
    for (int t = 0; t < LANE; ++t) m |= (s[t] < nb ? 1u : 0u) << t;
    return m & mask;
}
// the greatest base + s[t] above 0 over the positions of `mask`, and its t: the largest on a tie for the back end, the smallest for the
// front end.  0 and t = -1 where there is none.
BL_DEV int64_t best_sum(const int32_t s[LANE], int64_t base, uint32_t mask, bool tie_largest, int& at)
{
    const int32_t nb = minus_base(base);
    int32_t best = 0;
    at = -1;
    BL_UNROLL
    for (int t = 0; t < LANE; ++t) {
        const bool in = (mask >> t) & 1u;
        const bool better = in && s[t] > nb && (at < 0 || s[t] > best || (tie_largest && s[t] == best));
        best = better ? s[t] : best;
        at = better ? t : at;
    }
    return at >= 0 ? base + best : 0;
}

// ---- step C, the window.  x[t] = the sum of (u[j] - v[j]) over the positions j < t of `mask`: what the window sum at pos0 + t has
// gained over the one at pos0.  u: the values W positions on.  Returns the lane's total.
BL_DEV int32_t window_gains(const uint32_t v[LANE], const uint32_t u[LANE], uint32_t mask, int32_t x[LANE])
{
    int32_t acc = 0;
    BL_UNROLL
    for (int t = 0; t < LANE; ++t) {
        x[t] = acc;
        acc += ((mask >> t) & 1u) ? (int32_t)u[t] - (int32_t)v[t] : 0;
    }
    return acc;
}
// bit t of `mask`: base + x[t] < limit
BL_DEV uint32_t below_mask(const int32_t x[LANE], int32_t base, uint32_t mask, int32_t limit)
{
    uint32_t m = 0;
    BL_UNROLL
    for (int t = 0; t < LANE; ++t) m |= (base + x[t] < limit ? 1u : 0u) << t;
    return m & mask;
}
BL_DEV uint32_t masked_sum(const uint32_t v[LANE], uint32_t mask)
{
    uint32_t acc = 0;
    BL_UNROLL
    for (int t = 0; t < LANE; ++t) acc += ((mask >> t) & 1u) ? v[t] : 0u;
    return acc;
}

// ---- the statistics of a span, summed lane by lane and joined by the group
struct Stats {
    uint64_t sum, ee, n_low, n_ambiguous;
    uint32_t q_min, q_max;
};
BL_DEV Stats stats_zero()
{
    Stats s;
    s.sum = s.ee = 0;
    s.n_low = s.n_ambiguous = 0;
    s.q_min = 255;
    s.q_max = 0;
    return s;
}
// Which statistics a call has to take: all of them for the records, otherwise those of the filters that are not at their neutral values.
enum { NEED_SUM = 1, NEED_EE = 2, NEED_LOW = 4, NEED_AMBIGUOUS = 8, NEED_MINMAX = 16, NEED_ALL = 31 };
BL_DEV uint32_t stats_needed(const Rule& r, bool with_records)
{
    if (with_records) return NEED_ALL;
    return (r.mean_q ? NEED_SUM : 0u) | (r.max_ee != ~0ull ? NEED_EE : 0u) | (r.low_max_num < r.low_max_den ? NEED_LOW : 0u) |
           (r.max_ambiguous != 0xffffffffu ? NEED_AMBIGUOUS : 0u);
}
// err: BL_PHRED_ERR where the kernel keeps it (LDS).  A statistic that is not needed stays at its zero value; its filter is at its
// neutral value and passes whatever the statistic is.
BL_DEV void stats_add(Stats& s, const uint32_t v[LANE], uint32_t mask, uint32_t low_q, uint32_t need, const uint32_t* err)
{
    if (need & NEED_SUM) s.sum += masked_sum(v, mask);
    if (need & NEED_MINMAX) {
        BL_UNROLL
        for (int t = 0; t < LANE; ++t) {
            const bool in = (mask >> t) & 1u;
            s.q_min = in && v[t] < s.q_min ? v[t] : s.q_min;
            s.q_max = in && v[t] > s.q_max ? v[t] : s.q_max;
        }
    }
    if (need & NEED_LOW) s.n_low += (uint32_t)__builtin_popcount(mask & ~ge_mask(v, low_q));
    if (need & NEED_EE) {
        uint64_t ee = 0;
        BL_UNROLL
        for (int t = 0; t < LANE; ++t) ee += ((mask >> t) & 1u) ? err[v[t]] : 0u;  // (v <= 93)
        s.ee += ee;
    }
}

// the filters of a read whose trimmed span holds n positions
BL_DEV uint32_t failed_bits(const Rule& r, uint64_t n, const Stats& s)
{
    uint32_t f = 0;
    if (n < r.min_len) f |= FAIL_MIN_LEN;
    if (r.max_len != 0 && n > r.max_len) f |= FAIL_MAX_LEN;
    if (s.n_ambiguous > r.max_ambiguous) f |= FAIL_AMBIGUOUS;
    if (s.n_low * r.low_max_den > n * r.low_max_num) f |= FAIL_LOW;  // (no wrap below 2^32 positions)
    if (s.sum < (uint64_t)r.mean_q * n) f |= FAIL_MEAN;
    if (s.ee > r.max_ee) f |= FAIL_EE;
    return f;
}
BL_DEV Record make_record(uint64_t b, uint64_t e, const Stats& s, uint32_t failed)
{
    Record r;
    r.begin = b;
    r.end = e;
    r.sum = s.sum;
    r.ee = s.ee;
    r.n_low = s.n_low < 0xffffffffull ? (uint32_t)s.n_low : 0xffffffffu;  // (a read of 2^32 positions or more: saturated)
    r.n_ambiguous = s.n_ambiguous < 0xffffffffull ? (uint32_t)s.n_ambiguous : 0xffffffffu;
    r.q_min = (uint8_t)s.q_min;
    r.q_max = (uint8_t)s.q_max;
    r.failed = (uint16_t)failed;
    r.reserved = 0;
    return r;
}

// ---- bl_spans_intersect: thread i < n_seqs (the pair (2j, 2j + 1) under PAIRED is one thread's: j < n_seqs / 2)
constexpr uint32_t SPANS_PAIRED = 1u;
struct IntersectParams {
    const uint64_t* offsets;  // as blsel::SelectParams
    uint64_t n_seqs, read_len, n_bases;
    const uint64_t* a;        // [n_seqs][2]
    const uint64_t* b;        // [n_seqs][2] or NULL
    uint32_t flags;
    uint64_t* out;            // [n_seqs][2]; may be a or b
};
BL_DEV void intersect_one(const IntersectParams& p, uint64_t i, uint64_t& ob, uint64_t& oe)
{
    uint64_t first, L;
    blsel::read_extent(p.offsets, p.read_len, p.n_bases, i, first, L);
    uint64_t b = p.a[2 * i], e = p.a[2 * i + 1];
    b = b < L ? b : L;
    e = e < L ? e : L;
    if (p.b) {
        uint64_t b2 = p.b[2 * i], e2 = p.b[2 * i + 1];
        b2 = b2 < L ? b2 : L;
        e2 = e2 < L ? e2 : L;
        b = b > b2 ? b : b2;
        e = e < e2 ? e : e2;
    }
    const bool empty = e <= b;
    ob = empty ? 0 : b;
    oe = empty ? 0 : e;
}
BL_DEV void intersect_spans(const IntersectParams& p, uint64_t t)
{
    if (p.flags & SPANS_PAIRED) {
        if (t >= p.n_seqs / 2) return;
        uint64_t b0, e0, b1, e1;
        intersect_one(p, 2 * t, b0, e0);  // (both reads are read before either is written: out may be an input)
        intersect_one(p, 2 * t + 1, b1, e1);
        if (e0 == 0 || e1 == 0) b0 = e0 = b1 = e1 = 0;
        p.out[4 * t] = b0;
        p.out[4 * t + 1] = e0;
        p.out[4 * t + 2] = b1;
        p.out[4 * t + 3] = e1;
    } else {
        if (t >= p.n_seqs) return;
        uint64_t b, e;
        intersect_one(p, t, b, e);
        p.out[2 * t] = b;
        p.out[2 * t + 1] = e;
    }
}

}  // namespace blq
