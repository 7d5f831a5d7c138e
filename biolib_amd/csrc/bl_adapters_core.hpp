// bl_adapters_core.hpp — per-lane bodies of bl_scan_read_adapters (poly tails, read-through between mates and 3' adapters; the rule is
// stated in include/biolib_amd.h).  Compiled two ways like bl_quality_core.hpp: by hipcc for gfx950 (bl_adapters.hip) and by a host
// compiler under BL_CPU_EMU for tests/emu/emu_adapters.cpp, which runs the lanes as loops over arrays of exactly their sizes.
//
// Bases as bits.  A wave stages a block of its read as 16-base chunks, read-relative: a dword of 2-bit codes, first base most
// significant (the packed copy's form, bl_scan_core.hpp: encode16), and a dword of invalid bits, bit 30 - 2j for base j, so that one
// funnel shift serves both.  A chunk comes from the batch's packed copy (two dwords, shifted to the read's start) where no chunk_bad
// bit of the two is set, and from the ASCII bases otherwise and for a batch without a packed copy.  Bases at or behind the read's end
// are invalid: what the packed words hold there belongs to the next read.  A window of 32 bases at any position of the block is three
// staged dwords and a shift; the mismatches of up to 32 bases are x = a ^ b, popcount((((x | x >> 1) & 0x5555...) | invalid) & length).
//
// Safety.  Offsets and input spans are trusted for content only: read boundaries are clamped to [0, n_bases] (blsel::read_extent), spans
// to the read.  ASCII bytes are read only inside [0, n_bases), packed words only for chunks that hold a base of the batch and the one
// behind (the copy's tail guard).
#pragma once
#include "bl_quality_core.hpp"

// a function that calls the wave's own members (device only in the kernel, plain host code in the emulation)
#if defined(__HIPCC__) && !defined(BL_CPU_EMU)
#define BLA_WAVE __device__ __forceinline__
#else
#define BLA_WAVE static inline
#endif

namespace bla {

constexpr int TPB = 256;                 // threads of a workgroup: four waves, a read or a pair of mates each at a time
constexpr int BLOCK = 1024;              // positions of a staged block
constexpr int BLOCK_CHUNKS = BLOCK / 16;
constexpr int STAGE_CHUNKS = 72;         // chunks staged per block: its 64, four behind them (an adapter of 64 at its last position), one
                                         // for the funnel, rounded up; stage_chunk makes the ones behind the read invalid
constexpr int MAX_ADAPTERS = 8, ADAPTER_MAX = 64;
constexpr int PAIR_MAX = 512;            // the longest shorter mate step 2 takes
constexpr int PAIR_CHUNKS = PAIR_MAX / 16 + 4;  // chunks of a mate's staged head, and of the reverse complement, with the windows' reach
constexpr uint64_t M5 = 0x5555555555555555ull;
constexpr int STRIPES = 64, STRIPE_WORDS = 32;  // the statistics: STRIPES copies of N_COUNTERS counters
enum { C_READS = 0, C_CUT, C_KEPT, C_BASES_IN, C_BASES_KEPT, C_BIT0 /* six: BL_ADAPT_* */, C_ADAPTER0 = C_BIT0 + 6, N_COUNTERS = C_ADAPTER0 + MAX_ADAPTERS };
// include/biolib_amd.h: BL_ADAPT_*, BL_ADAPTERS_PAIRED
enum { CUT_POLY_BEFORE = 1, CUT_PAIR = 2, CUT_ADAPTER = 4, CUT_POLY_AFTER = 8, CUT_TOO_SHORT = 16, CUT_PAIR_SKIPPED = 32, CUT_MOVED = 15 };
constexpr uint32_t FLAG_PAIRED = 1u;
constexpr uint32_t NONE32 = 0xffffffffu;

// include/biolib_amd.h: bl_adapter_rule, bl_read_adapters
struct Rule {
    uint32_t flags, n_adapters;
    uint32_t adapter_len[MAX_ADAPTERS];
    char adapters[MAX_ADAPTERS][ADAPTER_MAX];
    uint32_t min_overlap, error_num, error_den;
    uint32_t pair_min_overlap, pair_error_num, pair_error_den, pair_max_diff;
    uint32_t poly_before, poly_after, poly_min_len, poly_per, poly_max_mismatch;
    uint32_t reserved;
    uint64_t min_len;
};
struct alignas(16) Record {
    uint64_t begin, end;
    uint32_t match_pos, insert;
    uint16_t adapter;
    uint8_t overlap, mismatches;
    uint16_t pair_mismatches;
    uint8_t cut, reserved;
};

// the rule as the kernel takes it: the adapters as packed words (first base most significant, zeros behind the last)
struct KRule {
    uint32_t flags, n_adapters;
    uint32_t adapter_len[MAX_ADAPTERS];
    uint64_t adapter_words[MAX_ADAPTERS][2];
    uint32_t min_overlap, error_num, error_den;
    uint32_t pair_min_overlap, pair_error_num, pair_error_den, pair_max_diff;
    uint32_t poly_before, poly_after, poly_min_len, poly_per, poly_max_mismatch;
    uint64_t min_len;
};

// the code of an adapter's byte, -1 for anything but ACGTUacgtu (bl::encode4's rule)
BL_DEV int base_code(unsigned char c)
{
    switch (c | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't':
    case 'u': return 3;
    default: return -1;
    }
}

// NULL where the rule is valid, else what is wrong with it (the entry point's message)
BL_DEV const char* rule_error(const Rule& r, uint64_t n_seqs)
{
    if (r.flags & ~FLAG_PAIRED) return "bl_adapter_rule: unknown flag bits";
    if ((r.flags & FLAG_PAIRED) && (n_seqs & 1)) return "BL_ADAPTERS_PAIRED needs an even number of sequences: reads 2j and 2j + 1 are mates";
    if (r.n_adapters > (uint32_t)MAX_ADAPTERS) return "bl_adapter_rule: n_adapters is at most 8";
    for (uint32_t a = 0; a < r.n_adapters; ++a) {
        if (r.adapter_len[a] == 0 || r.adapter_len[a] > (uint32_t)ADAPTER_MAX) return "bl_adapter_rule: an adapter holds 1 .. 64 bases";
        for (uint32_t j = 0; j < r.adapter_len[a]; ++j)
            if (base_code((unsigned char)r.adapters[a][j]) < 0) return "bl_adapter_rule: an adapter holds ACGTUacgtu only";
    }
    if (r.n_adapters && r.min_overlap == 0) return "bl_adapter_rule: min_overlap is at least 1";
    if (r.error_den == 0 || r.error_num > r.error_den) return "bl_adapter_rule: error_den is at least 1 and error_num at most error_den";
    if (r.pair_error_den == 0 || r.pair_error_num > r.pair_error_den)
        return "bl_adapter_rule: pair_error_den is at least 1 and pair_error_num at most pair_error_den";
    if ((r.flags & FLAG_PAIRED) && r.pair_min_overlap == 0) return "bl_adapter_rule: pair_min_overlap is at least 1";
    if (r.poly_before > 15 || r.poly_after > 15) return "bl_adapter_rule: a poly mask holds the bits of codes 0 .. 3";
    if ((r.poly_before | r.poly_after) && r.poly_min_len == 0) return "bl_adapter_rule: poly_min_len is at least 1";
    if (r.reserved != 0) return "bl_adapter_rule: reserved must be 0";
    return nullptr;
}

// (r is valid)
BL_DEV void pack_rule(const Rule& r, KRule& k)
{
    k.flags = r.flags;
    k.n_adapters = r.n_adapters;
    for (int a = 0; a < MAX_ADAPTERS; ++a) {
        const uint32_t A = (uint32_t)a < r.n_adapters ? r.adapter_len[a] : 0;
        k.adapter_len[a] = A;
        k.adapter_words[a][0] = k.adapter_words[a][1] = 0;
        for (uint32_t j = 0; j < A; ++j) k.adapter_words[a][j >> 5] |= (uint64_t)base_code((unsigned char)r.adapters[a][j]) << (62 - 2 * (j & 31));
    }
    k.min_overlap = r.min_overlap;
    k.error_num = r.error_num;
    k.error_den = r.error_den;
    k.pair_min_overlap = r.pair_min_overlap;
    k.pair_error_num = r.pair_error_num;
    k.pair_error_den = r.pair_error_den;
    k.pair_max_diff = r.pair_max_diff;
    k.poly_before = r.poly_before;
    k.poly_after = r.poly_after;
    k.poly_min_len = r.poly_min_len;
    k.poly_per = r.poly_per;
    k.poly_max_mismatch = r.poly_max_mismatch;
    k.min_len = r.min_len;
}

struct AdapterParams {
    const uint8_t* bases;          // [n_bases], 16-byte aligned, nothing behind it
    uint64_t n_bases;
    const uint64_t* offsets;       // [n_seqs + 1] or NULL: reads of read_len
    uint64_t read_len, n_seqs;
    const uint32_t* codes_packed;  // the batch's packed copy (bl_scan_core.hpp: ScanParams), chunk 0; NULL: none
    const uint32_t* chunk_bad;
    const uint64_t* spans_in;      // [n_seqs][2] or NULL
    KRule rule;
    // outputs, each nullable
    Record* out_records;            // [n_seqs]
    uint64_t* out_spans;            // [n_seqs][2]
    unsigned long long* counters;   // [STRIPES][STRIPE_WORDS]
};

// the invalid bits of the bases j >= n of a chunk (n = 0 .. 16)
BL_DEV uint32_t tail_invalid(int n) { return (uint32_t)(0x55555555ull & ((1ull << (32 - 2 * n)) - 1ull)); }
// bit t of a 16-bit mask (base t) to bit 30 - 2t
BL_DEV uint32_t spread_invalid(uint32_t bad16)
{
    uint32_t x = __builtin_bitreverse32(bad16) >> 16;  // base t at bit 15 - t
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// Chunk c of the read [first, first + L) of the batch (first + L <= n_bases): the codes and invalid bits of its bases [16 c, 16 c + 16).
// Returns 0 for a chunk behind the read (nothing is loaded), 1 for one from the packed copy, 2 for one from the ASCII bases.
BL_DEV int stage_chunk(const AdapterParams& p, uint64_t first, uint64_t L, uint64_t c, uint32_t& code, uint32_t& inv)
{
    const uint64_t pos0 = c * 16;
    const int n = blq::count_before(pos0, L);
    code = 0;
    inv = 0x55555555u;
    if (n == 0) return 0;
    const uint64_t g = first + pos0, gi = g >> 4;
    const int r = (int)(g & 15);
    if (p.codes_packed) {
        // the read's n bases lie in the batch's chunks gi and, where r + n > 16, gi + 1.  Word gi + 1 of either array is loaded whether it is
        // needed or not: chunk gi holds base g < n_bases, and the copy goes on for bl::PACK_TAIL guard chunks behind the batch's last
        // (zero codes, bad bits set; bl_scan_core.hpp: packed_total), so gi + 1 is there at the batch's last chunk too
        const uint32_t bad_word = p.chunk_bad[gi >> 5], bad_next = p.chunk_bad[(gi + 1) >> 5];
        const bool bad = ((bad_word >> (gi & 31)) & 1u) || (r + n > 16 && ((bad_next >> ((gi + 1) & 31)) & 1u));
        if (!bad) {
            const uint64_t two = ((uint64_t)p.codes_packed[gi] << 32) | p.codes_packed[gi + 1];
            code = (uint32_t)((two << (2 * r)) >> 32);
            inv = tail_invalid(n);
            return 1;
        }
    }
    uint32_t w[4];
    blq::load16(p.bases, p.n_bases, g, n, w);
    uint32_t bad16 = 0;
    BL_UNROLL
    for (int i = 0; i < 4; ++i) {
        uint32_t code8, diff;
        bl::encode4(w[i], code8, diff);
        code |= code8 << (24 - 8 * i);
        bad16 |= bl::bad_bits4(diff) << (4 * i);
    }
    inv = spread_invalid(bad16) | tail_invalid(n);
    return 2;
}

// the 32 bases from base q (>= 0) of a staged array on, first base most significant; reads arr[q / 16 .. q / 16 + 2]
BL_DEV uint64_t window64(const uint32_t* arr, uint32_t q)
{
    const uint32_t i = q >> 4;
    const int sh = 2 * (int)(q & 15);
    const uint64_t two = ((uint64_t)arr[i] << 32) | arr[i + 1];
    return (two << sh) | ((uint64_t)arr[i + 2] >> (32 - sh));
}
// the first n (1 .. 32) bases of a 64-bit window
BL_DEV uint64_t length_mask(int n) { return ~0ull << (64 - 2 * n); }
BL_DEV int mismatches64(uint64_t a, uint64_t b, uint64_t invalid, int n)
{
    const uint64_t x = a ^ b;
    return __builtin_popcountll((((x | (x >> 1)) & M5) | invalid) & length_mask(n));
}

// the base at q of a staged array: its code, 4 where it is invalid
BL_DEV uint32_t base_at(const uint32_t* codes, const uint32_t* inv, uint32_t q)
{
    const int sh = 30 - 2 * (int)(q & 15);
    return ((inv[q >> 4] >> sh) & 1u) ? 4u : (codes[q >> 4] >> sh) & 3u;
}

// ---- steps 1 and 4.  A lane holds position e - t of the walk for base X with x = the number of the last t bases that are not X.
BL_DEV bool poly_stops(const KRule& r, uint64_t t, uint64_t x)
{
    if (x > r.poly_max_mismatch) return true;
    if (t < r.poly_min_len) return false;
    return r.poly_per ? t < x * (uint64_t)r.poly_per : x > 0;  // x > floor(t / per); (x <= poly_max_mismatch < 2^32: no wrap)
}

// x of the lane at position q0 + lane of a round: the round's bases at and behind it that are not X, and those of the rounds before
BL_DEV uint64_t poly_count(uint64_t carry, uint64_t not_x, int lane) { return carry + (uint64_t)__builtin_popcountll(not_x >> lane); }
// What a round of 64 positions from q0 on decides, from its ballots (bit = lane): stops, the lanes where the walk stops; is_x, the
// lanes that hold X.  The first t that stops is the ballot's top bit, and the walk holds the positions behind it; n becomes the bases
// walked, left the leftmost X among the walked ones of this round.  True where the walk ends here.
BL_DEV bool poly_join(uint64_t stops, uint64_t is_x, uint64_t q0, uint64_t e, uint64_t& n, uint64_t& left)
{
    if (stops) {
        const int top = 63 - __builtin_clzll(stops);
        n = e - (q0 + (uint64_t)top) - 1;
        is_x = top == 63 ? 0ull : is_x & (~0ull << (top + 1));
    }
    if (is_x) left = q0 + (uint64_t)__builtin_ctzll(is_x);
    return stops != 0;
}

// ---- step 3.  Adapter a at position p of the span [b, e), p + O <= e: q is p relative to the staged block.  The candidate's key, 0 for
// none: matches + 1, then the smaller p, then the lower a.
constexpr uint64_t KEY_POS = (1ull << 48) - 1;
BL_DEV uint64_t adapter_key(const KRule& r, int a, const uint32_t* codes, const uint32_t* inv, uint32_t q, uint64_t p, uint64_t e, int& o_out, int& m_out)
{
    const int A = (int)r.adapter_len[a];
    const int o = e - p < (uint64_t)A ? (int)(e - p) : A;
    int m = mismatches64(window64(codes, q), r.adapter_words[a][0], window64(inv, q), o < 32 ? o : 32);
    if (o > 32) m += mismatches64(window64(codes, q + 32), r.adapter_words[a][1], window64(inv, q + 32), o - 32);
    o_out = o;
    m_out = m;
    if ((uint64_t)m * r.error_den > (uint64_t)o * r.error_num) return 0;  // m > floor(o * num / den)
    return ((uint64_t)(o - m + 1) << 52) | ((KEY_POS - (p < KEY_POS ? p : KEY_POS)) << 4) | (uint64_t)(15 - a);
}
BL_DEV uint64_t key_pos(uint64_t key) { return KEY_POS - ((key >> 4) & KEY_POS); }
BL_DEV int key_adapter(uint64_t key) { return 15 - (int)(key & 15); }

// ---- step 2.  M = min(L1, L2) <= PAIR_MAX.  r1 and r2 are staged from their first bases; rc is the reverse complement of r2's first M
// bases: rc[k] = complement(r2[M - 1 - k]), so that r2[I - 1 - i] = rc[M - I + i].
// chunk c of rc from r2's staged chunks (PAIR_CHUNKS of them)
BL_DEV void reverse_chunk(const uint32_t* r2_codes, const uint32_t* r2_inv, int M, int c, uint32_t& code, uint32_t& inv)
{
    const int n = M - 16 * c < 0 ? 0 : (M - 16 * c > 16 ? 16 : M - 16 * c);
    code = 0;
    inv = 0x55555555u;
    if (n == 0) return;
    const int q = M - 16 * c - 16;  // r2's positions [q, q + 16); q > -16, and the ones below 0 become the bases k >= M
    uint32_t wc, wi;
    if (q >= 0) {
        wc = (uint32_t)(window64(r2_codes, (uint32_t)q) >> 32);
        wi = (uint32_t)(window64(r2_inv, (uint32_t)q) >> 32);
    } else {
        wc = r2_codes[0] >> (2 * -q);
        wi = r2_inv[0] >> (2 * -q);
    }
    const uint32_t rc = __builtin_bitreverse32(~wc), ri = __builtin_bitreverse32(wi);
    code = ((rc >> 1) & 0x55555555u) | ((rc & 0x55555555u) << 1);
    inv = (ri >> 1) | tail_invalid(n);
}
// d(I) for I in [1, M]; stops counting above `stop`
BL_DEV uint32_t pair_diff(const uint32_t* r1_codes, const uint32_t* r1_inv, const uint32_t* rc_codes, const uint32_t* rc_inv, int M, int I, uint32_t stop)
{
    uint32_t d = 0;
    const int s = M - I;
    for (int at = 0; at < I && d <= stop; at += 32) {
        const int n = I - at < 32 ? I - at : 32;
        d += (uint32_t)mismatches64(window64(r1_codes, (uint32_t)at), window64(rc_codes, (uint32_t)(s + at)),
                                    window64(r1_inv, (uint32_t)at) | window64(rc_inv, (uint32_t)(s + at)), n);
    }
    return d;
}
BL_DEV bool pair_qualifies(const KRule& r, int I, uint32_t d)
{
    return d <= r.pair_max_diff && (uint64_t)d * r.pair_error_den <= (uint64_t)I * r.pair_error_num;
}

// ---- a read's span at the start: the input span clamped as blsel::span_lengths clamps, [0, L) without one
BL_DEV void start_span(const AdapterParams& p, uint64_t i, uint64_t L, uint64_t& b, uint64_t& e)
{
    b = 0;
    e = L;
    if (p.spans_in) {
        const uint64_t b0 = p.spans_in[2 * i], e0 = p.spans_in[2 * i + 1];
        b = b0 < L ? b0 : L;
        e = e0 < L ? e0 : L;
    }
    if (e <= b) b = e = 0;
}

// what one lane of the wave keeps of a read while the steps run, and writes at the end
struct Outcome {
    uint64_t b, e;
    uint32_t match_pos, insert;
    uint32_t adapter, overlap, mismatches, pair_mismatches, cut;
};
BL_DEV Outcome outcome_none()
{
    Outcome o;
    o.b = o.e = 0;
    o.match_pos = NONE32;
    o.insert = 0;
    o.adapter = 0xffffu;
    o.overlap = o.mismatches = o.pair_mismatches = o.cut = 0;
    return o;
}
BL_DEV Record make_record(const Outcome& o)
{
    Record r;
    r.begin = o.b;
    r.end = o.e;
    r.match_pos = o.match_pos;
    r.insert = o.insert;
    r.adapter = (uint16_t)o.adapter;
    r.overlap = (uint8_t)o.overlap;
    r.mismatches = (uint8_t)o.mismatches;
    r.pair_mismatches = (uint16_t)o.pair_mismatches;
    r.cut = (uint8_t)o.cut;
    r.reserved = 0;
    return r;
}
// The four steps of read i of length L, written once for the kernel's wave and the emulation's loops over the lanes.  Pass has
//   uint64_t poly(b, e, mask)    steps 1 and 4 on [b, e), e > b: the new end
//   uint64_t adapters(b, e)      step 3 on [b, e): the best candidate's key over the wave, 0 for none
// insert, pair_mismatches and skipped are step 2's answer for the pair.  Uniform over the wave.
template <typename Pass>
BLA_WAVE Outcome read_steps(Pass& pass, const AdapterParams& p, uint64_t i, uint64_t L, bool paired, uint32_t insert, uint32_t pair_mismatches, bool skipped,
                            bool& input_empty)
{
    const KRule& r = p.rule;
    Outcome o = outcome_none();
    uint64_t b, e;
    start_span(p, i, L, b, e);
    input_empty = e <= b;
    if (input_empty) return o;
    if (r.poly_before) {
        const uint64_t e2 = pass.poly(b, e, r.poly_before);
        if (e2 < e) o.cut |= CUT_POLY_BEFORE;
        e = e2;
    }
    if (paired && skipped) o.cut |= CUT_PAIR_SKIPPED;
    if (paired && insert) {
        o.insert = insert;
        o.pair_mismatches = pair_mismatches;
        const uint64_t e2 = insert < e ? (insert > b ? insert : b) : e;
        if (e2 < e) o.cut |= CUT_PAIR;
        e = e2;
    }
    if (r.n_adapters) {
        const uint64_t key = pass.adapters(b, e);
        if (key) {
            const uint64_t pos = key_pos(key);
            const int a = key_adapter(key);
            o.adapter = (uint32_t)a;
            o.overlap = e - pos < r.adapter_len[a] ? (uint32_t)(e - pos) : r.adapter_len[a];
            o.mismatches = o.overlap - ((uint32_t)(key >> 52) - 1u);
            o.match_pos = pos < NONE32 ? (uint32_t)pos : NONE32 - 1;  // (a read of 2^32 bases or more: saturated)
            o.cut |= CUT_ADAPTER;
            e = pos;
        }
    }
    if (r.poly_after && e > b) {
        const uint64_t e2 = pass.poly(b, e, r.poly_after);
        if (e2 < e) o.cut |= CUT_POLY_AFTER;
        e = e2;
    }
    o.b = b;
    o.e = e;
    return o;
}

// the span that goes out, the TOO_SHORT bit, and the read's part of the statistics (counts NULL: nobody asked); input_empty: no step ran
BL_DEV void finish_read(const KRule& r, Outcome& o, bool input_empty, uint64_t L, uint64_t& sb, uint64_t& se, unsigned long long* counts)
{
    const uint64_t n = o.e - o.b;
    if (!input_empty && n < r.min_len) o.cut |= CUT_TOO_SHORT;
    const bool kept = n > 0 && n >= r.min_len;
    sb = kept ? o.b : 0;
    se = kept ? o.e : 0;
    if (!counts) return;
    counts[C_READS] += 1;
    counts[C_CUT] += (o.cut & CUT_MOVED) ? 1 : 0;
    counts[C_KEPT] += kept ? 1 : 0;
    counts[C_BASES_IN] += L;
    counts[C_BASES_KEPT] += kept ? n : 0;
    BL_UNROLL
    for (int k = 0; k < 6; ++k) counts[C_BIT0 + k] += (o.cut >> k) & 1u;
    BL_UNROLL
    for (int a = 0; a < MAX_ADAPTERS; ++a) counts[C_ADAPTER0 + a] += o.adapter == (uint32_t)a ? 1 : 0;
}

}  // namespace bla
