// bl_correct_core.hpp — per-thread bodies of bl_scan_read_edits (single-substitution repair of reads from a count table) and
// bl_batch_apply_edits.  Compiled two ways like bl_select_core.hpp and bl_lookup_core.hpp: by hipcc for gfx950 (bl_correct.hip) and by a
// host compiler under BL_CPU_EMU for tests/emu/emu_correct.cpp, which runs the lanes as loops over arrays of exactly their lengths.
//
// The rule (include/biolib_amd.h).  Every position of a read is INVALID (no valid k-mer starts there), SOLID (valid,
// table count >= min_count) or WEAK (valid, count < min_count).  A weak run is a maximal interval [a, b] of WEAK positions of one read.
// A substitution at base p touches exactly the k-mers max(0, p - k + 1) .. min(p, n - 1) of its read, so a run that is that interval for
// some p, with a SOLID position on one side, names p; the run is repaired iff exactly one of the three other bases at p makes every
// k-mer of the run SOLID.
//
// Passes:
//   1  state_thread    the tile of bl_scan_kmer_counts: a byte per position — the state in bits 0-1, "a read starts here" in bit 2.
//                      Positions behind a read's last k-mer (the window crosses the read's or the batch's end) are ST_NONE, which is
//                      INVALID for the rule and tells the run pass where n - 1 lies without the offsets.
//   2  run_at          one lane per position: is it a run's first position, how long is the run (at most k + 1 states are walked: a
//                      longer run is a misfit), which shape, enough support.  Candidates go to a position-ordered list
//                      (count -> exclusive sum -> write), the rejected classes to the statistics.
//   3  test_lane       one wave per candidate, lane i the run's k-mer i.  The wave's (at most 127) bases are staged as 2-bit codes in a
//                      256-bit string; a lane takes its k-mer with funnel shifts, builds the reverse complement once and patches the
//                      2-bit code at p in both: three alternatives, one search_group call.  Ballots AND the lanes; verdict() is lane 0's.
//   4  compaction of the edits in candidate order (exclusive sum of the edit flags), nothing at or beyond the capacity.
//   5  apply           edit_at: one lane per edit on a copy of the bases.
#pragma once
#include "bl_lookup_core.hpp"

namespace blcr {

constexpr int CTPB = 256;                       // threads of a workgroup, every kernel; the run pass takes one position per thread
constexpr int TEST_WAVES = CTPB / 64;           // candidates a workgroup of the test pass takes: one per wave
constexpr int MAX_RUN = 64;                     // k-mers of a run that fits: at most k <= 64, one per lane
constexpr int CODE_WORDS = 8;                   // the staged bases of a candidate: 128 two-bit codes
constexpr int CODE_WORDS_PADDED = CODE_WORDS + 4;  // zeros above: a lane reads five words from word (256 - 2(i + k)) / 32 on

enum : uint32_t { ST_INVALID = 0, ST_WEAK = 1, ST_SOLID = 2, ST_NONE = 3, ST_MASK = 3, ST_START = 4 };
enum : int { RUN_NOT_A_START = 0, RUN_MISFIT = 1, RUN_LOW_SUPPORT = 2, RUN_CANDIDATE = 3 };
enum : uint32_t { V_NONE = 0, V_EDIT = 1, V_AMBIGUOUS = 2, V_NO_BASE = 3 };

// include/biolib_amd.h: bl_edit
struct alignas(16) Edit {
    uint64_t pos;
    uint8_t from, to, support, anchor;
    uint32_t reserved;
};
struct alignas(16) Candidate {
    uint64_t a;       // the run's first position
    uint32_t len;     // b - a + 1, 1 .. k
    uint32_t anchor;  // 0 left-anchored (p = a + k - 1), 1 right-anchored (p = b)
};
// the device words of the statistics (include/biolib_amd.h: bl_edit_stats, in its order)
enum : int { STAT_RUNS = 0, STAT_EDITS, STAT_AMBIGUOUS, STAT_NO_BASE, STAT_MISFIT, STAT_LOW_SUPPORT, STAT_WORDS = 8 };

// ---- pass 1
struct StateParams {
    bl::Kmer128Params km;  // staging, k, strand; [first, end) are the positions whose states are stored
    bllk::TableView table;
    uint32_t min_count;
    uint8_t* states;       // indexed by position - km.first
};

BL_DEV void state_thread(const StateParams& p, const uint32_t* codes, const uint32_t* flags, int tid, int64_t q0)
{
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    const uint32_t inrange = bl::range_mask(p.km.first - j0, p.km.end - j0) & 0xffffu;
    if (inrange == 0) return;
    bl::Bits128 good, start;
    bl::gather_flags(flags, tid, good, start);
    const uint32_t ok = bl::window_valid_mask(good, start, p.km.unit) & inrange;
    // the same windows with every base inside the batch taken as good: the positions of a read that have a k-mer at all
    const int64_t left = p.km.n_bases - j0;  // > 0: a position of the range lies at or behind j0
    bl::Bits128 inside;
    inside.lo = left >= 64 ? ~0ull : ((1ull << left) - 1);
    inside.hi = left >= 128 ? ~0ull : (left <= 64 ? 0ull : ((1ull << (left - 64)) - 1));
    const uint32_t has = bl::window_valid_mask(inside, start, p.km.unit) & inrange;
    bl::Kmer128Lane L;
    bl::kmer128_lane_start(L, codes + tid, p.km.unit, p.km.canonical != 0);
    BL_ROLLED
    for (int s0 = 0; s0 < bl::S; s0 += bllk::G) {
        uint64_t lo[bllk::G], hi[bllk::G];
        uint32_t c[bllk::G];
        const uint32_t live = (ok >> s0) & ((1u << bllk::G) - 1u);
        BL_UNROLL
        for (int g = 0; g < bllk::G; ++g) bl::kmer128_at(L, s0 + g, p.km.canonical != 0, lo[g], hi[g]);
        bllk::search_group(p.table, lo, hi, live, c);
        BL_UNROLL
        for (int g = 0; g < bllk::G; ++g) {
            const int s = s0 + g;
            if ((inrange >> s) & 1u) {
                uint32_t st = ((live >> g) & 1u) ? (c[g] >= p.min_count ? ST_SOLID : ST_WEAK) : (((has >> s) & 1u) ? ST_INVALID : ST_NONE);
                if ((start.lo >> s) & 1u) st |= ST_START;
                p.states[j0 + s - p.km.first] = (uint8_t)st;
            }
        }
    }
}

// ---- pass 2
struct RunParams {
    const uint8_t* states;  // the states of [s0, s1): s0 = max(first - 1, 0), s1 = min(end + k + 1, n_bases)
    int64_t s0, s1;
    int64_t first, end;     // the runs whose first position lies in [first, end) are judged
    uint32_t k, min_support;
};

// position a in [first, end): is it a run's first position, and what becomes of the run
BL_DEV int run_at(const RunParams& p, int64_t a, Candidate& c)
{
    const uint32_t st = p.states[a - p.s0];
    if ((st & ST_MASK) != ST_WEAK) return RUN_NOT_A_START;
    const bool read_start = (st & ST_START) != 0 || a == 0;
    bool left = false;
    if (!read_start) {  // a - 1 >= s0 lies in the same read
        const uint32_t prev = p.states[a - 1 - p.s0] & ST_MASK;
        if (prev == ST_WEAK) return RUN_NOT_A_START;
        left = prev == ST_SOLID;
    }
    // the states a + 1 .. a + k: a + k < end + k + 1, so a position at or behind s1 lies behind the batch
    uint32_t len = 1;
    while (len <= p.k) {
        const int64_t j = a + (int64_t)len;
        if (j >= p.s1) break;
        const uint32_t x = p.states[j - p.s0];
        if ((x & ST_START) || (x & ST_MASK) != ST_WEAK) break;
        ++len;
    }
    if (len > p.k) return RUN_MISFIT;  // longer than any single substitution makes it
    // b + 1: a k-mer position of the same read (b <= n - 2), and is it SOLID
    bool has_next = false, next_solid = false;
    const int64_t j = a + (int64_t)len;
    if (j < p.s1) {
        const uint32_t x = p.states[j - p.s0];
        if (!(x & ST_START) && (x & ST_MASK) != ST_NONE) {
            has_next = true;
            next_solid = (x & ST_MASK) == ST_SOLID;
        }
    }
    bool fits;
    if (left) fits = len == p.k || !has_next;             // b = min(a + k - 1, n - 1)
    else if (next_solid) fits = len == p.k || read_start;  // a = max(0, b - k + 1)
    else return RUN_MISFIT;                                // unanchored
    if (!fits) return RUN_MISFIT;
    if (len < p.min_support) return RUN_LOW_SUPPORT;
    c.a = (uint64_t)a;
    c.len = len;
    c.anchor = left ? 0u : 1u;
    return RUN_CANDIDATE;
}

BL_DEV uint64_t edit_position(const Candidate& c, uint32_t k) { return c.anchor == 0 ? c.a + k - 1 : c.a + c.len - 1; }

// ---- pass 3
struct TestParams {
    const uint8_t* bases;
    int64_t n_bases;
    bllk::TableView table;
    uint32_t k, min_count, canonical;
    const Candidate* cand;
    uint64_t n_cand;
    Edit* edits;          // [n_cand]: the edit of candidate i where its verdict is V_EDIT
    uint8_t* verdicts;    // [n_cand]
    uint64_t* edit_flag;  // [n_cand + 1]: 1 where the verdict is V_EDIT (entry n_cand is zeroed by the host)
};

// lane l < 32 of a candidate's wave: the codes of the four bases from g = a + 4l on, first base in the top pair; zeros behind the batch
// (the dword load takes `bases` itself to be at least 4-byte aligned: every batch buffer is 16-byte aligned, bl_batch_from_device insists on it)
BL_DEV uint32_t code_byte(const uint8_t* bases, int64_t n_bases, int64_t g)
{
    uint32_t d = 0;
    if (g + 4 <= n_bases && (g & 3) == 0) {
        d = *reinterpret_cast<const uint32_t*>(bases + g);
    } else {
        for (int b = 0; b < 4; ++b)
            if (g + b < n_bases) d |= (uint32_t)bases[g + b] << (8 * b);
    }
    uint32_t x = (d >> 1) & 0x03030303u;
    x ^= (x >> 1) & 0x01010101u;
    return (x * 0x40100401u) >> 24;
}
// where lane l's byte goes in the little-endian byte string of the 256 bits (base 0 in the top pair of the top byte)
BL_DEV int code_byte_index(int lane) { return 4 * CODE_WORDS - 1 - lane; }

BL_DEV void patch2(uint64_t& lo, uint64_t& hi, int bit, uint64_t code)
{
    if (bit < 64) lo = (lo & ~(3ull << bit)) | (code << bit);
    else hi = (hi & ~(3ull << (bit - 64))) | (code << (bit - 64));
}

// reverse complement of a k-mer held in the low 2k bits of hi:lo
BL_DEV void revcomp_kmer(uint64_t lo, uint64_t hi, int k, uint64_t& rlo, uint64_t& rhi)
{
    const uint64_t a = ~bl::pairrev64(hi), b = ~bl::pairrev64(lo);  // b:a = the complement reversed over all 64 pairs
    const int s = 128 - 2 * k;                                      // 0 .. 126
    if (s == 0) {
        rlo = a;
        rhi = b;
    } else if (s < 64) {
        rlo = (a >> s) | (b << (64 - s));
        rhi = b >> s;
    } else {
        rlo = s == 64 ? b : b >> (s - 64);
        rhi = 0;
    }
}

// Lane i < c.len: words = the candidate's 256-bit code string (CODE_WORDS_PADDED words, low word first, bases a .. a + 127 from the top).
// Returns bit t set iff alternative t — the code (original + 1 + t) & 3 at p — leaves this lane's k-mer not SOLID; orig: the code at p.
BL_DEV uint32_t test_lane(const TestParams& p, const uint32_t* words, const Candidate& c, int i, uint32_t& orig)
{
    const int k = (int)p.k;
    const int sh = 256 - 2 * (i + k), q = sh >> 5, bits = sh & 31;  // i + k <= 127: 2 <= sh <= 254
    uint32_t f[4];
    BL_UNROLL
    for (int j = 0; j < 4; ++j) {
        const int nb = 2 * k - 32 * j;
        const uint32_t m = nb >= 32 ? ~0u : (nb <= 0 ? 0u : (1u << nb) - 1u);
        f[j] = bl::funnel_shr(words[q + j + 1], words[q + j], bits) & m;
    }
    const uint64_t flo = ((uint64_t)f[1] << 32) | f[0], fhi = ((uint64_t)f[3] << 32) | f[2];
    uint64_t rlo = 0, rhi = 0;
    if (p.canonical) revcomp_kmer(flo, fhi, k, rlo, rhi);
    const int at = (int)(edit_position(c, p.k) - c.a) - i;  // the base of this k-mer that p is: 0 .. k - 1
    const int fbit = 2 * (k - 1 - at), rbit = 2 * at;
    orig = (uint32_t)((fbit < 64 ? flo >> fbit : fhi >> (fbit - 64)) & 3u);
    uint64_t lo[bllk::G], hi[bllk::G];
    uint32_t cnt[bllk::G];
    BL_UNROLL
    for (int t = 0; t < bllk::G; ++t) {
        const uint64_t code = (orig + 1u + (uint32_t)t) & 3u;
        lo[t] = flo;
        hi[t] = fhi;
        patch2(lo[t], hi[t], fbit, code);
        if (p.canonical) {
            uint64_t xlo = rlo, xhi = rhi;
            patch2(xlo, xhi, rbit, 3u - code);
            const bool less = xhi < hi[t] || (xhi == hi[t] && xlo < lo[t]);
            lo[t] = less ? xlo : lo[t];
            hi[t] = less ? xhi : hi[t];
        }
    }
    bllk::search_group(p.table, lo, hi, 7u, cnt);
    uint32_t fail = 0;
    BL_UNROLL
    for (int t = 0; t < 3; ++t)
        if (cnt[t] < p.min_count) fail |= 1u << t;
    return fail;
}

// lane 0: qualifying = bit t set iff alternative t made every k-mer of the run SOLID; from = the byte at p; orig = its code
BL_DEV uint32_t verdict(uint32_t qualifying, uint32_t orig, uint8_t from, const Candidate& c, uint32_t k, Edit& e)
{
    if (qualifying == 0) return V_NO_BASE;
    if (qualifying & (qualifying - 1)) return V_AMBIGUOUS;
    const uint32_t t = qualifying == 1 ? 0u : (qualifying == 2 ? 1u : 2u);
    const uint32_t code = (orig + 1u + t) & 3u;
    e.pos = edit_position(c, k);
    e.from = from;
    e.to = (uint8_t)(((0x54474341u >> (8 * code)) & 0xffu) | (from & 0x20u));  // "ACGT"[code] with the original's case bit
    e.support = (uint8_t)c.len;
    e.anchor = (uint8_t)c.anchor;
    e.reserved = 0;
    return V_EDIT;
}

// ---- pass 4: candidate i's edit goes to slot edit_sum[i]; nothing at or beyond the capacity
BL_DEV void compact_edit(const Edit* edits, const uint8_t* verdicts, const uint64_t* edit_sum, uint64_t i, Edit* out, uint64_t capacity)
{
    if (verdicts[i] != V_EDIT) return;
    const uint64_t at = edit_sum[i];
    if (at < capacity) out[at] = edits[i];
}

// ---- pass 5: edit i of n; bases: the new batch's n_bases bytes
BL_DEV void edit_at(const Edit* edits, uint64_t n_edits, uint64_t i, uint8_t* bases, uint64_t n_bases)
{
    if (i >= n_edits) return;
    const uint64_t pos = edits[i].pos;
    if (pos >= n_bases) return;
    if (i > 0 && edits[i - 1].pos == pos) return;  // among equal neighbours the first wins
    bases[pos] = edits[i].to;
}

}  // namespace blcr
