// bl_minimizers128_core.hpp — per-thread bodies of bl_scan_minimizers128: window minimizers of k-mers up to k = 64
// (sampler::minimizer_sampler over kmer_view<__uint128_t>), the units hashed as 16-byte keys.  Compiled two ways like
// bl_kmers128_core.hpp: by hipcc for gfx950 (bl_minimizers128.hip) and by a host compiler under BL_CPU_EMU for
// tests/emu/emu_minimizers128.cpp.
//
// The rule (include/biolib_amd.h): the units, their validity and canonical form are bl_scan_kmers128's; a window is w
// consecutive valid units, its occurrence the LEFTMOST smallest hash; window p is a record iff it exists and window p-1 does not
// exist or has another occurrence.
//
// Layout: the tile of the 128-bit k-mer kernels — 256 lanes x 16 window starts — staged from ONE CHUNK BEHIND the tile's first
// window: staged position sp = q - (q0 - 16).  The chunk in front holds the unit at q0 - 1, whose window decides whether the tile's
// first window continues an occurrence.  A workgroup runs
//   phase A  every lane hashes the (canonical) units at its 16 positions and writes their 16 validity bits; lanes 0 .. w-2 hash one
//            position each of the halo behind the tile, lane w-1 the unit in front of it; lanes 0 .. 4 the validity of the five
//            chunks no lane owns
//   phase B  every lane folds its 16 windows over the hash array (bl_syncmers128_core.hpp's core + suffix / prefix minima), decides
//            its records, rebuilds the records' units and folds the digest
// The canonical value has ONE hash per position, so one round and one array do for both strands.
//
// Whether window t continues window t-1's occurrence needs no neighbour: with both windows present, and m the leftmost minimum of the
// w-1 units they share, occ(t-1) = (h[t-1] <= h[m] ? t-1 : m) and occ(t) = (h[m] <= h[t+w-1] ? m : t+w-1).  They are equal iff
// occ(t) != t+w-1 and h[t-1] > h[occ(t)] — one comparison of the hash left of the window with the window's minimum.  And with
// window t present, window t-1 is present iff unit t-1 is valid.
#pragma once
#include "bl_kmers128_core.hpp"

namespace bl {

constexpr int MIN128_NCHUNK = NCHUNK_POS + 4;             // staged chunks: one in front of the tile, H / 16 of it, 11 behind
constexpr int MIN128_NPOS = 16 + H + MAX_W;               // staged positions that are hashed: sp = 15 (q0 - 1) .. 16 + H + w - 2
constexpr int MIN128_SLOTS = MIN128_NPOS + MIN128_NPOS / 16;
constexpr int MIN128_NVALID = TPB + 5;                     // chunks with validity bits: lane tid reads those of chunks tid .. tid + 5

// the rightmost halo unit starts at sp = 16 + H - 1 + MAX_W - 1 and ends MAX_UNIT128 - 1 bases on
static_assert(16 + H + MAX_W - 2 < MIN128_NPOS, "the windows of a tile must lie in the hash array");
static_assert((16 + H + MAX_W - 2) / 16 + 4 < MIN128_NCHUNK, "the five code words of the last halo unit must be staged");
static_assert(MIN128_NVALID - 1 + 7 < MIN128_NCHUNK, "gather_flags reads eight chunks from the one whose validity it takes");
static_assert((16 + H + MAX_W - 2 + MAX_UNIT128 - 1) / 16 < MIN128_NCHUNK, "the last halo unit's last base must be staged");
static_assert((16 * TPB - 1 + S + MAX_W - 1) / 16 < MIN128_NVALID, "unit p0 - 1 and the units of a lane's 16 windows must have validity bits");
static_assert(MAX_W <= TPB && MIN128_NCHUNK <= 2 * TPB, "one lane per halo position, two staging steps");

// LDS index of staged position sp: one pad word after every 16 (bl_syncmers128_core.hpp: sync128_slot)
BL_DEV int min128_slot(int sp) { return sp + (sp >> 4); }

struct Min128Params {
    Kmer128Params km;     // the units (unit = k), the range of window starts, rec_* / capacity, lane_masks, tile counts and bases, shards
    int32_t w;
    uint32_t* lane_offs;  // [n_tiles][3][TPB] pass 1 -> pass 2: the 16 six-bit offsets of a lane's occurrences in their windows
};

// validity of the 16 units that start in staged chunk c (first position j0): kmer128_ok_mask without the range — windows read units
// outside it
BL_DEV uint32_t min128_unit_ok(const Kmer128Params& p, const uint32_t* flags, int c, int64_t j0)
{
    Bits128 good, start;
    gather_flags(flags, c, good, start);
    uint32_t ok = window_valid_mask(good, start, p.unit) & 0xffffu;
    if (p.drop_last) {
        uint32_t last = (uint32_t)b128_shr(start, p.unit).lo & 0xffffu;  // a sequence starts right after the unit
        const int64_t s_end = p.n_bases - p.unit - j0;                   // ... or the batch ends there
        if (s_end >= 0 && s_end < S) last |= 1u << s_end;
        ok &= ~last;
    }
    return ok;
}

// Phase A.  codes / flags: MIN128_NCHUNK chunks staged from r0 = q0 - 16; hash: MIN128_SLOTS words; valid: MIN128_NVALID words
BL_DEV void min128_hash_thread(const Min128Params& p, const uint32_t* codes, const uint32_t* flags, uint64_t* hash, uint16_t* valid, int tid, int64_t r0)
{
    const bool canonical = p.km.canonical != 0;
    Kmer128Lane L;
    kmer128_lane_start(L, codes + tid + 1, p.km.unit, canonical);
    const int at = min128_slot(16 * (tid + 1));
    BL_ROLLED
    for (int i = 0; i < S; ++i) {
        uint64_t lo, hi;
        kmer128_at(L, i, canonical, lo, hi);
        hash[at + i] = murmur64_u128(lo, hi, p.km.seed);
    }
    valid[tid + 1] = (uint16_t)min128_unit_ok(p.km, flags, tid + 1, r0 + 16 * (int64_t)(tid + 1));
    if (tid < p.w) {
        const int sp = tid < p.w - 1 ? 16 + H + tid : 15;
        kmer128_lane_start(L, codes + (sp >> 4), p.km.unit, canonical);
        uint64_t lo, hi;
        kmer128_at(L, sp & 15, canonical, lo, hi);
        hash[min128_slot(sp)] = murmur64_u128(lo, hi, p.km.seed);
    }
    if (tid < MIN128_NVALID - TPB) {
        const int c = tid == 0 ? 0 : TPB + tid;
        valid[c] = (uint16_t)min128_unit_ok(p.km, flags, c, r0 + 16 * (int64_t)c);
    }
}

// the 16 six-bit offsets of a lane: windows 0 .. 9 in a, 10 .. 15 in b
struct Min128Offs {
    uint64_t a, b;
};
BL_DEV int min128_off(const Min128Offs& o, int t) { return (int)((t < 10 ? o.a >> (6 * t) : o.b >> (6 * (t - 10))) & 63u); }

// pass 1 -> pass 2: the 96 bits of a lane in three dwords of lane_offs, [tile][3][TPB].  a has 60 bits and b 36: the four bits of b
// above its low dword (window 15's offset from 4 on) ride on top of a's high dword
BL_DEV void min128_offs_store(uint32_t* lane_offs, int tile, int tid, const Min128Offs& o)
{
    uint32_t* d = lane_offs + (size_t)tile * 3 * TPB + tid;
    d[0] = (uint32_t)o.a;
    d[TPB] = (uint32_t)(o.a >> 32) | ((uint32_t)(o.b >> 32) << 28);
    d[2 * TPB] = (uint32_t)o.b;
}
BL_DEV Min128Offs min128_offs_load(const uint32_t* lane_offs, int tile, int tid)
{
    const uint32_t* d = lane_offs + (size_t)tile * 3 * TPB + tid;
    return Min128Offs{((uint64_t)(d[TPB] & 0x0fffffffu) << 32) | d[0], ((uint64_t)(d[TPB] >> 28) << 32) | d[2 * TPB]};
}

// Phase B: bit t of the result = window t of the lane (start at staged position 16 (tid + 1) + t) is a record; offs: the offset of every
// window's occurrence from the window's start, the leftmost of equal minima.
// w >= 16: the 16 windows share the core [15, w-1] (offsets from the lane's first position).  Its minimum is taken once; window t adds
// the suffix [t, 14] on the left and the prefix [w, w+t-1] on the right.  The prefix minimum runs along with t; of the suffix minima
// only the positions are kept (16 nibbles) and the hash is read again: w + 46 reads for the lane instead of 16 w, and both loops stay
// ROLLED — with the minima of both sides in registers (bl_syncmers128_core.hpp, 30 more registers) and this kernel's extra state the
// unrolled form took 190 registers, two waves per SIMD.  w < 16: no common core, every window is read on its own.
BL_DEV uint32_t min128_window_thread(const Min128Params& p, const uint64_t* hash, const uint16_t* valid, int tid, int64_t r0, Min128Offs& offs)
{
    const int w = p.w;
    const int p0 = 16 * (tid + 1);
    // unit validity from staged position p0 - 1 on: 81 bits
    Bits128 v{(uint64_t)valid[tid] | ((uint64_t)valid[tid + 1] << 16) | ((uint64_t)valid[tid + 2] << 32) | ((uint64_t)valid[tid + 3] << 48),
              (uint64_t)valid[tid + 4] | ((uint64_t)valid[tid + 5] << 16)};
    v = b128_shr(v, 15);
    const uint32_t prev = (uint32_t)v.lo & 0xffffu;                       // bit t: the unit left of window t is valid
    const uint32_t exist = (uint32_t)(and_run(v, w).lo >> 1) & 0xffffu;   // bit t: window t exists
    const int64_t j0 = r0 + p0;
    const uint32_t want = exist & range_mask(p.km.first - j0, p.km.end - j0);
    uint32_t cont = 0;  // bit t: window t has the occurrence window t-1 would have
    offs.a = offs.b = 0;
    if (w < 16) {
        BL_ROLLED
        for (int t = 0; t < S; ++t) {
            uint64_t best = hash[min128_slot(p0 + t)];
            int arg = 0;
            for (int j = 1; j < w; ++j) {
                const uint64_t h = hash[min128_slot(p0 + t + j)];
                const bool take = h < best;
                best = take ? h : best;
                arg = take ? j : arg;
            }
            const uint64_t left = hash[min128_slot(p0 + t - 1)];
            cont |= (uint32_t)(arg != w - 1 && left > best) << t;
            if (t < 10) offs.a |= (uint64_t)arg << (6 * t);
            else offs.b |= (uint64_t)arg << (6 * (t - 10));
        }
        return want & ~(cont & prev);
    }
    uint64_t cm = hash[min128_slot(p0 + 15)];
    int ci = 15;
    for (int j = 16; j < w; ++j) {
        const uint64_t h = hash[min128_slot(p0 + j)];
        const bool take = h < cm;
        cm = take ? h : cm;
        ci = take ? j : ci;
    }
    // suffix minima of [t, 14], t = 14 .. 0: only their positions are kept (nibble t); the hash is read again where it is needed
    uint64_t sfx = 0, lm = 0;
    uint32_t li = 0;
    BL_ROLLED
    for (int t = S - 2; t >= 0; --t) {
        const uint64_t h = hash[min128_slot(p0 + t)];
        const bool take = t == S - 2 || h <= lm;  // prepended on the left
        lm = take ? h : lm;
        li = take ? (uint32_t)t : li;
        sfx |= (uint64_t)li << (4 * t);
    }
    uint64_t pm = 0;  // minimum of the prefix [w, w+t-1], at pidx
    int pidx = 0;
    BL_ROLLED
    for (int t = 0; t < S; ++t) {
        uint64_t m = cm;
        int a = ci;
        if (t < S - 1) {
            const int i = (int)((sfx >> (4 * t)) & 15u);
            const uint64_t h = hash[min128_slot(p0 + i)];
            const bool core = cm < h;
            m = core ? cm : h;
            a = core ? ci : i;
        }
        if (t > 0) {
            const uint64_t h = hash[min128_slot(p0 + w + t - 1)];
            const bool take = t == 1 || h < pm;  // appended on the right
            pm = take ? h : pm;
            pidx = take ? w + t - 1 : pidx;
            const bool right = pm < m;
            m = right ? pm : m;
            a = right ? pidx : a;
        }
        const uint64_t left = hash[min128_slot(p0 + t - 1)];
        a -= t;
        cont |= (uint32_t)(a != w - 1 && left > m) << t;
        if (t < 10) offs.a |= (uint64_t)a << (6 * t);
        else offs.b |= (uint64_t)a << (6 * (t - 10));
    }
    return want & ~(cont & prev);
}

// the (canonical) unit at staged position sp; L holds the lane state of chunk `cur` (-1: none yet) — consecutive records mostly
// share it
BL_DEV void min128_unit_at(const Kmer128Params& p, const uint32_t* codes, int sp, Kmer128Lane& L, int& cur, uint64_t& lo, uint64_t& hi)
{
    const int c = sp >> 4;
    if (c != cur) {
        kmer128_lane_start(L, codes + c, p.unit, p.canonical != 0);
        cur = c;
    }
    kmer128_at(L, sp & 15, p.canonical != 0, lo, hi);
}

// Phase B, second half: the digest of the lane's records — values rebuilt from the codes, hashes from the array, sx the XOR of positions
BL_DEV void min128_digest_thread(const Kmer128Params& p, const uint32_t* codes, const uint64_t* hash, int tid, int64_t r0, uint32_t sel,
                                 const Min128Offs& offs, Kmer128Acc& acc)
{
    Kmer128Lane L;
    int cur = -1;
    for (; sel; sel &= sel - 1) {
        const int t = __builtin_ctz(sel);
        const int sp = 16 * (tid + 1) + t + min128_off(offs, t);
        uint64_t lo, hi;
        min128_unit_at(p, codes, sp, L, cur, lo, hi);
        acc.xlo ^= lo;
        acc.xhi ^= hi;
        acc.xh ^= hash[min128_slot(sp)];
        acc.sx ^= (uint64_t)(p.pos_base + r0 + sp);
    }
}

// Pass 2: the lane's records (mask and offsets of pass 1) rebuilt one by one and stored from record index `at` on, in window order;
// nothing at or beyond capacity.  codes: staged as in pass 1.
BL_DEV void min128_emit_thread(const Kmer128Params& p, const uint32_t* codes, int tid, int64_t r0, uint32_t sel, const Min128Offs& offs, uint64_t at)
{
    Kmer128Lane L;
    int cur = -1;
    for (; sel; sel &= sel - 1, ++at) {
        if (at >= p.capacity) return;
        const int t = __builtin_ctz(sel);
        const int sp = 16 * (tid + 1) + t + min128_off(offs, t);
        uint64_t lo, hi;
        min128_unit_at(p, codes, sp, L, cur, lo, hi);
        if (p.rec_value) reinterpret_cast<U64x2*>(p.rec_value)[at] = U64x2{lo, hi};  // one 16-byte store
        if (p.rec_pos) p.rec_pos[at] = (uint64_t)(p.pos_base + r0 + sp);
        if (p.rec_hash) p.rec_hash[at] = murmur64_u128(lo, hi, p.seed);
    }
}

}  // namespace bl
