// bl_superkmer128_core.hpp — per-thread bodies of the 32-byte super-k-mer record (k up to 64): pack, expand, k-mer and minimizer
// extraction, and the slot protocol of the counter's LDS table with 16-byte keys.  Compiled two ways like bl_kmers128_core.hpp: by
// hipcc for gfx950 (bl_superkmer128.hip) and by a host compiler under BL_CPU_EMU for tests/emu/emu_superkmer128.cpp.
//
// The record (include/biolib_amd.h): four 64-bit words per group of size k-mers = size + k - 1 <= 122 bases,
//   word 0  bases 0..31, word 1  bases 32..63, word 2  bases 64..95   (2 bits per base, first base in the most significant pair)
//   word 3  bases 96..121 in bits 63..12, mm_pos in bits 11..6, size - 1 in bits 5..0
// Read as eight CHUNKS of 16 bases (chunk 2i = high half of word i, chunk 2i+1 = its low half, the low 12 bits of chunk 7 cleared) the
// record is the code array of bl_kmers128_core.hpp: k-mer q of the record is position q & 15 of the lane that starts at chunk q >> 4,
// and the minimizer is the m-mer at mm_pos, the same way.  Both are taken with kmer128_lane_start / kmer128_at — there is no second
// extraction routine.  q and mm_pos are six-bit fields: q >> 4 <= 3, so the five chunks a lane reads are chunks <= 7 for ANY record
// bits; nothing here indexes by a value the record could push out of range.
#pragma once
#include "bl_kmers128_core.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
#define BL_LDS_CAS32(p, cmp, val) atomicCAS((p), (cmp), (val))
#define BL_LDS_ADD32(p, val) atomicAdd((p), (val))
#else  // the emulation runs the lanes one after the other
#define BL_LDS_CAS32(p, cmp, val) bl::emu_cas32((p), (cmp), (val))
#define BL_LDS_ADD32(p, val) (*(p) += (val))
#endif

namespace bl {

constexpr int SK128_MAX_BASES = 122;  // of one record
constexpr int SK128_CHUNKS = 8;

BL_DEV uint32_t emu_cas32(uint32_t* p, uint32_t cmp, uint32_t val)
{
    const uint32_t old = *p;
    if (old == cmp) *p = val;
    return old;
}

BL_DEV int sk128_size(uint64_t w3) { return (int)(w3 & 63u) + 1; }
BL_DEV int sk128_mm_pos(uint64_t w3) { return (int)((w3 >> 6) & 63u); }

// the record's eight chunks
BL_DEV void sk128_chunks(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t* c)
{
    c[0] = (uint32_t)(w0 >> 32); c[1] = (uint32_t)w0;
    c[2] = (uint32_t)(w1 >> 32); c[3] = (uint32_t)w1;
    c[4] = (uint32_t)(w2 >> 32); c[5] = (uint32_t)w2;
    c[6] = (uint32_t)(w3 >> 32); c[7] = (uint32_t)w3 & ~0xfffu;
}

// chunks c0 .. c0+4 of a record held in registers, 0 <= c0 <= 3: selects instead of a dynamic index (which would send the array to
// scratch memory on the device)
BL_DEV void sk128_pick5(const uint32_t* c, int c0, uint32_t* out)
{
    BL_UNROLL
    for (int i = 0; i < 5; ++i) {
        const uint32_t a = (c0 & 1) ? c[i + 1] : c[i], b = (c0 & 1) ? c[i + 3] : c[i + 2];
        out[i] = (c0 & 2) ? b : a;
    }
}

// the same from a record in memory (LDS on the device) as eight dwords in memory order: dword j ^ 1 is chunk j
BL_DEV void sk128_load5(const uint32_t* rec32, int c0, uint32_t* out)
{
    BL_UNROLL
    for (int i = 0; i < 5; ++i) {
        const int j = c0 + i;  // <= 7
        const uint32_t v = rec32[j ^ 1];
        out[i] = j == 7 ? v & ~0xfffu : v;
    }
}

// the (canonical) t-mer at base `pos` (0..63) of the record whose chunks pos >> 4 .. are `five`: t = k for k-mer `pos`, t = m and
// pos = mm_pos for the minimizer (high word 0 for t <= 32)
BL_DEV void sk128_mer_at(const uint32_t* five, int pos, int t, bool canonical, uint64_t& lo, uint64_t& hi)
{
    Kmer128Lane L;
    kmer128_lane_start(L, five, t, canonical);
    kmer128_at(L, pos & 15, canonical, lo, hi);
}

// hash of the record's minimizer, as bl_scan_super_kmers hashed it: an 8-byte key (MinimizerType = uint64_t)
BL_DEV uint64_t sk128_minimizer_hash(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, int m, bool canonical, uint32_t seed)
{
    uint32_t c[SK128_CHUNKS], five[5];
    sk128_chunks(w0, w1, w2, w3, c);
    const int mp = sk128_mm_pos(w3);
    sk128_pick5(c, mp >> 4, five);
    uint64_t lo, hi;
    sk128_mer_at(five, mp, m, canonical, lo, hi);
    return murmur64(lo, seed);
}

// all k-mers of one record, in order, two words each (low, high), to dst[0 .. 2 size)
BL_DEV void sk128_expand(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, int k, bool canonical, uint64_t* dst)
{
    uint32_t c[SK128_CHUNKS];
    sk128_chunks(w0, w1, w2, w3, c);
    const int size = sk128_size(w3);
    BL_UNROLL
    for (int b = 0; b < 4; ++b) {
        if (16 * b >= size) break;
        Kmer128Lane L;
        kmer128_lane_start(L, c + b, k, canonical);
        const int n = size - 16 * b < 16 ? size - 16 * b : 16;
        BL_ROLLED
        for (int s = 0; s < n; ++s) {
            uint64_t lo, hi;
            kmer128_at(L, s, canonical, lo, hi);
            reinterpret_cast<U64x2*>(dst)[16 * b + s] = U64x2{lo, hi};
        }
    }
}

// ---- pack ---------------------------------------------------------------------------------------------------------------

// 8 bases at `at` as 16 bits of 2-bit codes, the first base in the two most significant bits: one (unaligned) 8-byte load where the
// batch has 8 bytes left, byte loads at its end (nothing behind n_bases is read)
struct __attribute__((packed)) Sk128Unaligned8 {
    uint64_t v;
};
BL_DEV uint64_t sk128_codes8(const uint8_t* bases, uint64_t at, uint64_t n_bases)
{
    uint64_t w = 0;
    if (n_bases >= 8 && at <= n_bases - 8) {  // (not `at + 8 <= n_bases`: a wrapped `at` must not pass)
        w = reinterpret_cast<const Sk128Unaligned8*>(bases + at)->v;
    } else {
        for (int i = 0; i < 8; ++i)
            if (at + i < n_bases) w |= (uint64_t)bases[at + i] << (8 * i);
    }
    w = __builtin_bswap64(w);                                 // first base in the most significant byte
    uint64_t x = ((w >> 1) ^ (w >> 2)) & 0x0303030303030303ULL;  // A0 C1 G2 T/U3 of all eight bytes (constants.hpp:12-21)
    x = (x | (x >> 6)) & 0x000f000f000f000fULL;
    x = (x | (x >> 12)) & 0x000000ff000000ffULL;
    x = (x | (x >> 24)) & 0xffffULL;
    return x;
}

// p = first_pos - origin as an unsigned value (a position in front of the origin is huge and packs an empty record); `size` and `mp`
// as the caller gave them.  The clipping contract is bl_pack_super_kmers'.
BL_DEV void sk128_pack(const uint8_t* bases, uint64_t n_bases, uint64_t p, int size, int mp, int k, uint64_t* w)
{
    int nb = size + k - 1;
    if (nb > SK128_MAX_BASES) nb = SK128_MAX_BASES;
    if (p >= n_bases) nb = 0;                                               // nothing of the batch: an empty record
    else if ((uint64_t)nb > n_bases - p) nb = (int)(n_bases - p);           // never read past the batch (neither guard adds to p)
    w[0] = w[1] = w[2] = w[3] = 0;
    BL_UNROLL
    for (int j = 0; j < 16; ++j)
        if (8 * j < nb) w[j >> 2] |= sk128_codes8(bases, p + 8 * j, n_bases) << (48 - 16 * (j & 3));
    BL_UNROLL
    for (int i = 0; i < 4; ++i) {  // bases beyond the record's own are not part of it
        const int rem = nb - 32 * i;
        if (rem <= 0) w[i] = 0;
        else if (rem < 32) w[i] &= ~0ULL << (64 - 2 * rem);
    }
    w[3] = (w[3] & ~0xfffULL) | ((uint64_t)(mp & 63) << 6) | (uint64_t)((size - 1) & 63);
}

// ---- the counter's table (one per wave) -----------------------------------------------------------------------------------
// No 128-bit compare-and-swap exists in LDS, and no key value is free to mark an empty slot (the all-T 64-mer is all ones), so a slot
// has an OWNER word: 0 = empty.  One probe step of the wave is
//   claim    every pending lane: 32-bit CAS 0 -> 1 on its slot's owner word; the lane that wins writes both key words
//   (wave_lds_sync: the keys written in this step are visible to the wave)
//   settle   every pending lane compares the slot's 128 bits with its own key: equal -> count it, done; otherwise step to the next slot
// A lane never waits for another: whatever the CAS returned, the slot it looks at after the sync holds a complete key — its own, a
// key written in this step by the lane that won, or one written in an earlier step.  A slot that is empty in step s+1 was looked at by
// nobody in step s (looking at a slot is preceded by the CAS that makes it non-empty), so the next step's key writes cannot race with
// this step's key reads.  The wave repeats the step while any lane is pending, at most CT128_SLOTS times; the caller keeps the table
// below CT128_FULL < CT128_SLOTS keys, so an empty slot or the key itself is met before the walk comes round.
constexpr int CT128_SLOTS = 1024;   // table slots of ONE WAVE
constexpr int CT128_CAP = 700;      // k-mers one ROUND of a bucket inserts (the work list's size)
constexpr int CT128_FULL = 820;     // DISTINCT k-mers a bucket's table may come to hold: beyond it the fallback counts the bucket
constexpr int CT128_RECS = 64;      // records a round stages (one per lane)
constexpr int CT128_MAXREC = 1023;  // records a bucket may hold at all: 1023 x 64 k-mers < 2^16, the width of a count
constexpr int CT128_WAVES = 2;      // waves per workgroup
static_assert(CT128_MAXREC * 64 < 65536, "counts are kept in 16 bits");
static_assert(CT128_FULL < CT128_SLOTS && CT128_CAP <= CT128_FULL && CT128_CAP >= 64, "a round fits the table; a record fits a round");
static_assert((CT128_SLOTS & (CT128_SLOTS - 1)) == 0 && CT128_SLOTS % 128 == 0, "slot arithmetic");

struct WaveTable128 {
    uint64_t klo[CT128_SLOTS];
    uint64_t khi[CT128_SLOTS];
    uint32_t owner[CT128_SLOTS];
    uint32_t cnt[CT128_SLOTS / 2];   // 16 bits per slot: slot h is half h & 1 of word h >> 1
    uint32_t recs[8 * CT128_RECS];   // the round's records, eight dwords each in memory order (dword 2i = low half of word i)
    uint16_t work[CT128_CAP + 4];    // k-mer j of the round = k-mer (entry & 63) of staged record (entry >> 6)
};

BL_DEV uint32_t table128_slot(uint64_t lo, uint64_t hi) { return (uint32_t)(((lo ^ (hi * 0x9E3779B97F4A7C15ULL)) * 0xD6E8FEB86659FD93ULL) >> (64 - 10)); }
static_assert((1 << 10) == CT128_SLOTS, "table128_slot spans the table");

BL_DEV bool table128_claim(WaveTable128& t, uint32_t h, uint64_t lo, uint64_t hi)
{
    if (BL_LDS_CAS32(&t.owner[h], 0u, 1u) != 0u) return false;
    t.klo[h] = lo;
    t.khi[h] = hi;
    return true;
}

// true: the key sits in slot h and has been counted; false: h has moved on
BL_DEV bool table128_settle(WaveTable128& t, uint32_t& h, uint64_t lo, uint64_t hi)
{
    if (t.klo[h] == lo && t.khi[h] == hi) {
        BL_LDS_ADD32(&t.cnt[h >> 1], 1u << (16 * (h & 1u)));
        return true;
    }
    h = (h + 1) & (uint32_t)(CT128_SLOTS - 1);
    return false;
}

BL_DEV uint32_t table128_count(const WaveTable128& t, uint32_t h) { return (t.cnt[h >> 1] >> (16 * (h & 1u))) & 0xffffu; }

BL_DEV void table128_stage(WaveTable128& t, int r, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3)
{
    uint32_t* d = &t.recs[8 * r];
    d[0] = (uint32_t)w0; d[1] = (uint32_t)(w0 >> 32);
    d[2] = (uint32_t)w1; d[3] = (uint32_t)(w1 >> 32);
    d[4] = (uint32_t)w2; d[5] = (uint32_t)(w2 >> 32);
    d[6] = (uint32_t)w3; d[7] = (uint32_t)(w3 >> 32);
}

// k-mer `entry & 63` of staged record `entry >> 6`
BL_DEV void table128_work_key(const WaveTable128& t, uint32_t entry, int k, bool canonical, uint64_t& lo, uint64_t& hi)
{
    const int q = (int)(entry & 63u);
    uint32_t five[5];
    sk128_load5(&t.recs[8 * (entry >> 6)], q >> 4, five);
    sk128_mer_at(five, q, k, canonical, lo, hi);
}

}  // namespace bl
