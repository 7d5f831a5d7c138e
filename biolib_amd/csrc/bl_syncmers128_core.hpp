// bl_syncmers128_core.hpp — per-thread bodies of bl_scan_syncmers128: syncmers of k-mers up to k = 64 (KmerType = __uint128_t) with
// s-mers up to s = 32 hashed as 16-byte keys.  Compiled two ways like bl_kmers128_core.hpp: by hipcc for gfx950 (bl_syncmers128.hip)
// and by a host compiler under BL_CPU_EMU for tests/emu/emu_syncmers128.cpp.
//
// Reference semantics reproduced (file:line in the reference), evaluated in KmerType = __uint128_t:
//   kmer_view.hpp:266-283   minimizer_position_extractor::operator(): `km & mask` is a 128-bit value with a zero high word, hashed by
//                           hash64::hash<__uint128_t> with seed argument; the `>=` loop from the right keeps the LEFTMOST minimum
//   syncmer_sampler.hpp     a k-mer is kept when that offset equals start_offset or end_offset
// The k-mers, their validity and their canonical form are bl_scan_kmers128's (bl_kmers128_core.hpp).
//
// Layout: the tile of the 128-bit k-mer kernels — 256 lanes x 16 k-mer start positions, codes and flags of NCHUNK_POS chunks in
// LDS — plus ONE array of 64-bit s-mer hashes for the tile's H + W - 1 s-mer positions.  A workgroup runs
//   phase A  every lane hashes the s-mers at its 16 positions (taken straight from the 2-bit codes: one 64-bit extraction), lanes
//            0 .. W-2 one position each of the halo behind the tile
//   phase B  every lane folds the W-wide windows of its 16 k-mers over the hash array
// once for the forward s-mers and, for canonical scans, once more for their reverse complements: ONE strand's hashes are in LDS at
// a time (35 KB, four workgroups per CU), not both (69 KB, two).  Nothing is computed twice for it — a lane's 16 k-mers lie on
// both strands in general, so a lane folds both strands' windows whichever way the hashes are kept; the price is two barriers.
//
// A canonical k-mer that is the reverse complement has its s-mer number j at forward position p + W-1 - j, as the reverse
// complement of the forward s-mer there: the leftmost minimum over j is the RIGHTMOST minimum over forward positions.
#pragma once
#include "bl_kmers128_core.hpp"

namespace bl {

constexpr int MAX_SMER128 = 32;                            // `km & mask`: the mask is a uint64_t (kmer_view.hpp:262)
constexpr int SYNC128_NPOS = H + MAX_W;                    // s-mer positions of a tile: H + W - 1 <= H + 63
constexpr int SYNC128_SLOTS = SYNC128_NPOS + SYNC128_NPOS / 16;

// the last k-mer's last s-mer, and that s-mer's last base, lie in the staged chunks
static_assert(H - 1 + MAX_W - 1 < SYNC128_NPOS, "the windows of a tile's k-mers must lie in the hash array");
static_assert((H + MAX_W - 2) / 16 + 2 < NCHUNK_POS, "an s-mer's three code words must lie in the staged chunks");
static_assert(MAX_W - 1 <= TPB, "one lane per halo position");

// LDS index of s-mer position q: one pad word after every 16, so that the lanes of a wave half — lane l reads position 16 l + j —
// hit 32 different bank pairs (34 l mod 64 takes every even value once) instead of two
BL_DEV int sync128_slot(int q) { return q + (q >> 4); }

struct Sync128Params {
    Kmer128Params km;      // the k-mers (unit = k), the range, rec_pos / capacity, lane_masks, tile counts and bases, shards
    int32_t s, w;          // s-mer length, w = k - s + 1 s-mers per k-mer
    int32_t fwd_a, fwd_b;  // forward strand: the k-mer at p is a record iff its leftmost minimum lies at p + fwd_a or p + fwd_b (-1: never)
    int32_t rev_a, rev_b;  // reverse strand: ... iff the rightmost minimum of the reverse-complement hashes lies at p + rev_a or p + rev_b
};

BL_DEV void plan_syncmers128(int k, int s, uint32_t start_offset, uint32_t end_offset, Sync128Params& p)
{
    p.km.unit = k;
    p.s = s;
    p.w = k - s + 1;
    const int w = p.w;
    p.fwd_a = start_offset < (uint32_t)w ? (int32_t)start_offset : -1;  // an offset >= w matches nothing
    p.fwd_b = end_offset < (uint32_t)w ? (int32_t)end_offset : -1;
    p.rev_a = p.fwd_a < 0 ? -1 : w - 1 - p.fwd_a;
    p.rev_b = p.fwd_b < 0 ? -1 : w - 1 - p.fwd_b;
}

// murmur64_u128(x, 0, seed): the second body block multiplies zero, k2 = 0 — six constant multiplies instead of eight
BL_DEV uint64_t murmur64_u128_lo(uint64_t x, uint32_t seed)
{
    const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
    uint64_t h1 = seed, h2 = seed;
    h1 ^= mul64c(rotl64_31(mul64c(x, c1)), c2);
    h1 = rotl64(h1, 27) + h2;
    h1 = h1 * 5 + 0x52dce729;
    h2 = rotl64_31(h2) + h1;
    h2 = h2 * 5 + 0x38495ab5;
    h1 ^= 16; h2 ^= 16;
    h1 += h2; h2 += h1;
    h1 = fmix64(h1); h2 = fmix64(h2);
    return h1 + h2;
}

// What the s-mers at the 16 positions of one chunk share.  Words little-endian (word 0 = bits 0..31).
struct Smer128Lane {
    uint32_t u[3];     // forward: the 48 bases >> (66 - 2s), the s-mer at i is bits [2(15-i), 2(15-i) + 2s)
                       // reverse: the reverse complement of the 48 bases, the s-mer's at i is bits [2i, 2i + 2s)
    uint32_t mlo, mhi; // the low 2s bits
};

// codes: three chunks (codes[0] = bases 0..15, first base in the top pair)
BL_DEV void smer128_lane_start(Smer128Lane& L, const uint32_t* codes, int s, bool rc)
{
    if (rc) {
        BL_UNROLL
        for (int i = 0; i < 3; ++i) L.u[i] = revcomp16(codes[i]);
    } else {
        uint32_t a[6] = {codes[2], codes[1], codes[0], 0u, 0u, 0u};
        const int sh = 66 - 2 * s, q = sh >> 5, bits = sh & 31;  // 2 .. 64
        if (q & 1) {
            BL_UNROLL
            for (int i = 0; i < 4; ++i) a[i] = a[i + 1];
        }
        if (q & 2) {
            BL_UNROLL
            for (int i = 0; i < 4; ++i) a[i] = a[i + 2];
        }
        BL_UNROLL
        for (int i = 0; i < 3; ++i) L.u[i] = funnel_shr(a[i + 1], a[i], bits);  // bits = 0: the low word itself
    }
    L.mlo = s >= 16 ? ~0u : (1u << (2 * s)) - 1u;
    L.mhi = s >= 32 ? ~0u : (s <= 16 ? 0u : (1u << (2 * s - 32)) - 1u);
}

// the s-mer (rc: its reverse complement) at position i of the chunk, 0 <= i < 16
BL_DEV uint64_t smer128_at(const Smer128Lane& L, int i, bool rc)
{
    const int sh = rc ? 2 * i : 30 - 2 * i;
    const uint32_t lo = funnel_shr(L.u[1], L.u[0], sh) & L.mlo, hi = funnel_shr(L.u[2], L.u[1], sh) & L.mhi;
    return ((uint64_t)hi << 32) | lo;
}

// Phase A: the hashes of one strand's s-mers into hash[] (SYNC128_SLOTS words): positions 16 tid .. 16 tid + 15, and H + tid for tid < w - 1
BL_DEV void sync128_hash_thread(const Sync128Params& p, const uint32_t* codes, uint64_t* hash, int tid, bool rc)
{
    Smer128Lane L;
    smer128_lane_start(L, codes + tid, p.s, rc);
    const int at = sync128_slot(16 * tid);
    BL_ROLLED
    for (int i = 0; i < S; ++i) hash[at + i] = murmur64_u128_lo(smer128_at(L, i, rc), p.km.seed);
    if (tid < p.w - 1) {
        const int q = H + tid;
        smer128_lane_start(L, codes + (q >> 4), p.s, rc);
        hash[sync128_slot(q)] = murmur64_u128_lo(smer128_at(L, q & 15, rc), p.km.seed);
    }
}

// bit t: a valid k-mer starts at the lane's position t (kmer128_ok_mask); strand bit t: its reverse complement is the smaller value
BL_DEV uint32_t sync128_ok_strand(const Kmer128Params& p, const uint32_t* codes, const uint32_t* flags, int tid, int64_t q0, uint32_t& strand)
{
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    uint32_t inrange;
    const uint32_t ok = kmer128_ok_mask(p, flags, tid, j0, inrange);
    strand = 0;
    if (p.canonical) {
        Kmer128Lane L;
        kmer128_lane_start(L, codes + tid, p.unit, true);
        BL_ROLLED
        for (int t = 0; t < S; ++t) {
            uint64_t lo, hi, flo, fhi;
            kmer128_at(L, t, true, lo, hi);
            kmer128_at(L, t, false, flo, fhi);
            strand |= (uint32_t)(lo != flo || hi != fhi) << t;  // equal values (a k-mer that is its own reverse complement): forward
        }
    }
    return ok;
}

// Phase B: bit t of the result = the minimum of hash[16 tid + t .. + w - 1] lies at offset ta or tb of that window; of equal minima the
// leftmost counts (LEFT) or the rightmost.
// w >= 16: the 16 windows share the core [15, w-1] (offsets from the lane's first position).  Its minimum is taken once; window t adds
// the suffix [t, 14] on the left and the prefix [w, w+t-1] on the right, whose running minima cost one read per element: w + 15 reads
// for the lane instead of 16 w.  The prefix minima are kept in registers (the loops are unrolled: constant indices), the suffix
// minima run against them.  w < 16: no common core, every window is read on its own (at most 15 x 16 reads).
template <bool LEFT>
BL_DEV uint32_t sync128_window_thread(const uint64_t* hash, int tid, int w, int ta, int tb)
{
    const int p0 = 16 * tid;
    uint32_t hit = 0;
    if (w < 16) {
        BL_ROLLED
        for (int t = 0; t < S; ++t) {
            uint64_t best = hash[sync128_slot(p0 + t)];
            int arg = 0;
            for (int j = 1; j < w; ++j) {
                const uint64_t h = hash[sync128_slot(p0 + t + j)];
                const bool take = LEFT ? h < best : h <= best;
                best = take ? h : best;
                arg = take ? j : arg;
            }
            hit |= (uint32_t)(arg == ta || arg == tb) << t;
        }
        return hit;
    }
    uint64_t cm = hash[sync128_slot(p0 + 15)];
    int ci = 15;
    for (int j = 16; j < w; ++j) {
        const uint64_t h = hash[sync128_slot(p0 + j)];
        const bool take = LEFT ? h < cm : h <= cm;
        cm = take ? h : cm;
        ci = take ? j : ci;
    }
    uint64_t ph[S];  // ph[t], pi[t]: minimum of [w, w+t-1], t = 1 .. 15
    int pi[S];
    ph[0] = 0;
    pi[0] = 0;
    BL_UNROLL
    for (int t = 1; t < S; ++t) {
        const uint64_t h = hash[sync128_slot(p0 + w + t - 1)];
        const bool take = t == 1 || (LEFT ? h < ph[t - 1] : h <= ph[t - 1]);  // appended on the right
        ph[t] = take ? h : ph[t - 1];
        pi[t] = take ? w + t - 1 : pi[t - 1];
    }
    uint64_t lm = 0;
    int li = 0;
    BL_UNROLL
    for (int t = S - 1; t >= 0; --t) {
        uint64_t m = cm;
        int a = ci;
        if (t < S - 1) {
            const uint64_t h = hash[sync128_slot(p0 + t)];
            const bool take = t == S - 2 || (LEFT ? h <= lm : h < lm);  // prepended on the left
            lm = take ? h : lm;
            li = take ? t : li;
            const bool core = LEFT ? cm < lm : cm <= lm;
            m = core ? cm : lm;
            a = core ? ci : li;
        }
        if (t > 0) {
            const bool right = LEFT ? ph[t] < m : ph[t] <= m;
            a = right ? pi[t] : a;
        }
        a -= t;
        hit |= (uint32_t)(a == ta || a == tb) << t;
    }
    return hit;
}

// the lane's records: XOR of their reported positions into xor_pos; returns the mask
BL_DEV uint32_t sync128_select(const Kmer128Params& p, int tid, int64_t q0, uint32_t ok, uint32_t strand, uint32_t hit_fwd, uint32_t hit_rev,
                               unsigned long long& xor_pos)
{
    const uint32_t sel = ok & ((hit_fwd & ~strand) | (hit_rev & strand));
    const int64_t j0 = p.pos_base + q0 + 16 * (int64_t)tid;
    for (uint32_t m = sel; m; m &= m - 1) xor_pos ^= (unsigned long long)(j0 + __builtin_ctz(m));
    return sel;
}

// Pass 2: the lane's records (mask of pass 1) from record index `at` on, in position order; nothing at or beyond capacity
BL_DEV void sync128_emit_thread(const Kmer128Params& p, int tid, int64_t q0, uint32_t sel, uint64_t at)
{
    const int64_t j0 = p.pos_base + q0 + 16 * (int64_t)tid;
    for (; sel; sel &= sel - 1, ++at) {
        if (at >= p.capacity) return;
        p.rec_pos[at] = (uint64_t)(j0 + __builtin_ctz(sel));
    }
}

}  // namespace bl
