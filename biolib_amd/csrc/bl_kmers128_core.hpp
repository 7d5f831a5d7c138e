// bl_kmers128_core.hpp — per-thread body of the 128-bit k-mer scans (1 <= k <= 64): the dense scan bl_scan_kmers128 and the two
// passes of the hash sampler bl_scan_hash_sample128.  Compiled two ways like bl_scan_core.hpp: by hipcc for gfx950
// (bl_kmers128.hip) and by a host compiler under BL_CPU_EMU for tests/emu/emu_kmers128.cpp.
//
// Reference semantics reproduced (file:line in /root/reference), evaluated in KmerType = __uint128_t:
//   kmer_view.hpp:190-199   forward / reverse-complement registers, canonical = numeric minimum of the two 128-bit values
//                           (the reference's own reverse-strand term shifts a 64-bit operand by up to 126 bits: undefined for
//                           k >= 33; DESIGN.md §2 pins the intended meaning, as for minimizer_view)
//   hash.hpp:55-59          hash64::hash<__uint128_t>(value, seed): MurmurHash3_x64_128 over the 16 bytes of the value
//                           (low word first), first output word, seed truncated to 32 bits
//
// Layout: the tile of kmer_kernel — 256 lanes x 16 positions, codes and flags of NCHUNK_POS chunks in LDS.  A lane's 16 k-mers
// span at most 79 bases = the five code words of chunks tid .. tid+4.  There is no rolling state: the lane shifts its 160 bits of
// codes ONCE so that the k-mer at position s is the 2k bits from bit 2(15-s) on, and builds the reverse complement of all 80 bases
// ONCE, in which the k-mer at s lies at bit 2s whatever k is; a position then costs four v_alignbit_b32 with a scalar shift and four
// v_and with the (scalar) mask words per strand, and any single position can be rebuilt on its own (the record pass does).
#pragma once
#include "bl_scan_phases.hpp"

// The loop over a lane's 16 positions stays a loop (s is a scalar register, so are the shift amounts): unrolled, the compiler keeps the
// k-mers of many positions alive at once — 135 registers for the dense kernel and 212 for the sampler's first pass (3 and 2 waves per
// SIMD) against 61 and 59 rolled (7 waves), for the same instructions per position.
#if defined(__HIPCC__) && !defined(BL_CPU_EMU)
#define BL_ROLLED _Pragma("nounroll")
#else
#define BL_ROLLED
#endif

namespace bl {

constexpr int MAX_UNIT128 = 64;  // KmerType = __uint128_t

// the last lane reads codes up to chunk TPB-1+4 and flags up to chunk TPB-1+7 (gather_flags): inside the halo kmer_kernel stages
static_assert(TPB - 1 + (S - 1 + MAX_UNIT128 - 1) / 16 < NCHUNK_POS, "a lane's k-mers must lie in the staged chunks");
static_assert(TPB - 1 + 7 < NCHUNK_POS, "gather_flags reads eight chunks from the lane's own");
static_assert(S - 1 + MAX_UNIT128 < 128, "validity and sequence-end bits of a lane must fit Bits128");

struct Kmer128Params {
    const uint8_t* bases;
    int64_t n_bases;
    const uint32_t* start_bits;
    int64_t first, end;          // positions [first, end) are reported
    int64_t origin;              // 16-aligned, <= first
    int64_t pos_base;            // sampler: added to every reported position (bl_batch_set_origin)
    int32_t n_tiles;
    int32_t unit;
    uint32_t seed;
    int32_t canonical;
    int32_t drop_last;
    uint64_t hash_below;         // sampler: records are the k-mers with hash < hash_below
    // dense scan: indexed by position - first (nullable)
    uint64_t* out_value;         // two words per position: low, high
    uint64_t* out_hash;
    uint8_t* out_valid;
    // sampler: records in position order (nullable), at most `capacity` of them
    uint64_t* rec_value;         // two words per record: low, high
    uint64_t* rec_pos;
    uint64_t* rec_hash;
    uint64_t capacity;
    uint16_t* lane_masks;              // [n_tiles][TPB] pass 1 -> pass 2: bit s = the lane's position s is a record
    unsigned long long* tile_counts;   // [n_tiles] records of the tile (pass 1), then the prefix scan of bl_kernels.hip
    unsigned long long* tile_base;
    unsigned long long* block_base;
    unsigned long long* shards;        // [NSHARD][8]: count, xor low words, xor hashes, sum of hashes | xor of positions, xor high words
};

// stage_chunk (bl_scan_phases.hpp) stages the chunks of these scans too: the staging code only looks at these three fields
BL_DEV ScanParams kmer128_staging_params(const Kmer128Params& p)
{
    ScanParams lp{};
    lp.bases = p.bases;
    lp.n_bases = p.n_bases;
    lp.start_bits = p.start_bits;
    return lp;
}

struct Kmer128Acc {
    unsigned long long cnt, xlo, xhi, xh, sx;
};

// hash64::hash<__uint128_t>: MurmurHash3_x64_128 of a 16-byte key (one body block, no tail), first output word
BL_DEV uint64_t murmur64_u128(uint64_t lo, uint64_t hi, uint32_t seed)
{
    const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
    uint64_t h1 = seed, h2 = seed;
    const uint64_t k1 = mul64c(rotl64_31(mul64c(lo, c1)), c2);
    h1 ^= k1;
    h1 = rotl64(h1, 27) + h2;
    h1 = h1 * 5 + 0x52dce729;
    const uint64_t k2 = mul64c(rotl64(mul64c(hi, c2), 33), c1);
    h2 ^= k2;
    h2 = rotl64_31(h2) + h1;
    h2 = h2 * 5 + 0x38495ab5;
    h1 ^= 16; h2 ^= 16;
    h1 += h2; h2 += h1;
    h1 = fmix64(h1); h2 = fmix64(h2);
    return h1 + h2;
}

// What the 16 positions of a lane share.  All words little-endian (word 0 = bits 0..31).
struct Kmer128Lane {
    uint32_t u[5];  // the lane's 80 bases >> (130 - 2k): the forward k-mer at s is bits [2(15-s), 2(15-s) + 2k)
    uint32_t r[5];  // reverse complement of the 80 bases: the reverse-complement k-mer at s is bits [2s, 2s + 2k)
    uint32_t m[4];  // the low 2k bits
};

// codes: the lane's five chunks (codes[0] = bases 0..15, first base in the top pair)
BL_DEV void kmer128_lane_start(Kmer128Lane& L, const uint32_t* codes, int k, bool canonical)
{
    // 160 bits, low word first, zeros above: shifted right by whole words in three uniform stages, then by bits
    uint32_t a[10];
    BL_UNROLL
    for (int i = 0; i < 5; ++i) a[i] = codes[4 - i];
    BL_UNROLL
    for (int i = 5; i < 10; ++i) a[i] = 0;
    const int sh = 130 - 2 * k, q = sh >> 5, bits = sh & 31;
    if (q & 1) {
        BL_UNROLL
        for (int i = 0; i < 6; ++i) a[i] = a[i + 1];
    }
    if (q & 2) {
        BL_UNROLL
        for (int i = 0; i < 6; ++i) a[i] = a[i + 2];
    }
    if (q & 4) {
        BL_UNROLL
        for (int i = 0; i < 6; ++i) a[i] = a[i + 4];
    }
    BL_UNROLL
    for (int i = 0; i < 5; ++i) L.u[i] = funnel_shr(a[i + 1], a[i], bits);  // bits = 0: the low word itself
    BL_UNROLL
    for (int i = 0; i < 5; ++i) L.r[i] = canonical ? revcomp16(codes[i]) : 0u;
    BL_UNROLL
    for (int j = 0; j < 4; ++j) {
        const int nb = 2 * k - 32 * j;
        L.m[j] = nb >= 32 ? ~0u : (nb <= 0 ? 0u : (1u << nb) - 1u);
    }
}

// the (canonical) k-mer at the lane's position s, 0 <= s < 16
BL_DEV void kmer128_at(const Kmer128Lane& L, int s, bool canonical, uint64_t& lo, uint64_t& hi)
{
    uint32_t f[4];
    const int fs = 30 - 2 * s;
    BL_UNROLL
    for (int j = 0; j < 4; ++j) f[j] = funnel_shr(L.u[j + 1], L.u[j], fs) & L.m[j];
    lo = ((uint64_t)f[1] << 32) | f[0];
    hi = ((uint64_t)f[3] << 32) | f[2];
    if (canonical) {
        uint32_t c[4];
        BL_UNROLL
        for (int j = 0; j < 4; ++j) c[j] = funnel_shr(L.r[j + 1], L.r[j], 2 * s) & L.m[j];
        const uint64_t rlo = ((uint64_t)c[1] << 32) | c[0], rhi = ((uint64_t)c[3] << 32) | c[2];
        const bool less = rhi < hi || (rhi == hi && rlo < lo);  // numeric minimum of the two 128-bit values
        lo = less ? rlo : lo;
        hi = less ? rhi : hi;
    }
}

// bit s: a k-mer starts at the lane's position s, the position lies in [first, end) and — BL_FLAG_DROP_LAST — the k-mer does not
// end its sequence (quirk Q1).  Exactly kmer_thread's mask, for spans up to 64.
BL_DEV uint32_t kmer128_ok_mask(const Kmer128Params& p, const uint32_t* flags, int tid, int64_t j0, uint32_t& inrange)
{
    Bits128 good, start;
    gather_flags(flags, tid, good, start);
    inrange = range_mask(p.first - j0, p.end - j0) & 0xffffu;
    uint32_t ok = window_valid_mask(good, start, p.unit) & inrange;
    if (p.drop_last) {
        uint32_t last = (uint32_t)b128_shr(start, p.unit).lo & 0xffffu;  // a sequence starts right after the k-mer at s
        const int64_t s_end = p.n_bases - p.unit - j0;                   // ... or the batch ends there
        if (s_end >= 0 && s_end < S) last |= 1u << s_end;
        ok &= ~last;
    }
    return ok;
}

struct alignas(16) U64x2 {
    uint64_t lo, hi;
};

// Dense scan: every position's value / hash / validity (any of the arrays may be missing), digest folded into acc.
BL_DEV void kmer128_dense_thread(const Kmer128Params& p, const uint32_t* codes, const uint32_t* flags, int tid, int64_t q0, Kmer128Acc& acc)
{
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    uint32_t inrange;
    const uint32_t ok = kmer128_ok_mask(p, flags, tid, j0, inrange);
    Kmer128Lane L;
    kmer128_lane_start(L, codes + tid, p.unit, p.canonical != 0);
    const bool any_out = p.out_value || p.out_hash || p.out_valid;  // uniform: the digest-only scan stores nothing
    // every lane of the wave counts all 16 of its positions: nothing to mask (as in kmer_thread)
    const bool plain = !any_out && !wave_any(ok != 0xffffu);
    BL_ROLLED
    for (int s = 0; s < S; ++s) {
        uint64_t lo, hi;
        kmer128_at(L, s, p.canonical != 0, lo, hi);
        const uint64_t h = murmur64_u128(lo, hi, p.seed);
        if (plain) {
            acc.xlo ^= lo;
            acc.xhi ^= hi;
            acc.xh ^= h;
            acc.sx += h;
            continue;
        }
        const uint32_t m32 = 0u - ((ok >> s) & 1u);
        const uint64_t m = ((uint64_t)m32 << 32) | m32;
        const uint64_t lom = lo & m, him = hi & m, hm = h & m;
        acc.xlo ^= lom;
        acc.xhi ^= him;
        acc.xh ^= hm;
        acc.sx += hm;
        if (any_out && ((inrange >> s) & 1)) {
            const int64_t o = j0 + s - p.first;
            if (p.out_value) reinterpret_cast<U64x2*>(p.out_value)[o] = U64x2{lom, him};  // one 16-byte store
            if (p.out_hash) p.out_hash[o] = hm;
            if (p.out_valid) p.out_valid[o] = (uint8_t)(m32 & 1u);
        }
    }
    acc.cnt += (unsigned)__builtin_popcount(ok);
}

// Sampler, pass 1: which of the lane's positions are records (valid k-mer, hash below the threshold), digest folded into acc
// (sx: XOR of the records' reported positions).  Returns the lane's record mask.
BL_DEV uint32_t kmer128_count_thread(const Kmer128Params& p, const uint32_t* codes, const uint32_t* flags, int tid, int64_t q0, Kmer128Acc& acc)
{
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    uint32_t inrange;
    const uint32_t ok = kmer128_ok_mask(p, flags, tid, j0, inrange);
    Kmer128Lane L;
    kmer128_lane_start(L, codes + tid, p.unit, p.canonical != 0);
    uint32_t sel = 0;
    BL_ROLLED
    for (int s = 0; s < S; ++s) {
        uint64_t lo, hi;
        kmer128_at(L, s, p.canonical != 0, lo, hi);
        const uint64_t h = murmur64_u128(lo, hi, p.seed);
        const uint32_t take = ((ok >> s) & 1u) & (h < p.hash_below ? 1u : 0u);
        const uint32_t m32 = 0u - take;
        const uint64_t m = ((uint64_t)m32 << 32) | m32;
        acc.xlo ^= lo & m;
        acc.xhi ^= hi & m;
        acc.xh ^= h & m;
        acc.sx ^= (uint64_t)(p.pos_base + j0 + s) & m;
        sel |= take << s;
    }
    acc.cnt += (unsigned)__builtin_popcount(sel);
    return sel;
}

// Sampler, pass 2: the lane's records (mask of pass 1) rebuilt one by one and stored from record index `at` on, in position order.
BL_DEV void kmer128_emit_thread(const Kmer128Params& p, const uint32_t* codes, int tid, int64_t q0, uint32_t sel, uint64_t at)
{
    if (sel == 0) return;
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    Kmer128Lane L;
    kmer128_lane_start(L, codes + tid, p.unit, p.canonical != 0);
    while (sel) {
        const int s = __builtin_ctz(sel);
        sel &= sel - 1;
        if (at >= p.capacity) return;  // nothing is written at or beyond capacity
        uint64_t lo, hi;
        kmer128_at(L, s, p.canonical != 0, lo, hi);
        if (p.rec_value) reinterpret_cast<U64x2*>(p.rec_value)[at] = U64x2{lo, hi};
        if (p.rec_pos) p.rec_pos[at] = (uint64_t)(p.pos_base + j0 + s);
        if (p.rec_hash) p.rec_hash[at] = murmur64_u128(lo, hi, p.seed);
        ++at;
    }
}

// tiles of a range, as bl_scan_kmers plans them
BL_DEV void plan_kmers128(int64_t first, int64_t end, Kmer128Params& p)
{
    p.first = first;
    p.end = end;
    p.origin = align_down16(first);
    p.n_tiles = end > first ? (int32_t)((end - 1 - p.origin) / H + 1) : 0;
}

}  // namespace bl
