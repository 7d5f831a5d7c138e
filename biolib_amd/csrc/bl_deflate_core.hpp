// bl_deflate_core.hpp — DEFLATE (RFC 1951) encoder for ONE wavefront per BGZF member, the inflate kernel run backwards: a member is at
// most 65,280 bytes of text and an independent deflate stream, so the members of a text are compressed side by side, one wave each.
// Compiled two ways: by hipcc for gfx950 (bl_deflate.hip) and by a host compiler under BL_CPU_EMU for tests/emu/emu_deflate.cpp, where a
// lane block (BLD_LANES) is a loop over 64 lanes, per-lane values (PerLane) are arrays and LDS is a struct.  tests/deflate_cases.py
// restates every rule below in Python; the two must give the same bytes.
//
// A member in six phases (all loops are bounded by the member's byte count n <= 65,280; the bound of each is stated where it stands):
//   0  literal price   byte histogram of the text -> LIT4, the average cost of a literal in quarter bits (integer arithmetic only)
//   1  parse           LZ77 over the member's own text, 64 positions per step: per lane up to three candidates (the byte before, the
//                      last position with the same 3 bytes, the last with the same 8 bytes: two u16 tables in LDS that hold positions of
//                      EARLIER steps only), the best of them by  score = len * LIT4 - 4 * (12 + extra bits of the distance)  (>= 0 to be
//                      taken, ties to the smaller distance), then a wave-uniform greedy selection.  Tokens go to the wave's area of
//                      scratch, their symbols into the two histograms in LDS.
//   2  code build      Huffman lengths of both alphabets from the histograms (rank sort by (count, symbol) across the lanes, two-queue
//                      merge, depths), limited to 15 bits by the count-per-length adjustment, reassigned in frequency order
//   3  sizes           the exact bit count of the fixed and of the dynamic form; the smallest of stored / fixed / dynamic in bytes,
//                      ties in that order
//   4  CRC-32          slices and their combination (bl_crc_wave.hpp)
//   5  emission        header, block and trailer through one bit emitter: per 64 pieces an exclusive sum of bit counts, every lane's
//                      bits OR-ed into an LDS staging area at the place so computed, whole dwords stored to the member's slot
// The dynamic header uses no repeat symbols: code-length symbols 0..15 get 4 bits each, 16..18 none, HCLEN is 19.
//
// Safety: no byte at or behind text[n] is read whatever the alignment of `text` (8-byte compares only where 8 bytes are inside);
// the slot is written up to the dword that holds the member's last byte; no atomic decides a placement (LDS adds count, LDS ors merge
// bits at computed places; the position tables take the highest position of a step by a write / read-back loop); reruns are bit-equal.
#pragma once
#include <cstdint>
#include <cstring>

#include "bl_crc_wave.hpp"

#if defined(BL_CPU_EMU)
#define BLD_DEV inline
#define BLD_LANES(l) for (int l = 0; l < 64; ++l)
#define BLD_SYNC() ((void)0)
#define BLD_GLOBAL_SYNC() ((void)0)
#else
#define BLD_DEV __device__ __forceinline__
#define BLD_LANES(l) for (int l = (int)(threadIdx.x & 63u), once_ = 1; once_; once_ = 0)
// LDS operations of one wave complete in program order; the fence keeps the compiler from moving accesses across the point where the
// lanes exchange roles (written by one lane, read by another)
#define BLD_SYNC()                                             \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
// the same for what the lanes exchange through global memory (the tokens): the stores have completed before another lane loads them
#define BLD_GLOBAL_SYNC()                                      \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); \
        __builtin_amdgcn_wave_barrier();                       \
    } while (0)
#endif

namespace bl_deflate {

constexpr uint32_t MEMBER_TEXT = 65280;             // bgzip's 0xff00
constexpr uint32_t MEMBER_OVERHEAD = 31;            // header 18 + stored block 5 + trailer 8: no member is larger than its text + this
constexpr uint32_t SLOT_BYTES = 65344;              // a member's slot: MEMBER_TEXT + MEMBER_OVERHEAD, the dword behind it, to 64 bytes
constexpr uint32_t MAX_TOKENS = MEMBER_TEXT;        // every token covers at least one byte
constexpr uint32_t MAX_LEN = 258, MAX_DIST = 32768;
constexpr int T3_BITS = 12, T8_BITS = 13;
constexpr uint32_t N_LL = 286, N_D = 30, D_OFF = 288, N_SYMS = 320;
constexpr uint32_t TOKEN_MATCH = 1u << 31;          // match token: bit 31, (distance - 1) << 8, length - 3; a literal token is its byte
constexpr uint32_t NO_HASH = 0xffffffffu;
constexpr uint32_t FORM_STORED = 0, FORM_FIXED = 1, FORM_DYNAMIC = 2;
constexpr uint32_t MATCH_BASE_BITS = 12;            // what a match is taken to cost besides its distance's extra bits

static_assert(SLOT_BYTES >= MEMBER_TEXT + MEMBER_OVERHEAD + 8 && SLOT_BYTES % 64 == 0, "slot");

#if defined(BL_CPU_EMU)
template <typename T>
struct PerLane {
    T v[64];
    T& operator[](int l) { return v[l]; }
    const T& operator[](int l) const { return v[l]; }
};
struct Stats {  // what the emulation reports beside the bytes (tests/deflate_cases.py counts the same)
    uint32_t forms[3] = {0, 0, 0}, limited = 0, max_len = 0, min_len = 0, max_dist = 0, min_dist = 0;
};
#define BLD_STAT(x) \
    do {            \
        if (st) {   \
            x;      \
        }           \
    } while (0)
#else
template <typename T>
struct PerLane {
    T v;
    __device__ __forceinline__ T& operator[](int) { return v; }
    __device__ __forceinline__ const T& operator[](int) const { return v; }
};
struct Stats;
#define BLD_STAT(x) ((void)0)
#endif

// ---- what the lanes exchange
#if defined(BL_CPU_EMU)
inline uint64_t ballot(const PerLane<uint32_t>& x)
{
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)(x[l] != 0) << l;
    return m;
}
inline uint32_t excl_sum(const PerLane<uint32_t>& x, PerLane<uint32_t>& ex)
{
    uint32_t s = 0;
    for (int l = 0; l < 64; ++l) {
        ex[l] = s;
        s += x[l];
    }
    return s;
}
inline uint32_t xor_all(const PerLane<uint32_t>& x)
{
    uint32_t s = 0;
    for (int l = 0; l < 64; ++l) s ^= x[l];
    return s;
}
inline uint32_t read_lane(const PerLane<uint32_t>& x, uint32_t lane) { return x[(int)lane]; }
inline void lds_add(uint32_t* p, uint32_t v) { *p += v; }
inline void lds_or(uint32_t* p, uint32_t v) { *p |= v; }
#else
__device__ __forceinline__ uint64_t ballot(const PerLane<uint32_t>& x) { return __ballot(x.v != 0); }
__device__ __forceinline__ uint32_t excl_sum(const PerLane<uint32_t>& x, PerLane<uint32_t>& ex)
{
    const int lane = (int)(threadIdx.x & 63u);
    uint32_t incl = x.v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += t;
    }
    ex.v = incl - x.v;
    return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);  // (a scalar: what depends on it stays wave-uniform for the compiler)
}
__device__ __forceinline__ uint32_t xor_all(const PerLane<uint32_t>& x)
{
    uint32_t v = x.v;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d, 64);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint32_t read_lane(const PerLane<uint32_t>& x, uint32_t lane)  // `lane` is wave-uniform
{
    return (uint32_t)__builtin_amdgcn_readlane((int)x.v, __builtin_amdgcn_readfirstlane((int)lane));
}
__device__ __forceinline__ void lds_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void lds_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
#endif
BLD_DEV uint32_t sum_all(const PerLane<uint32_t>& x)
{
    PerLane<uint32_t> ex;
    return excl_sum(x, ex);
}

struct Shared {
    uint16_t t3[1 << T3_BITS];  // position + 1 of the last earlier step's occurrence of a 3-byte hash; 0: none.  After the parse: the staging area
    uint16_t t8[1 << T8_BITS];  // the same for 8 bytes
    uint32_t freq[N_SYMS];      // literal/length counts at 0, distance counts at D_OFF (phase 0: byte counts)
    uint8_t lens[N_SYMS];       // code lengths, same layout
    uint16_t code[N_SYMS];      // codes as they go into the stream (bit-reversed)
    uint16_t sorted[N_D > N_LL ? N_D : N_LL + 2];  // used symbols by (count, symbol)
    uint32_t weight[2 * N_LL];  // tree nodes: leaves in sorted order, then the merges in the order made.  Phase 4: the CRC byte table
    uint16_t parent[2 * N_LL];
    uint16_t depth[2 * N_LL];
    uint32_t blc[16], nxt[16];  // codes per length; next code of a length
    uint32_t uni[4];            // what lane 0 tells the wave
};
constexpr uint32_t STAGE_WORDS = 128;  // 64 pieces of at most 48 bits behind at most 31 pending bits: 98 dwords
static_assert(sizeof(Shared) <= 32768, "five waves per CU");
static_assert(sizeof(uint16_t) * (1 << T3_BITS) >= STAGE_WORDS * 4 && sizeof(uint32_t) * 2 * N_LL >= 1024, "the two reuses");

// ---- symbols (RFC 1951 §3.2.5) by arithmetic
BLD_DEV uint32_t floor_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v > 0
BLD_DEV void length_symbol(uint32_t len, uint32_t& sym, uint32_t& nx, uint32_t& x)
{
    const uint32_t l = len - 3;
    if (l < 8) {
        sym = 257 + l, nx = 0, x = 0;
    } else if (len == 258) {
        sym = 285, nx = 0, x = 0;
    } else {
        const uint32_t e = floor_log2(l) - 2;
        sym = 257 + 4 * e + 4 + ((l >> e) & 3u), nx = e, x = l & ((1u << e) - 1u);
    }
}
BLD_DEV void distance_symbol(uint32_t dist, uint32_t& sym, uint32_t& nx, uint32_t& x)
{
    const uint32_t d = dist - 1;
    if (d < 4) {
        sym = d, nx = 0, x = 0;
    } else {
        const uint32_t e = floor_log2(d) - 1;
        sym = 2 * e + 2 + ((d >> e) & 1u), nx = e, x = d & ((1u << e) - 1u);
    }
}
BLD_DEV uint32_t ll_extra_bits(uint32_t sym) { return sym < 265 || sym == 285 ? 0u : (sym - 261) >> 2; }
BLD_DEV uint32_t d_extra_bits(uint32_t sym) { return sym < 4 ? 0u : (sym >> 1) - 1u; }
BLD_DEV uint32_t fixed_ll_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }
BLD_DEV uint32_t fixed_ll_code(uint32_t s) { return s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xc0 + (s - 280); }
BLD_DEV uint32_t reverse_bits(uint32_t v, uint32_t n)  // 1 <= n <= 16
{
    v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
    v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
    v = ((v >> 4) & 0x0f0fu) | ((v & 0x0f0fu) << 4);
    v = ((v >> 8) & 0x00ffu) | ((v & 0x00ffu) << 8);
    return v >> (16 - n);
}

// ---- text access
BLD_DEV uint64_t load8_inside(const uint8_t* p)  // all 8 bytes are inside the text
{
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}
BLD_DEV uint64_t load8(const uint8_t* text, uint32_t p, uint32_t n)  // text[p, p + 8), zeros at and behind n
{
    if (p + 8 <= n) return load8_inside(text + p);
    uint64_t w = 0;
    for (uint32_t i = 0; i < 8 && p + i < n; ++i) w |= (uint64_t)text[p + i] << (8 * i);
    return w;
}
// how many bytes text[c ..] and text[p ..] share, at most max_len; c < p and p + max_len <= n.  At most max_len / 8 + 7 steps.
BLD_DEV uint32_t match_length(const uint8_t* text, uint32_t c, uint32_t p, uint32_t max_len)
{
    uint32_t k = 0;
    while (k + 8 <= max_len) {
        const uint64_t x = load8_inside(text + c + k) ^ load8_inside(text + p + k);
        if (x) return k + ((uint32_t)__builtin_ctzll(x) >> 3);
        k += 8;
    }
    while (k < max_len && text[c + k] == text[p + k]) ++k;
    return k;
}
BLD_DEV uint32_t hash3(uint64_t w) { return (((uint32_t)w & 0xffffffu) * 0x9e3779b1u) >> (32 - T3_BITS); }
BLD_DEV uint32_t hash8(uint64_t w) { return (uint32_t)((w * 0x9e3779b97f4a7c15ull) >> (64 - T8_BITS)); }

// one candidate c of lane position p: better than `best` (len | dist << 9, with its score)?  wc, wp: the 8 bytes at c and at p (load8), so
// that the loads of a position's candidates are in flight together and most candidates are settled without another load
BLD_DEV void consider(const uint8_t* text, uint32_t c, uint64_t wc, uint32_t p, uint64_t wp, uint32_t max_len, uint32_t lit4, uint32_t& best, int32_t& best_score)
{
    const uint32_t dist = p - c;
    if (dist > MAX_DIST) return;
    const uint64_t x = wc ^ wp;
    uint32_t len = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
    if (len > max_len) len = max_len;
    if (len == 8 && max_len > 8) len = 8 + match_length(text, c + 8, p + 8, max_len - 8);
    if (len < 3) return;
    const uint32_t eb = dist <= 4 ? 0u : floor_log2(dist - 1) - 1u;
    const int32_t score = (int32_t)(len * lit4) - (int32_t)(4u * (MATCH_BASE_BITS + eb));
    if (score < 0) return;
    if (best == 0 || score > best_score || (score == best_score && dist < (best >> 9))) {
        best = len | (dist << 9);
        best_score = score;
    }
}

// table[h] = position + 1 for the step's lanes, the highest position of a slot staying: every round the hardware leaves one writer's
// value per slot and the lanes at or below it retire, so a slot's value rises each round: at most 64 rounds (one where the highest lane's
// write lands last, as in the emulation).
BLD_DEV void insert_positions(uint16_t* table, const PerLane<uint32_t>& h, uint32_t b)
{
    PerLane<uint32_t> act;
    BLD_LANES(l) act[l] = h[l] != NO_HASH;
    for (int round = 0; round < 64; ++round) {
        BLD_LANES(l)
        {
            if (act[l]) table[h[l]] = (uint16_t)(b + (uint32_t)l + 1u);
        }
        BLD_SYNC();
        BLD_LANES(l)
        {
            if (act[l]) act[l] = table[h[l]] < b + (uint32_t)l + 1u;
        }
        if (!ballot(act)) break;
    }
}

// ---- phase 2: the lengths of one alphabet's code.  Returns the number of code lengths the header sends (highest coded symbol + 1).
// freq / lens / code point at the alphabet's part of the arrays in `sh`.
BLD_DEV uint32_t build_code(Shared& sh, const uint32_t* freq, uint32_t nsym, uint8_t* lens, uint16_t* code, uint32_t& limited)
{
    // the used symbols ranked by (count, symbol): a lane takes symbols lane, lane + 64, ...; nsym steps for each
    PerLane<uint32_t> cnt;
    BLD_LANES(l)
    {
        uint32_t c = 0;
        for (uint32_t s = (uint32_t)l; s < nsym; s += 64) {
            lens[s] = 0;
            code[s] = 0;
            const uint32_t f = freq[s];
            if (f) {
                ++c;
                const uint32_t key = (f << 9) | s;  // (counts stay below 2^17)
                uint32_t r = 0;
                for (uint32_t t = 0; t < nsym; ++t) {
                    const uint32_t ft = freq[t];
                    r += (ft != 0) & (((ft << 9) | t) < key);
                }
                sh.sorted[r] = (uint16_t)s;
            }
        }
        cnt[l] = c;
    }
    const uint32_t m = sum_all(cnt);
    BLD_SYNC();
    BLD_LANES(l)
    {
        if (l == 0) {
            uint32_t lim = 0;
            if (m < 2) {
                // fewer than two used symbols: two 1-bit codes, the used one and the lowest other symbol (as zlib does), so that
                // the code is complete for every decoder
                const uint32_t s0 = m ? sh.sorted[0] : 0u;
                lens[s0] = 1;
                lens[s0 == 0 ? 1 : 0] = 1;
            } else {
                // two-queue merge: leaves 0 .. m-1 in sorted order, merges m .. 2m-2 in the order made; the lighter goes first, a
                // merge before a leaf of the same weight (of the optimal trees the deeper one).  m - 1 steps.
                for (uint32_t i = 0; i < m; ++i) sh.weight[i] = freq[sh.sorted[i]];
                uint32_t li = 0, ii = m, nn = m;
                for (uint32_t k = 0; k + 1 < m; ++k) {
                    uint32_t pick[2];
                    for (int j = 0; j < 2; ++j) {
                        if (li < m && (ii >= nn || sh.weight[li] < sh.weight[ii])) pick[j] = li++;
                        else pick[j] = ii++;
                    }
                    sh.weight[nn] = sh.weight[pick[0]] + sh.weight[pick[1]];
                    sh.parent[pick[0]] = sh.parent[pick[1]] = (uint16_t)nn;
                    ++nn;
                }
                // depths from the root down (a parent was made after its children: higher index); 2m - 2 steps
                sh.depth[2 * m - 2] = 0;
                for (uint32_t i = 2 * m - 2; i-- > 0;) sh.depth[i] = (uint16_t)(sh.depth[sh.parent[i]] + 1u);
                for (int k = 0; k < 16; ++k) sh.blc[k] = 0;
                for (uint32_t i = 0; i < m; ++i) {
                    const uint32_t d = sh.depth[i];
                    if (d > 15) lim = 1;
                    ++sh.blc[d > 15 ? 15 : d];
                }
                // the limit: while the Kraft sum (in units of 2^-15) exceeds one, take one code off length 15, move the deepest
                // shorter length one down and split it: the sum falls by one unit a step; fewer than m steps
                uint32_t kraft = 0;
                for (uint32_t k = 1; k < 16; ++k) kraft += sh.blc[k] << (15 - k);
                while (kraft > 32768u) {
                    uint32_t bits = 14;  // (a length below 15 is in use: codes of length 15 alone have a Kraft sum of at most 286 units)
                    while (sh.blc[bits] == 0) --bits;
                    --sh.blc[bits];
                    sh.blc[bits + 1] += 2;
                    --sh.blc[15];
                    --kraft;
                }
                // the lengths go back to the symbols in frequency order, the rarest take the longest
                uint32_t at = 0;
                for (uint32_t k = 15; k >= 1; --k)
                    for (uint32_t j = 0; j < sh.blc[k]; ++j) lens[sh.sorted[at++]] = (uint8_t)k;
            }
            // canonical codes (§3.2.2), bit-reversed for the stream; nsym steps
            for (int k = 0; k < 16; ++k) sh.blc[k] = 0;
            uint32_t top = 0;
            for (uint32_t s = 0; s < nsym; ++s)
                if (lens[s]) {
                    ++sh.blc[lens[s]];
                    top = s + 1;
                }
            uint32_t c = 0;
            for (uint32_t k = 1; k < 16; ++k) {
                c = (c + sh.blc[k - 1]) << 1;
                sh.nxt[k] = c;
            }
            for (uint32_t s = 0; s < nsym; ++s)
                if (lens[s]) code[s] = (uint16_t)reverse_bits(sh.nxt[lens[s]]++, lens[s]);
            sh.uni[0] = top;
            sh.uni[1] = lim;
        }
    }
    BLD_SYNC();
    PerLane<uint32_t> t, li;
    BLD_LANES(l)
    {
        t[l] = sh.uni[0];
        li[l] = sh.uni[1];
    }
    limited |= read_lane(li, 0);
    const uint32_t top = read_lane(t, 0);
    BLD_SYNC();
    return top;
}

// ---- phase 5: the bit emitter.  Pieces of at most 48 bits, 64 at a time, in lane order.
struct Emitter {
    uint32_t* stage;  // STAGE_WORDS dwords of LDS, zero where no bit has been put
    uint32_t* out;    // the member's slot (16-byte aligned)
    uint32_t bitpos = 0, flushed = 0;  // bits emitted; dwords stored
};
BLD_DEV void emit(Emitter& e, const PerLane<uint64_t>& bits, const PerLane<uint32_t>& nb)
{
    PerLane<uint32_t> ex;
    const uint32_t total = excl_sum(nb, ex);
    BLD_LANES(l)
    {
        if (nb[l]) {
            const uint32_t off = e.bitpos + ex[l], wi = (off >> 5) - e.flushed, s = off & 31u;
            const uint32_t lo = (uint32_t)bits[l], hi = (uint32_t)(bits[l] >> 32);
            lds_or(&e.stage[wi], lo << s);
            const uint32_t w1 = (s ? lo >> (32 - s) : 0u) | (hi << s), w2 = s ? hi >> (32 - s) : 0u;
            if (w1) lds_or(&e.stage[wi + 1], w1);
            if (w2) lds_or(&e.stage[wi + 2], w2);
        }
    }
    BLD_SYNC();
    e.bitpos += total;
    const uint32_t done = (e.bitpos >> 5) - e.flushed;  // <= 97
    PerLane<uint32_t> carry;
    BLD_LANES(l)
    {
        for (uint32_t i = (uint32_t)l; i < done; i += 64) e.out[e.flushed + i] = e.stage[i];
        carry[l] = e.stage[done];
    }
    BLD_SYNC();
    BLD_LANES(l)
    {
        for (uint32_t i = (uint32_t)l; i <= done; i += 64) e.stage[i] = i == 0 ? carry[l] : 0u;
    }
    BLD_SYNC();
    e.flushed += done;
}
BLD_DEV void emit_finish(Emitter& e)  // the dword that holds the last bits
{
    if (e.bitpos & 31u) {
        BLD_LANES(l)
        {
            if (l == 0) e.out[e.flushed] = e.stage[0];
        }
    }
}

// ---- one member: text[0, n) (1 <= n <= MEMBER_TEXT) -> the whole BGZF member at `slot` (SLOT_BYTES, 16-byte aligned); `tokens`: the
// wave's MAX_TOKENS + 1 dwords of scratch.  Returns the member's size; crc: the text's CRC-32.
BLD_DEV uint32_t deflate_member(Shared& sh, const uint8_t* text, uint32_t n, uint32_t* tokens, uint8_t* slot, uint32_t& crc, Stats* st = nullptr)
{
    // ---- phase 0: the price of a literal
    BLD_LANES(l)
    {
        for (uint32_t i = (uint32_t)l; i < N_SYMS; i += 64) sh.freq[i] = 0;
        for (uint32_t i = (uint32_t)l; i < (1u << T3_BITS); i += 64) sh.t3[i] = 0;
        for (uint32_t i = (uint32_t)l; i < (1u << T8_BITS); i += 64) sh.t8[i] = 0;
    }
    BLD_SYNC();
    BLD_LANES(l)
    {
        for (uint32_t q = 8u * (uint32_t)l; q < n; q += 512) {  // n / 512 steps, 8 bytes a lane
            const uint64_t w = load8(text, q, n);
            const uint32_t k = n - q < 8 ? n - q : 8u;
            for (uint32_t i = 0; i < k; ++i) lds_add(&sh.freq[(uint32_t)(w >> (8 * i)) & 0xffu], 1u);
        }
    }
    BLD_SYNC();
    PerLane<uint32_t> part;
    BLD_LANES(l)
    {
        uint32_t s = 0;
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = sh.freq[l + 64 * k];
            if (c) {  // floor(4 * log2(n / c)), the fraction read off the two bits behind the leading one
                const uint32_t x = (n << 16) / c, e = floor_log2(x);
                s += c * (4u * (e - 16u) + ((x >> (e - 2u)) & 3u));
            }
        }
        part[l] = s;
    }
    uint32_t lit4 = sum_all(part) / n;
    if (lit4 < 4) lit4 = 4;
    BLD_SYNC();
    BLD_LANES(l)
    {
        for (int k = 0; k < 4; ++k) sh.freq[l + 64 * k] = 0;
    }
    BLD_SYNC();

    // ---- phase 1: the parse, n / 64 steps of 64 positions
    uint32_t next = 0, ntok = 0;  // the first position no token covers yet; tokens so far (both wave-uniform)
    PerLane<uint64_t> ahead;       // the 8 bytes at the lane's position of the NEXT step, loaded a step early
    BLD_LANES(l) ahead[l] = (uint32_t)l < n ? load8(text, (uint32_t)l, n) : 0ull;
    for (uint32_t b = 0; b < n; b += 64) {
        const uint32_t end = b + 64 < n ? b + 64 : n;
        PerLane<uint32_t> h3, h8, best, byte;
        BLD_LANES(l)
        {
            const uint32_t p = b + (uint32_t)l;
            const uint64_t w = ahead[l];
            ahead[l] = p + 64 < n ? load8(text, p + 64, n) : 0ull;
            h3[l] = p + 3 <= n ? hash3(w) : NO_HASH;
            h8[l] = p + 8 <= n ? hash8(w) : NO_HASH;
            byte[l] = (uint32_t)w & 0xffu;
            uint32_t bst = 0;
            if (p >= next && p < n && n - p >= 3) {  // (a step that a match covers whole only enters its positions)
                const uint32_t max_len = n - p < MAX_LEN ? n - p : MAX_LEN;
                int32_t score = 0;
                const uint32_t c3 = sh.t3[h3[l]], c8 = h8[l] != NO_HASH ? sh.t8[h8[l]] : 0u;
                const uint64_t w1 = p >= 1 ? load8(text, p - 1, n) : 0ull, w3 = c3 ? load8(text, c3 - 1, n) : 0ull, w8 = c8 ? load8(text, c8 - 1, n) : 0ull;
                if (p >= 1) consider(text, p - 1, w1, p, w, max_len, lit4, bst, score);
                if (c3) consider(text, c3 - 1, w3, p, w, max_len, lit4, bst, score);
                if (c8) consider(text, c8 - 1, w8, p, w, max_len, lit4, bst, score);
            }
            best[l] = bst;
        }
        // greedy selection: literals up to the first position at or behind `next` that has a match, the match, and again; `next` grows
        // every round: at most 64 rounds a step
        const uint64_t have = ballot(best);
        while (next < end) {
            const uint64_t m = have & ~((1ull << (next - b)) - 1ull);
            const uint32_t first = m ? b + (uint32_t)__builtin_ctzll(m) : end;
            BLD_LANES(l)
            {
                const uint32_t p = b + (uint32_t)l;
                if (p >= next && p < first) {
                    tokens[ntok + (p - next)] = byte[l];
                    lds_add(&sh.freq[byte[l]], 1u);
                }
            }
            ntok += first - next;
            next = first;
            if (first < end) {
                const uint32_t bm = read_lane(best, first - b), len = bm & 511u, dist = bm >> 9;
                BLD_LANES(l)
                {
                    if (l == 0) {
                        uint32_t sym, nx, x;
                        tokens[ntok] = TOKEN_MATCH | ((dist - 1u) << 8) | (len - 3u);
                        length_symbol(len, sym, nx, x);
                        lds_add(&sh.freq[sym], 1u);
                        distance_symbol(dist, sym, nx, x);
                        lds_add(&sh.freq[D_OFF + sym], 1u);
                    }
                }
                BLD_STAT(st->max_len = len > st->max_len ? len : st->max_len; st->min_len = st->min_len && st->min_len < len ? st->min_len : len;
                         st->max_dist = dist > st->max_dist ? dist : st->max_dist; st->min_dist = st->min_dist && st->min_dist < dist ? st->min_dist : dist);
                ++ntok;
                next += len;
            }
        }
        insert_positions(sh.t3, h3, b);
        insert_positions(sh.t8, h8, b);
    }
    BLD_LANES(l)
    {
        if (l == 0) sh.freq[256] = 1;  // end of block
    }
    BLD_SYNC();
    BLD_GLOBAL_SYNC();  // (the tokens are read back by other lanes than wrote them)

    // ---- phase 2: the two codes
    uint32_t limited = 0;
    const uint32_t hlit_raw = build_code(sh, sh.freq, N_LL, sh.lens, sh.code, limited);
    const uint32_t hlit = hlit_raw < 257 ? 257u : hlit_raw;
    const uint32_t hdist = build_code(sh, sh.freq + D_OFF, N_D, sh.lens + D_OFF, sh.code + D_OFF, limited);
    BLD_STAT(st->limited += limited);

    // ---- phase 3: the three sizes
    PerLane<uint32_t> dyn, fix;
    BLD_LANES(l)
    {
        uint32_t d = 0, f = 0;
        for (uint32_t s = (uint32_t)l; s < N_LL; s += 64) {
            d += sh.freq[s] * (sh.lens[s] + ll_extra_bits(s));
            f += sh.freq[s] * (fixed_ll_len(s) + ll_extra_bits(s));
        }
        if (l < (int)N_D) {
            d += sh.freq[D_OFF + l] * (sh.lens[D_OFF + l] + d_extra_bits((uint32_t)l));
            f += sh.freq[D_OFF + l] * (5u + d_extra_bits((uint32_t)l));
        }
        dyn[l] = d;
        fix[l] = f;
    }
    const uint32_t dyn_bits = sum_all(dyn) + 3u + 14u + 57u + 4u * (hlit + hdist), fix_bits = sum_all(fix) + 3u;
    const uint32_t stored_bytes = n + 5u, fix_bytes = (fix_bits + 7u) >> 3, dyn_bytes = (dyn_bits + 7u) >> 3;
    uint32_t form = FORM_STORED, data_bytes = stored_bytes;
    if (fix_bytes < data_bytes) form = FORM_FIXED, data_bytes = fix_bytes;
    if (dyn_bytes < data_bytes) form = FORM_DYNAMIC, data_bytes = dyn_bytes;
    const uint32_t member_bytes = 18u + data_bytes + 8u;
    BLD_STAT(++st->forms[form]);
    BLD_SYNC();
    if (form == FORM_FIXED) {
        BLD_LANES(l)
        {
            for (uint32_t s = (uint32_t)l; s < N_LL; s += 64) {
                sh.lens[s] = (uint8_t)fixed_ll_len(s);
                sh.code[s] = (uint16_t)reverse_bits(fixed_ll_code(s), fixed_ll_len(s));
            }
            if (l < (int)N_D) {
                sh.lens[D_OFF + l] = 5;
                sh.code[D_OFF + l] = (uint16_t)reverse_bits((uint32_t)l, 5);
            }
        }
        BLD_SYNC();
    }

    // ---- phase 4: CRC-32 of the text
    uint32_t* crc_table = sh.weight;
    BLD_LANES(l) blcrcw::fill_table(crc_table, (uint32_t)l);
    BLD_SYNC();
    PerLane<uint32_t> share;
    BLD_LANES(l) share[l] = blcrcw::lane_share(crc_table, text, n, (uint32_t)l);
    crc = xor_all(share);

    // ---- phase 5: emission
    Emitter e;
    e.stage = reinterpret_cast<uint32_t*>(sh.t3);
    e.out = reinterpret_cast<uint32_t*>(slot);
    BLD_LANES(l)
    {
        for (uint32_t i = (uint32_t)l; i < STAGE_WORDS; i += 64) e.stage[i] = 0;
    }
    BLD_SYNC();
    PerLane<uint64_t> bits;
    PerLane<uint32_t> nb;
    // the BGZF header (SAM §4.1): 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00, BSIZE - 1; then the block's first bits
    BLD_LANES(l)
    {
        uint64_t v = 0;
        uint32_t k = 0;
        switch (l) {
        case 0: v = 0x04088b1full, k = 32; break;
        case 1: v = 0, k = 32; break;
        case 2: v = 0x0006ff00ull, k = 32; break;
        case 3: v = 0x00024342ull, k = 32; break;
        case 4: v = member_bytes - 1u, k = 16; break;
        case 5:
            if (form == FORM_STORED) v = 1, k = 8;  // BFINAL, BTYPE 00, up to the byte boundary
            else if (form == FORM_FIXED) v = 1u | (1u << 1), k = 3;
            else v = 1u | (2u << 1) | ((hlit - 257u) << 3) | ((hdist - 1u) << 8) | (15u << 13), k = 17;  // HLIT, HDIST, HCLEN = 19
            break;
        case 6:
            if (form == FORM_STORED) v = n | ((n ^ 0xffffu) << 16), k = 32;  // LEN, NLEN
            break;
        default: break;
        }
        // the code-length code, in the order of §3.2.7 (16 17 18 0 8 ...): 16..18 have no code, 0..15 four bits each
        if (form == FORM_DYNAMIC && l >= 6 && l < 25) v = l < 9 ? 0u : 4u, k = 3;
        bits[l] = v;
        nb[l] = k;
    }
    emit(e, bits, nb);
    if (form == FORM_STORED) {
        for (uint32_t q0 = 0; q0 < n; q0 += 256) {  // n / 256 steps
            BLD_LANES(l)
            {
                const uint32_t q = q0 + 4u * (uint32_t)l;
                uint32_t v = 0, k = 0;
                for (; k < 4 && q + k < n; ++k) v |= (uint32_t)text[q + k] << (8 * k);
                bits[l] = v;
                nb[l] = 8 * k;
            }
            emit(e, bits, nb);
        }
    } else {
        if (form == FORM_DYNAMIC) {
            for (uint32_t i0 = 0; i0 < hlit + hdist; i0 += 64) {  // the code lengths one by one: at most 5 steps
                BLD_LANES(l)
                {
                    const uint32_t i = i0 + (uint32_t)l;
                    const bool live = i < hlit + hdist;
                    const uint32_t len = live ? (i < hlit ? sh.lens[i] : sh.lens[D_OFF + (i - hlit)]) : 0u;
                    bits[l] = reverse_bits(len, 4);  // symbol `len` of the code-length code is the 4-bit code `len`
                    nb[l] = live ? 4u : 0u;
                }
                emit(e, bits, nb);
            }
        }
        PerLane<uint32_t> tok_ahead;  // the next step's tokens, loaded a step early
        BLD_LANES(l) tok_ahead[l] = (uint32_t)l < ntok ? tokens[l] : 0u;
        for (uint32_t i0 = 0; i0 <= ntok; i0 += 64) {  // the tokens and the end of block: ntok / 64 + 1 steps
            BLD_LANES(l)
            {
                const uint32_t i = i0 + (uint32_t)l;
                uint64_t v = 0;
                uint32_t k = 0;
                const uint32_t t = tok_ahead[l];
                tok_ahead[l] = i + 64 < ntok ? tokens[i + 64] : 0u;
                if (i < ntok) {
                    if (t & TOKEN_MATCH) {
                        uint32_t sym, nx, x;
                        length_symbol((t & 0xffu) + 3u, sym, nx, x);
                        v = sh.code[sym];
                        k = sh.lens[sym];
                        v |= (uint64_t)x << k;
                        k += nx;
                        distance_symbol(((t >> 8) & 0x7fffu) + 1u, sym, nx, x);
                        v |= (uint64_t)sh.code[D_OFF + sym] << k;
                        k += sh.lens[D_OFF + sym];
                        v |= (uint64_t)x << k;
                        k += nx;
                    } else {
                        v = sh.code[t];
                        k = sh.lens[t];
                    }
                } else if (i == ntok) {
                    v = sh.code[256];
                    k = sh.lens[256];
                }
                bits[l] = v;
                nb[l] = k;
            }
            emit(e, bits, nb);
        }
    }
    e.bitpos = (e.bitpos + 7u) & ~7u;  // the bits up to the byte boundary are zero already
    BLD_LANES(l)
    {
        bits[l] = l == 0 ? crc : n;
        nb[l] = l < 2 ? 32u : 0u;
    }
    emit(e, bits, nb);
    emit_finish(e);
    return e.bitpos == 8u * member_bytes ? member_bytes : 0u;  // (0: the size computed beforehand was not met — never)
}

// ---- the gather: thread t of `threads` copies its share of a member from its slot (16-byte aligned) to out + off: whole dwords of the
// destination, each put together from the two source dwords it covers, and the bytes in front of and behind them one by one.  Reads at
// most 7 bytes behind the member inside its slot.
BLD_DEV void gather_member(const uint8_t* slot, uint8_t* dst, uint32_t size, uint32_t t, uint32_t threads)
{
    uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;
    if (head > size) head = size;
    const uint32_t n_words = (size - head) >> 2, tail = head + 4u * n_words;
    for (uint32_t i = t; i < head; i += threads) dst[i] = slot[i];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(slot);
    uint32_t* out = reinterpret_cast<uint32_t*>(dst + head);
    const uint32_t s = 8u * head;  // the source runs `head` bytes ahead of the destination's dwords
    for (uint32_t w = t; w < n_words; w += threads) out[w] = s ? (src[w] >> s) | (src[w + 1] << (32u - s)) : src[w];
    for (uint32_t i = tail + t; i < size; i += threads) dst[i] = slot[i];
}

}  // namespace bl_deflate
