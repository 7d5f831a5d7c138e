// bl_dedup_core.hpp — per-lane bodies of bl_scan_read_duplicates (exact duplicate reads and pairs; the rule is stated in
// include/biolib_amd.h).  Compiled two ways like bl_adapters_core.hpp: by hipcc for gfx950 (bl_dedup.hip) and by a host compiler under
// BL_CPU_EMU for tests/emu/emu_dedup.cpp, which runs the lanes as loops over arrays of exactly their sizes.
//
// Keys as words.  A read's key is the first n bases of its clamped span.  Word w of it holds the bases [32 w, 32 w + 32) as 64 bits of
// 2-bit codes, first base most significant, and 64 bits of invalid marks (the low bit of a base's pair); codes at an invalid base and
// everything behind the key's end are 0 in both, so that two keys are equal exactly where their lengths and all their words are.  A
// word comes from two chunks of bla::stage_chunk: the batch's packed copy, ASCII only for a chunk with an invalid base or without a
// copy.  Word w of the reverse complement is the reversed, complemented word of the bases [n - 32 w - m, n - 32 w).
//
// The hash of a key is a sum (mod 2^64, two halves with their own seeds) of mixed (word, w) terms and one for the length: sixteen lanes
// take the words of a key in turn and add their parts up in any order.  It only groups the units; the comparison decides.
//
// Safety.  Offsets, input spans and prefix_len are trusted for content only: read boundaries are clamped to [0, n_bases]
// (blsel::read_extent), spans to the read (bla::start_span).  stage_chunk reads ASCII bytes only inside [0, n_bases) and packed words
// only for chunks that hold a base of the batch and the one behind.
#pragma once
#include "bl_adapters_core.hpp"

#ifdef BL_CPU_EMU
#define BLD_RAN(k) (++bld::ran[k])
#define BLD_NOUNROLL
#else
#define BLD_RAN(k) ((void)0)
#define BLD_NOUNROLL _Pragma("nounroll")
#endif

namespace bld {

constexpr int TPB = 256;   // threads of a workgroup
constexpr int SUB = 16;    // lanes that share a unit in the hash and the comparison: four units to a wave
constexpr uint32_t FLAG_PAIRED = 1u, FLAG_CANONICAL = 2u;                       // include/biolib_amd.h: BL_DEDUP_*
enum { DUP_DUPLICATE = 1, DUP_EMPTY = 2, DUP_REVERSED = 4 };                    // BL_DUP_*
enum { U_EMPTY = 1, U_REVERSED = 2 };                                           // a unit's byte of notes: empty; equal to its class's head only reversed
constexpr uint32_t NONE32 = 0xffffffffu;
constexpr uint32_t HASH_BITS = 96;
constexpr int STRIPES = 64, STRIPE_WORDS = 32;
enum { C_EMPTY = 0, C_CLASSES, C_DUP, C_REV, C_READS_KEPT, C_BASES_KEPT, C_MIXED, C_HIST0, C_LARGEST = C_HIST0 + 16 /* a maximum */, N_COUNTERS };
static_assert(N_COUNTERS <= STRIPE_WORDS, "a stripe holds the counters");

#ifdef BL_CPU_EMU
enum { RAN_PACKED = 0, RAN_ASCII, RAN_REVERSED, RAN_HASH, RAN_COMPARE, RAN_HEAD, RAN_SINGLETON, RAN_FINISH, N_RAN };
static unsigned long long ran[N_RAN];
#endif

// include/biolib_amd.h: bl_dedup_rule, bl_read_duplicate
struct Rule {
    uint32_t flags, hash_bits;
    uint64_t prefix_len, seed, reserved;
};
struct alignas(16) Record {
    uint32_t first, kept, copies, flags;
};
// a sort key: the hash's top bits above the unit's index (a little-endian 128-bit number)
struct alignas(16) Key {
    uint64_t lo, hi;
};
struct Hash {
    uint64_t lo, hi;
};
// what a class knows of its members: the best (score, lowest index) and how many
struct alignas(16) Best {
    uint64_t score;
    uint32_t idx, count;
};

// NULL where the rule is valid, else what is wrong with it (the entry point's message)
BL_DEV const char* rule_error(const Rule& r, uint64_t n_seqs)
{
    if (r.flags & ~(FLAG_PAIRED | FLAG_CANONICAL)) return "bl_dedup_rule: unknown flag bits";
    if ((r.flags & FLAG_PAIRED) && (n_seqs & 1)) return "BL_DEDUP_PAIRED needs an even number of sequences: reads 2u and 2u + 1 are mates";
    if (r.hash_bits > HASH_BITS) return "bl_dedup_rule: hash_bits is at most 96";
    if (r.reserved != 0) return "bl_dedup_rule: reserved must be 0";
    if (((r.flags & FLAG_PAIRED) ? n_seqs / 2 : n_seqs) >= (1ull << 32)) return "bl_scan_read_duplicates takes fewer than 2^32 units";
    return nullptr;
}

BL_DEV uint64_t fmix64(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

struct DedupParams {
    bla::AdapterParams src;   // bases, n_bases, offsets, read_len, n_seqs, the packed copy and spans_in: what stage_chunk and start_span take
    const uint64_t* scores;   // [n_seqs] or NULL
    uint32_t flags, hash_bits;
    uint64_t prefix_len, seed_lo, seed_hi;
    uint64_t n_units;
    uint32_t round;           // the resolution round, from 1
    // work arrays
    Key* keys;                // [n_units]: written by the hash pass, then sorted
    uint8_t* notes;           // [n_units]: U_*
    uint32_t* rep;            // [n_units] by sorted place: the place of the class's head, NONE32 while unresolved
    uint64_t* scan;           // [n_units] by sorted place: group start << 32 | (the place where unresolved, else NONE32); scanned: the head
    const uint64_t* order;    // [n_units]: the places sorted by (rep, place), or NULL where the classes lie together already
    Best* members;            // [n_units] in that order
    uint32_t* member_class;   // [n_units] in that order: rep
    const Best* classes;      // [n_units] by the head's place
    uint32_t* flag_words;     // [0]: a member is left unresolved; [1]: a unit is empty; ([2]: the host's, the reduction's number of classes)
    // outputs, each nullable
    Record* out_records;            // [n_units]
    uint64_t* out_spans;            // [n_seqs][2]
    unsigned long long* counters;   // [STRIPES][STRIPE_WORDS]
};

// ---- where a unit's keys lie
struct UnitSpan {
    uint64_t start[2], n[2];  // the key of read t: n bases from base `start` of the batch
    uint64_t b[2], e[2];      // the clamped span, (0, 0) where empty
    int reads;
    bool empty;
};
BL_DEV UnitSpan unit_span(const DedupParams& p, uint64_t u)
{
    UnitSpan s;
    s.reads = (p.flags & FLAG_PAIRED) ? 2 : 1;
    s.empty = false;
    s.start[1] = s.n[1] = s.b[1] = s.e[1] = 0;
    BL_UNROLL
    for (int t = 0; t < 2; ++t) {  // (constant indices: the arrays stay in registers)
        if (t >= s.reads) break;
        const uint64_t i = (uint64_t)s.reads * u + (uint64_t)t;
        uint64_t first, L;
        blsel::read_extent(p.src.offsets, p.src.read_len, p.src.n_bases, i, first, L);
        bla::start_span(p.src, i, L, s.b[t], s.e[t]);
        uint64_t n = s.e[t] - s.b[t];
        if (p.prefix_len && n > p.prefix_len) n = p.prefix_len;
        s.n[t] = n;
        s.start[t] = first + s.b[t];
        if (n == 0) s.empty = true;
    }
    return s;
}

// ---- words.  The m (1 .. 32) bases from base `start` of the batch on, start + m <= n_bases: codes and invalid marks, zeros behind base m.
BL_DEV void key_word(const bla::AdapterParams& src, uint64_t start, int m, uint64_t& c, uint64_t& v)
{
    uint32_t c0, v0, c1, v1;
    const int how0 = bla::stage_chunk(src, start, (uint64_t)m, 0, c0, v0);
    const int how1 = bla::stage_chunk(src, start, (uint64_t)m, 1, c1, v1);
    if (how0 == 1 || how1 == 1) BLD_RAN(RAN_PACKED);
    if (how0 == 2 || how1 == 2) BLD_RAN(RAN_ASCII);
    const uint64_t mask = bla::length_mask(m);
    v = (((uint64_t)v0 << 32) | v1) & mask;
    c = (((uint64_t)c0 << 32) | c1) & mask & ~(v | (v << 1));
}
// the word of m bases reversed and complemented in place, rc(N) = N
BL_DEV void reverse_word(uint64_t& c, uint64_t& v, int m)
{
    BLD_RAN(RAN_REVERSED);
    uint64_t r = __builtin_bitreverse64(~c);
    r = ((r >> 1) & bla::M5) | ((r & bla::M5) << 1);  // base j at place 31 - j, its two bits in order again
    uint64_t rv = __builtin_bitreverse64(v) >> 1;
    const int sh = 2 * (32 - m);  // (m >= 1: at most 62)
    r <<= sh;
    rv <<= sh;
    v = rv;
    c = r & ~(rv | (rv << 1));
}
// word w of the key of n bases at `start`, forward or of its reverse complement (32 w < n)
BL_DEV void oriented_word(const bla::AdapterParams& src, uint64_t start, uint64_t n, uint64_t w, bool reversed, uint64_t& c, uint64_t& v)
{
    const uint64_t left = n - 32 * w;
    const int m = left < 32 ? (int)left : 32;
    if (!reversed) {
        key_word(src, start + 32 * w, m, c, v);
    } else {
        key_word(src, start + left - (uint64_t)m, m, c, v);
        reverse_word(c, v, m);
    }
}

// ---- the hash.  Lane `sub` of SUB: its part of the key's sum.
BL_DEV Hash hash_part(const DedupParams& p, uint64_t start, uint64_t n, bool reversed, int sub)
{
    Hash h;
    h.lo = h.hi = 0;
    const uint64_t words = (n + 31) / 32;
    for (uint64_t w = (uint64_t)sub; w < words; w += SUB) {
        uint64_t c, v;
        oriented_word(p.src, start, n, w, reversed, c, v);
        BLD_RAN(RAN_HASH);
        uint64_t a = fmix64(c ^ (p.seed_lo + w * 0x9e3779b97f4a7c15ull));
        uint64_t b = fmix64(c ^ (p.seed_hi + w * 0xd6e8feb86659fd93ull));
        if (v) {  // rare: a word with an invalid base
            a = fmix64(a ^ v);
            b = fmix64(b + v);
        }
        h.lo += a;
        h.hi += b;
    }
    return h;
}
BL_DEV Hash hash_add(Hash a, Hash b)
{
    a.lo += b.lo;
    a.hi += b.hi;
    return a;
}
// the key's hash from the sum of its parts: the length's term
BL_DEV Hash hash_length(const DedupParams& p, Hash sum, uint64_t n)
{
    sum.lo += fmix64(n ^ p.seed_hi ^ 0xa0761d6478bd642full);
    sum.hi += fmix64(n + p.seed_lo + 0xe7037ed1a0b428dbull);
    return sum;
}
BL_DEV bool hash_less(Hash a, Hash b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
BL_DEV Hash hash_min(Hash a, Hash b) { return hash_less(b, a) ? b : a; }
// the ordered pair (a, b)
BL_DEV Hash hash_pair(Hash a, Hash b)
{
    Hash h;
    h.lo = fmix64(a.lo + 0x8ebc6af09c88c6e3ull) ^ fmix64(b.lo + 0x589965cc75374cc3ull);
    h.hi = fmix64(a.hi + 0x1d8e4e27c47d124full) ^ fmix64(b.hi + 0xeb44accab455d165ull);
    return h;
}
// The unit's hash from its keys' hashes: fwd[t] of read t, rev[0] of the single read's reverse complement (canonical only).
BL_DEV Hash unit_hash(const DedupParams& p, const Hash fwd[2], Hash rev0)
{
    const bool canonical = (p.flags & FLAG_CANONICAL) != 0;
    if (p.flags & FLAG_PAIRED) {
        const Hash h = hash_pair(fwd[0], fwd[1]);
        return canonical ? hash_min(h, hash_pair(fwd[1], fwd[0])) : h;
    }
    return canonical ? hash_min(fwd[0], rev0) : fwd[0];
}
// the sort key of unit u: the top hash_bits of the 96 bits (hi, top half of lo) above the index; an empty unit's hash is 0
BL_DEV Key make_key(Hash h, uint32_t hash_bits, uint64_t u, bool empty)
{
    __uint128_t x = ((__uint128_t)h.hi << 32) | (h.lo >> 32);
    x = empty ? 0 : x >> (HASH_BITS - hash_bits);  // (hash_bits >= 1)
    x = (x << 32) | (uint32_t)u;
    Key k;
    k.lo = (uint64_t)x;
    k.hi = (uint64_t)(x >> 64);
    return k;
}
BL_DEV uint32_t key_unit(const Key& k) { return (uint32_t)k.lo; }
BL_DEV bool same_group(const Key& a, const Key& b) { return a.hi == b.hi && (a.lo >> 32) == (b.lo >> 32); }

// ---- resolution.  Place j of the sorted keys, one thread: the scan's input word; in round 1 also rep[j] (a singleton group and an empty
// unit are resolved at once and never read again).
BL_DEV void mark_place(const DedupParams& p, uint64_t j)
{
    const Key k = p.keys[j];
    const bool starts = j == 0 || !same_group(p.keys[j - 1], k);
    if (p.round == 1) {
        const bool ends = j + 1 == p.n_units || !same_group(p.keys[j + 1], k);
        const bool done = (starts && ends) || (p.notes[key_unit(k)] & U_EMPTY);
        if (done) BLD_RAN(RAN_SINGLETON);
        p.rep[j] = done ? (uint32_t)j : NONE32;
    }
    const uint32_t open = p.rep[j] == NONE32 ? (uint32_t)j : NONE32;
    p.scan[j] = ((uint64_t)(starts ? 1 : 0) << 32) | open;
}
// the segmented minimum: the first unresolved place of a group at or before each place
BL_DEV uint64_t scan_join(uint64_t a, uint64_t b)
{
    if (b >> 32) return b;
    const uint32_t x = (uint32_t)a, y = (uint32_t)b;
    return (a & ~0xffffffffull) | (x < y ? x : y);
}

// Lane `sub` of SUB: do its words of key a (n bases at start_a) equal those of key b, forward or b reversed?  (The lengths are equal.)
BL_DEV bool compare_part(const DedupParams& p, uint64_t start_a, uint64_t start_b, uint64_t n, bool reversed, int sub)
{
    bool same = true;
    const uint64_t words = (n + 31) / 32;
    for (uint64_t w = (uint64_t)sub; w < words && same; w += SUB) {
        uint64_t ca, va, cb, vb;
        oriented_word(p.src, start_a, n, w, false, ca, va);
        oriented_word(p.src, start_b, n, w, reversed, cb, vb);
        BLD_RAN(RAN_COMPARE);
        same = ca == cb && va == vb;
    }
    return same;
}
// A lane's part of unit a against the head h: bit 0 = the forward keys agree in this lane's words, bit 1 = they agree the other way
// round (the reverse complement of a read, the swapped mates of a pair; canonical only).  All SUB lanes' answers ANDed decide.
BL_DEV uint32_t compare_unit(const DedupParams& p, const UnitSpan& a, const UnitSpan& h, int sub)
{
    const bool paired = a.reads == 2;
    uint32_t ok = (p.flags & FLAG_CANONICAL) ? 3u : 1u;
    // q = 0 .. 3.  A read: its key against the head's (0) and against the head's reversed (2).  A pair: (s1, h1), (s2, h2) for bit 0,
    // (s1, h2), (s2, h1) for bit 1.  One body for all of them keeps the kernel small.
    BLD_NOUNROLL
    for (int q = 0; q < 4; ++q) {
        const bool second = (q & 1) != 0, other = (q >> 1) != 0;
        const uint32_t bit = other ? 2u : 1u;
        if ((second && !paired) || !(ok & bit)) continue;
        const bool head_second = paired && second != other;
        const uint64_t start_a = second ? a.start[1] : a.start[0], n_a = second ? a.n[1] : a.n[0];
        const uint64_t start_h = head_second ? h.start[1] : h.start[0], n_h = head_second ? h.n[1] : h.n[0];
        if (n_a != n_h || !compare_part(p, start_a, start_h, n_a, !paired && other, sub)) ok &= ~bit;
    }
    return ok;
}
// The head place j is compared with in this round, j itself where it is the head, NONE32 where j is resolved already.
BL_DEV uint32_t place_head(const DedupParams& p, uint64_t j)
{
    if (p.rep[j] != NONE32) return NONE32;
    return (uint32_t)p.scan[j];  // (<= j: j itself is unresolved)
}
// What place j does once its lanes' answers are ANDed into `ok` (unused for a head); one lane calls this.
// True where j is a head of round 2: every group that held more than one class has exactly one.
BL_DEV bool resolve_place(const DedupParams& p, uint64_t j, uint32_t head, uint32_t ok)
{
    if (head == (uint32_t)j) {  // the next class of the group: its head
        BLD_RAN(RAN_HEAD);
        p.rep[j] = head;
        return p.round == 2;
    }
    if (ok & 1u) {
        p.rep[j] = head;
    } else if (ok & 2u) {
        p.rep[j] = head;
        p.notes[key_unit(p.keys[j])] |= U_REVERSED;
    } else {
        p.flag_words[0] = 1u;  // (everyone stores the same word)
    }
    return false;
}

// ---- finish.  Sorting these puts the places of a class together, its head first.
BL_DEV uint64_t order_key(const DedupParams& p, uint64_t j) { return ((uint64_t)p.rep[j] << 32) | j; }
// Place t of the class order: the member's entry for the segmented maximum.
BL_DEV void member_entry(const DedupParams& p, uint64_t t)
{
    const uint64_t j = p.order ? (p.order[t] & 0xffffffffull) : t;
    const uint32_t u = key_unit(p.keys[j]);
    Best b;
    b.idx = u;
    b.count = 1;
    b.score = 0;
    if (p.scores) b.score = (p.flags & FLAG_PAIRED) ? p.scores[2 * (uint64_t)u] + p.scores[2 * (uint64_t)u + 1] : p.scores[u];
    p.members[t] = b;
    p.member_class[t] = p.rep[j];
}
BL_DEV Best best_join(const Best& a, const Best& b)
{
    const bool take_b = b.score > a.score || (b.score == a.score && b.idx < a.idx);
    Best r = take_b ? b : a;
    r.count = a.count + b.count;
    return r;
}

// what a unit adds to the statistics
struct Tally {
    uint32_t empty, head, dup, rev, reads_kept, copies;  // copies: the class size at its first member, else 0
    uint64_t bases_kept;
};
// Place j, one thread: the unit's record and its reads' spans.
BL_DEV Tally finish_place(const DedupParams& p, uint64_t j)
{
    BLD_RAN(RAN_FINISH);
    Tally t;
    t.empty = t.head = t.dup = t.rev = t.reads_kept = t.copies = 0;
    t.bases_kept = 0;
    const uint32_t u = key_unit(p.keys[j]);
    const UnitSpan s = unit_span(p, u);
    Record r;
    bool keep = true;
    if (s.empty) {
        r.first = r.kept = u;
        r.copies = 0;
        r.flags = DUP_EMPTY;
        t.empty = 1;
    } else {
        const uint32_t head = p.rep[j];
        const Best c = p.classes[head];
        r.first = key_unit(p.keys[head]);
        r.kept = c.idx;
        r.copies = c.count;
        r.flags = 0;
        if (u != c.idx) r.flags |= DUP_DUPLICATE;
        if ((p.notes[u] ^ p.notes[c.idx]) & U_REVERSED) r.flags |= DUP_REVERSED;
        keep = u == c.idx;
        t.head = head == (uint32_t)j ? 1 : 0;
        t.copies = t.head ? c.count : 0;
        t.dup = keep ? 0 : 1;
        t.rev = (r.flags & DUP_REVERSED) ? 1 : 0;
    }
    if (p.out_records) p.out_records[u] = r;
    BL_UNROLL
    for (int k = 0; k < 2; ++k) {
        if (k >= s.reads) break;
        const uint64_t i = (uint64_t)s.reads * u + (uint64_t)k;
        const uint64_t b = keep ? s.b[k] : 0, e = keep ? s.e[k] : 0;
        if (p.out_spans) {
            p.out_spans[2 * i] = b;
            p.out_spans[2 * i + 1] = e;
        }
        t.reads_kept += e > b ? 1 : 0;
        t.bases_kept += e - b;
    }
    return t;
}

}  // namespace bld
