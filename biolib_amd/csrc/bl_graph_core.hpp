// bl_graph_core.hpp — per-thread bodies of the table graph (bl_table_adjacency, bl_table_unitigs): the bidirected de Bruijn graph whose
// nodes are the canonical k-mers of a count table, k odd, and its compaction into unitigs.  The definitions are stated in full in
// include/biolib_amd.h.  Compiled two ways like bl_lookup_core.hpp: by hipcc for gfx950 (bl_graph.hip) and by a host compiler under
// BL_CPU_EMU for tests/emu/emu_graph.cpp, which runs every body lane by lane over arrays of exactly their lengths.
//
// The mask pass, the hot one.  A key x has eight neighbour candidates: its four successors f_c = ((x << 2) | c) mod 4^k on the right side
// and, on the left side, the reverse complements of the four successors of rc(x) (the candidate "base c prepended to x" is rc of the
// successor 3 - c of rc(x)).  So both sides are one routine, side_successors(z, rc(z)), run for z = x and for z = rc(x); the left nibble
// is the second answer with its four bits reversed.  A candidate is a key in exactly one of its two forms (k is odd: no k-mer is its own
// reverse complement; the table holds canonical values only, which bad_key checks before anything else runs):
//   forward   f_0 .. f_3 are four consecutive integers: those that are keys stand next to each other in the sorted table, at the slots
//             from the lower bound of f_0 on.  ONE search, then the four keys from that slot are read and compared.
//   reverse   rc(f_c) = (3 - c) * 4^(k-1) + (rc(z) >> 2): four values that differ in the top base only, one per quarter of the table.
//             One search each, and only where rc(f_c) < f_c — the other candidates cannot be keys in this form.
// The (up to) five searches of a side share nothing, so they run in lockstep as bllk::search_group does: every round issues all its
// loads before the first compare.  lower_bound_group is that function's slot-returning sibling: it answers the first slot whose key is
// >= the query instead of a count, and the slot it finds inside the query's bucket is the lower bound in the whole table (the bucket of
// a prefix holds every key of that prefix: where no key of the bucket reaches the query, the bucket's end is the answer).
// A side of degree 1 also leaves its one neighbour as (slot << 1) | entered side: the link pass needs no second search.
#pragma once
#include "bl_lookup_core.hpp"

namespace blgr {

using bllk::TableView;

constexpr int GTPB = 256;  // threads per workgroup of every kernel of bl_graph.hip; each is one thread per key (or per side, or per state):
                           // no grid is capped — n < 2^31 keys are at most 2^24 workgroups of 2n states
constexpr int NS = 5;      // searches in lockstep per side: the lower bound of the forward block and the four reverse forms
constexpr uint32_t LINK_NONE = 0xFFFFFFFFu;
constexpr uint32_t DONE = 0x80000000u;   // Rec::d: the chain's end has been reached
constexpr uint32_t DIST = 0x7FFFFFFFu;
constexpr uint32_t MAX_K = 63;

struct K128 {
    uint64_t lo, hi;
};

// what pointer doubling keeps per state (key, entered side): 16 bytes, one load
struct alignas(16) Rec {
    uint32_t p;  // not DONE: the state 2^round steps ahead; DONE: the chain's last state
    uint32_t d;  // steps to p (31 bits; meaningless on a cycle, where it wraps), DONE in the top bit
    uint32_t m;  // the smallest slot among the states from this one up to p (p's included once DONE)
    uint32_t pad;
};

// one key's entry of the node pass in front of the numbering
struct Placed {
    uint32_t start;      // slot of the unitig's start key
    uint32_t rank_flip;  // (rank << 1) | flip
    uint32_t length;     // keys in the unitig
};

template <int W>
BL_DEV K128 load_key(const TableView& t, uint32_t slot)
{
    K128 r;
    if (W == 2) {
        const bllk::Key2 k = reinterpret_cast<const bllk::Key2*>(t.keys)[slot];  // one 16-byte load
        r.lo = k.lo;
        r.hi = k.hi;
    } else {
        r.lo = t.keys[slot];
        r.hi = 0;
    }
    return r;
}

BL_DEV bool less(const K128& a, const K128& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
BL_DEV bool same(const K128& a, const K128& b) { return a.lo == b.lo && a.hi == b.hi; }

// the 32 base pairs of a word in reverse order
BL_DEV uint64_t reverse_pairs(uint64_t v)
{
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(v);
}

// reverse complement of a k-mer in 2k bits; W = 1: k <= 31, W = 2: k <= 63
template <int W>
BL_DEV K128 revcomp(const K128& x, uint32_t k)
{
    K128 r;
    if (W == 1) {
        r.lo = ~reverse_pairs(x.lo) >> (64 - 2 * k);  // shift 2 .. 62
        r.hi = 0;
        return r;
    }
    const uint64_t top = ~reverse_pairs(x.lo), bottom = ~reverse_pairs(x.hi);
    const uint32_t sh = 128 - 2 * k;  // 2 .. 126
    if (sh >= 64) {
        r.lo = top >> (sh - 64);
        r.hi = 0;
    } else {
        r.lo = (bottom >> sh) | (top << (64 - sh));
        r.hi = top >> sh;
    }
    return r;
}

// 4^k - 1
template <int W>
BL_DEV K128 low_bits(uint32_t k)
{
    K128 m;
    if (W == 1 || 2 * k < 64) {
        m.lo = (1ull << (2 * k)) - 1;
        m.hi = 0;
    } else {
        m.lo = ~0ull;
        m.hi = (1ull << (2 * k - 64)) - 1;
    }
    return m;
}

// (z << 2) mod 4^k
template <int W>
BL_DEV K128 shift_in(const K128& z, uint32_t k)
{
    const K128 m = low_bits<W>(k);
    K128 r;
    r.lo = (z.lo << 2) & m.lo;
    r.hi = W == 1 ? 0 : ((z.hi << 2) | (z.lo >> 62)) & m.hi;
    return r;
}

BL_DEV K128 shift_out(const K128& z)
{
    K128 r;
    r.lo = (z.lo >> 2) | (z.hi << 62);
    r.hi = z.hi >> 2;
    return r;
}

// c * 4^(k-1)
template <int W>
BL_DEV K128 top_base(uint32_t c, uint32_t k)
{
    const uint32_t p = 2 * k - 2;  // 0 .. 124
    K128 r;
    if (W == 1 || p < 64) {
        r.lo = (uint64_t)c << p;  // (p <= 62: the two bits fit)
        r.hi = 0;
    } else {
        r.lo = 0;
        r.hi = (uint64_t)c << (p - 64);
    }
    return r;
}

// the key of slot i breaks the table's promise: a bit at or above 2k, or a value above its own reverse complement
template <int W>
BL_DEV bool bad_key(const TableView& t, uint32_t k, uint32_t i)
{
    const K128 x = load_key<W>(t, i);
    const K128 m = low_bits<W>(k);
    if ((x.lo & ~m.lo) != 0 || (x.hi & ~m.hi) != 0) return true;
    return less(revcomp<W>(x, k), x);
}

// NS searches in lockstep: b[g] = the first slot whose key is >= q[g] (t.n: none), for the live ones; queries are below 2^key_bits
template <int W>
BL_DEV void lower_bound_group(const TableView& t, const K128* q, uint32_t live, uint32_t* b)
{
    uint32_t e[NS];
    BL_UNROLL
    for (int g = 0; g < NS; ++g) {
        b[g] = e[g] = 0;
        if ((live >> g) & 1u) {
            const uint32_t j = bllk::prefix_of(q[g].lo, q[g].hi, t.key_bits, t.prefix_bits);
            b[g] = t.index[j];
            e[g] = t.index[j + 1];
        }
    }
    for (;;) {
        bool more = false;
        uint32_t mid[NS];
        K128 mk[NS];
        BL_UNROLL
        for (int g = 0; g < NS; ++g) {  // the round's loads, all issued before the first compare
            mid[g] = b[g] + ((e[g] - b[g]) >> 1);
            mk[g].lo = mk[g].hi = 0;
            if (b[g] < e[g]) mk[g] = load_key<W>(t, mid[g]);
        }
        BL_UNROLL
        for (int g = 0; g < NS; ++g) {
            if (b[g] < e[g]) {
                if (less(mk[g], q[g])) b[g] = mid[g] + 1;
                else e[g] = mid[g];
                more = more || b[g] < e[g];
            }
        }
        if (!more) break;
    }
}

// The four successors of z (rz = rc(z)): bit c of the answer is set iff canon(((z << 2) | c) mod 4^k) is a key.  nbr: (slot << 1) | side
// of the last neighbour found — the side it is entered by is LEFT (0) where the key is the successor itself, RIGHT (1) where it is the
// successor's reverse complement — which is THE neighbour where the answer has one bit.
template <int W>
BL_DEV uint32_t side_successors(const TableView& t, const K128& z, const K128& rz, uint32_t k, uint32_t& nbr)
{
    const K128 base = shift_in<W>(z, k);
    const K128 tail = shift_out(rz);
    K128 q[NS];
    uint32_t b[NS];
    uint32_t live = 1u;
    q[0] = base;
    BL_UNROLL
    for (uint32_t c = 0; c < 4; ++c) {
        const K128 top = top_base<W>(3 - c, k);
        K128 r, f;
        r.lo = top.lo | tail.lo;
        r.hi = top.hi | tail.hi;
        f.lo = base.lo | c;
        f.hi = base.hi;
        q[1 + c].lo = q[1 + c].hi = 0;
        if (less(r, f)) {
            q[1 + c] = r;
            live |= 2u << c;
        }
    }
    lower_bound_group<W>(t, q, live, b);
    // the forward block's four slots and the reverse forms' one each: eight loads at most, issued together
    K128 fk[4], rk[4];
    uint32_t have = 0;
    BL_UNROLL
    for (uint32_t j = 0; j < 4; ++j) {
        fk[j].lo = fk[j].hi = rk[j].lo = rk[j].hi = 0;
        if (b[0] + j < t.n) {  // (b[0] <= n < 2^31: no wrap)
            fk[j] = load_key<W>(t, b[0] + j);
            have |= 1u << j;
        }
        if (((live >> (1 + j)) & 1u) && b[1 + j] < t.n) {
            rk[j] = load_key<W>(t, b[1 + j]);
            have |= 16u << j;
        }
    }
    uint32_t present = 0;
    nbr = LINK_NONE;
    BL_UNROLL
    for (uint32_t j = 0; j < 4; ++j) {
        if (((have >> j) & 1u) && fk[j].hi == base.hi && (fk[j].lo ^ base.lo) < 4) {  // a key of the block base .. base + 3
            present |= 1u << (uint32_t)(fk[j].lo & 3u);
            nbr = (b[0] + j) << 1;
        }
        if (((have >> (4 + j)) & 1u) && same(rk[j], q[1 + j])) {
            present |= 1u << j;
            nbr = (b[1 + j] << 1) | 1u;
        }
    }
    return present;
}

BL_DEV uint32_t reverse_nibble(uint32_t v) { return ((v & 1u) << 3) | ((v & 2u) << 1) | ((v & 4u) >> 1) | ((v & 8u) >> 3); }

// One key: its mask byte; nbr_left / nbr_right: the one neighbour of a side of degree 1, LINK_NONE for any other degree.
template <int W>
BL_DEV uint32_t mask_thread(const TableView& t, uint32_t k, uint32_t i, uint32_t& nbr_left, uint32_t& nbr_right)
{
    K128 z = load_key<W>(t, i);
    K128 rz = revcomp<W>(z, k);
    uint32_t mask = 0;
    nbr_left = nbr_right = LINK_NONE;
    BL_ROLLED
    for (int side = 1; side >= 0; --side) {  // right: the successors of x; left: those of rc(x), base 3 - c standing for "c prepended"
        uint32_t nbr;
        const uint32_t s = side_successors<W>(t, z, rz, k, nbr);
        if (__builtin_popcount(s) != 1) nbr = LINK_NONE;
        if (side) {
            mask |= s;
            nbr_right = nbr;
        } else {
            mask |= reverse_nibble(s) << 4;
            nbr_left = nbr;
        }
        const K128 swap = z;
        z = rz;
        rz = swap;
    }
    return mask;
}

BL_DEV uint32_t side_nibble(uint32_t mask, uint32_t side) { return side ? mask & 15u : mask >> 4; }

// link[s] of side s = 2i + side: the side's one neighbour where that is another key whose entered side has degree 1 too
BL_DEV uint32_t link_thread(const uint8_t* mask, const uint32_t* nbr, uint32_t s)
{
    const uint32_t x = nbr[s];
    if (x == LINK_NONE || (x >> 1) == (s >> 1)) return LINK_NONE;
    return __builtin_popcount(side_nibble(mask[x >> 1], x & 1u)) == 1 ? x : LINK_NONE;
}

struct KeyStats {
    uint32_t arcs, isolated, dead_end_sides, branch_sides, linked_sides;
};

BL_DEV KeyStats key_stats(const uint8_t* mask, const uint32_t* links, uint32_t i)
{
    const uint32_t m = mask[i];
    const uint32_t dl = (uint32_t)__builtin_popcount(m >> 4), dr = (uint32_t)__builtin_popcount(m & 15u);
    KeyStats st;
    st.arcs = dl + dr;
    st.isolated = m == 0;
    st.dead_end_sides = (dl == 0) + (dr == 0);
    st.branch_sides = (dl >= 2) + (dr >= 2);
    st.linked_sides = (links[2 * i] != LINK_NONE) + (links[2 * i + 1] != LINK_NONE);
    return st;
}

// ---- labelling.  State s = 2 * key + the side the walk entered the key by; it leaves by the other side: next(s) = link of that side,
// which is the state (neighbour, side entered) as it stands.
BL_DEV Rec label_init(const uint32_t* links, uint32_t s)
{
    const uint32_t next = links[s ^ 1u];
    Rec r;
    r.p = next == LINK_NONE ? s : next;
    r.d = next == LINK_NONE ? DONE : 1u;
    r.m = s >> 1;
    r.pad = 0;
    return r;
}

// one round of doubling for state s; live: the state had not reached its chain's end before the round
BL_DEV Rec label_step(const Rec* in, uint32_t s, bool& live)
{
    Rec r = in[s];
    live = (r.d & DONE) == 0;
    if (live) {
        const Rec q = in[r.p];
        r.p = q.p;
        r.d = ((r.d + (q.d & DIST)) & DIST) | (q.d & DONE);
        r.m = q.m < r.m ? q.m : r.m;
    }
    return r;
}

// rounds after which every chain of 2n states has ended and every state on a cycle has seen its whole cycle: ceil(log2(2n)) + 1
BL_DEV uint32_t max_rounds(uint32_t n)
{
    uint32_t r = 1;
    while (r < 32 && (1ull << r) < 2ull * n) ++r;
    return r + 1;
}

// After max_rounds rounds: key i is the smallest slot of a cycle (its state "entered by the left" never ended and saw nothing smaller).
// Then the link of its left side is cut, at both ends; returns whether.  One thread per cycle writes, and only that cycle's two words.
BL_DEV bool cut_cycle_thread(const Rec* rec, uint32_t* links, uint32_t i)
{
    const Rec r = rec[2 * i];
    if ((r.d & DONE) || r.m != i) return false;
    const uint32_t other = links[2 * i];
    links[other] = LINK_NONE;  // ((j << 1) | t is the word of side t of key j)
    links[2 * i] = LINK_NONE;
    return true;
}

// The two directions of key i's path end at key a (walking on from "entered by the left") and at key b; the unitig starts at the smaller
// and the key's rank is its distance from there.  Entered by the left in the chosen direction: read as stored.
BL_DEV Placed place_thread(const Rec* rec, uint32_t i)
{
    const Rec fwd = rec[2 * i], back = rec[2 * i + 1];
    const uint32_t a = fwd.p >> 1, b = back.p >> 1;
    const uint32_t da = fwd.d & DIST, db = back.d & DIST;
    Placed pl;
    pl.length = da + db + 1;
    if (b <= a) {  // (a == b: a path of one key)
        pl.start = b;
        pl.rank_flip = db << 1;
    } else {
        pl.start = a;
        pl.rank_flip = (da << 1) | 1u;
    }
    return pl;
}

// ---- emission
// the bytes key i stores into the unitig's string at `at` = offsets[unitig]: its last oriented base, and as the start key the k - 1 in front
template <int W>
BL_DEV void emit_thread(const TableView& t, uint32_t k, uint32_t i, uint32_t rank_flip, uint64_t at, uint8_t* out)
{
    K128 o = load_key<W>(t, i);
    if (rank_flip & 1u) o = revcomp<W>(o, k);
    const uint32_t rank = rank_flip >> 1;
    const uint32_t code = 0x54474341u;  // "ACGT", A in the low byte
    out[at + (k - 1) + rank] = (uint8_t)(code >> (8 * (uint32_t)(o.lo & 3u)));
    if (rank == 0) {
        for (uint32_t j = 0; j + 1 < k; ++j) {
            const uint32_t p = 2 * (k - 1 - j);  // 2 .. 124
            const uint32_t c = (uint32_t)((p >= 64 ? o.hi >> (p - 64) : o.lo >> p) & 3u);
            out[at + j] = (uint8_t)(code >> (8 * c));
        }
    }
}

// the result is not a fixed-length batch: unitig u is not `len` long
BL_DEV bool breaks_uniform(const uint64_t* offsets, uint64_t n_unitigs, uint64_t len, uint64_t u)
{
    return u < n_unitigs && offsets[u + 1] - offsets[u] != len;
}

// BL_ERR_INVALID reasons of both calls that need no device: 0 = fine
BL_DEV int refuse(uint32_t k, uint32_t key_words, uint32_t key_bits, uint64_t n)
{
    if (k == 0 || k > MAX_K || (k & 1u) == 0) return 1;
    if (2 * k > key_bits) return 2;
    if (key_words == 1 && k > 31) return 3;
    if (n >= (1ull << 31)) return 4;  // a link word holds a slot and a side
    return 0;
}

}  // namespace blgr
