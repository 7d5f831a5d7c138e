// bl_clean_core.hpp — per-thread bodies of graph cleaning: bl_unitigs_mark (which unitigs of the compacted graph are tips, islands or bubble
// branches) and bl_table_remove_unitigs (the table without the marked unitigs' keys).  The definitions are stated in full in
// include/biolib_amd.h.  Compiled two ways like bl_links_core.hpp: by hipcc for gfx950 (bl_clean.hip) and by a host compiler under
// BL_CPU_EMU for tests/emu/emu_clean.cpp, which runs every body lane by lane over arrays of exactly their lengths.
//
// mark_thread, one lane per unitig u, is a chain of dependent gathers, every level's independent loads issued before its first compare:
//   0  the unitig's own words: three link offsets, two offsets, the sum (info_of)                — most unitigs leave here: too long
//   1  the records of its live end (a tip candidate: up to four) or of both ends (a bubble candidate: one each)
//   2  the two link offsets of every junction end f ^ 1
//   3  per junction, its (up to four) records x, then the words of every x's unitig w (info_of again), then for a bubble the first
//      record of both ends of w
// The loops over the four records are unrolled: a record array is never indexed by a runtime value.
// The keep order compares S(w) * L(u) with S(u) * L(w) as 128-bit integers (an unsigned __int128: two 64-bit multiplies and a mul_hi
// each on the device), never in floating point.
//
// The compaction is count / exclusive sum / write over tiles of 64 * ROWS keys, one wave per tile: lane l of the wave reads slot
// tile * 64 * ROWS + row * 64 + l in row `row`, so that every load of nodes, keys and counts is one contiguous run per wave; the mark
// byte of the node's unitig is the only gather.  A kept key's place is the tile's base (the exclusive sum of the tile totals) plus the
// kept keys of the rows in front plus the kept lanes below it in its row (a ballot): no atomic places anything.
//
// Safety.  The arrays are trusted for content only (select's policy): a link offset is clamped to n_links, only the first four records of
// an end are read, a `to` at or above 2 * n_unitigs is ignored, a node whose unitig is at or above n_unitigs keeps its key.  Nothing
// outside [0, n_unitigs] of the offsets, [0, n_unitigs) of the sums and marks, [0, 2 n_unitigs] of the link offsets, [0, n_links) of the
// records and [0, n) of the nodes, keys and counts is read or written.
#pragma once
#include "bl_links_core.hpp"

namespace blcl {

constexpr int CTPB = 256;  // threads per workgroup of every kernel of bl_clean.hip; no grid is capped
constexpr int ROWS = 8;    // rows of a compaction tile: 512 keys per wave
constexpr uint32_t TIPS = 1u, ISOLATED = 2u, BUBBLES = 4u, ALL_RULES = 7u;  // include/biolib_amd.h: BL_CLEAN_*
constexpr uint8_t KEEP = 0, TIP = 1, ISLAND = 2, BUBBLE = 3;               // BL_MARK_*
constexpr uint32_t NO_END = 0xFFFFFFFFu;                                   // (at or above 2 * n_unitigs for every n_unitigs < 2^31)

typedef unsigned __int128 u128;

struct Rule {  // bl_clean_rule
    uint32_t flags, k;
    uint64_t max_tip_keys, max_isolated_keys, max_isolated_mean, max_bubble_keys, max_bubble_diff, reserved;
};

struct Graph {
    const uint64_t* offsets;       // n_unitigs + 1
    const uint64_t* sums;          // n_unitigs
    const uint64_t* link_offsets;  // 2 * n_unitigs + 1
    const bllnk::Link* links;      // n_links
    uint64_t n_unitigs, n_links;
};

// BL_ERR_INVALID reasons that need no device: 0 = fine
BL_DEV int refuse(uint32_t flags, uint32_t k, uint64_t reserved, uint64_t n_unitigs)
{
    if (!(k & 1u) || k < bllnk::MIN_K || k > 63) return 1;
    if (flags & ~ALL_RULES) return 2;
    if (reserved) return 3;
    if (n_unitigs >> 31) return 4;
    return 0;
}

// the records of one end: where they begin (below n_links, or n_links with none) and how many the offsets say there are
struct End {
    uint64_t at, deg;
};

BL_DEV End end_between(uint64_t a, uint64_t b, uint64_t n_links)
{
    a = a < n_links ? a : n_links;
    b = b < n_links ? b : n_links;
    End e;
    e.at = a;
    e.deg = b > a ? b - a : 0;
    return e;
}

// the words of one unitig: both ends, L (mod 2^64 on wrong offsets: only compared and multiplied) and S
struct Info {
    End end[2];  // + and -
    uint64_t keys, sum;
};

BL_DEV Info info_of(const Graph& g, uint32_t k, uint64_t u)
{
    const uint64_t a = g.link_offsets[2 * u], b = g.link_offsets[2 * u + 1], c = g.link_offsets[2 * u + 2];
    const uint64_t o0 = g.offsets[u], o1 = g.offsets[u + 1], s = g.sums[u];  // six loads in flight
    Info f;
    f.end[0] = end_between(a, b, g.n_links);
    f.end[1] = end_between(b, c, g.n_links);
    f.keys = o1 - o0 - (k - 1);
    f.sum = s;
    return f;
}

BL_DEV Info no_info()
{
    Info f;
    f.end[0].at = f.end[0].deg = f.end[1].at = f.end[1].deg = 0;
    f.keys = f.sum = 0;
    return f;
}

// the keep order: (S(w) L(u), L(w), -w) > (S(u) L(w), L(u), -u)
BL_DEV bool precedes(const Info& w, uint64_t wn, const Info& u, uint64_t un)
{
    const u128 a = (u128)w.sum * u.keys, b = (u128)u.sum * w.keys;
    if (a != b) return a > b;
    if (w.keys != u.keys) return w.keys > u.keys;
    return wn < un;
}

// the live end of a tip candidate, NO_END for any other unitig
BL_DEV uint32_t tip_live_end(const Info& f, uint64_t u, uint64_t max_tip_keys)
{
    const bool dead0 = f.end[0].deg == 0, dead1 = f.end[1].deg == 0;
    if (dead0 == dead1 || f.keys > max_tip_keys) return NO_END;
    return (uint32_t)(2 * u) | (dead0 ? 1u : 0u);
}

// the first four `to` words of an end, NO_END behind its last
BL_DEV void load_records(const Graph& g, const End& e, uint32_t to[4])
{
    BL_UNROLL
    for (uint32_t j = 0; j < 4; ++j) to[j] = j < e.deg ? g.links[e.at + j].to : NO_END;  // (at + j < n_links: deg is clamped)
}

BL_DEV bool tip_rule(const Graph& g, const Rule& r, uint64_t u, const Info& me, uint32_t e)
{
    const uint64_t n_ends = 2 * g.n_unitigs;
    uint32_t f[4];
    load_records(g, me.end[e & 1u], f);
    End junction[4];  // the records of f ^ 1: the ends that touch the junction e leads into, turned round
    BL_UNROLL
    for (uint32_t j = 0; j < 4; ++j) {
        junction[j].at = junction[j].deg = 0;
        if (f[j] < n_ends) junction[j] = end_between(g.link_offsets[f[j] ^ 1u], g.link_offsets[(f[j] ^ 1u) + 1], g.n_links);
    }
    bool marked = false;
    BL_UNROLL
    for (uint32_t j = 0; j < 4; ++j) {
        if (marked || junction[j].deg == 0) continue;
        uint32_t x[4];
        load_records(g, junction[j], x);
        Info w[4];
        BL_UNROLL
        for (uint32_t i = 0; i < 4; ++i) w[i] = x[i] < n_ends && (x[i] >> 1) != u ? info_of(g, r.k, x[i] >> 1) : no_info();
        BL_UNROLL
        for (uint32_t i = 0; i < 4; ++i) {
            if (x[i] >= n_ends || (x[i] >> 1) == u) continue;
            // a real continuation leaves the junction, or a better spur does
            if (tip_live_end(w[i], x[i] >> 1, r.max_tip_keys) != (x[i] ^ 1u) || precedes(w[i], x[i] >> 1, me, u)) marked = true;
        }
    }
    return marked;
}

BL_DEV bool bubble_rule(const Graph& g, const Rule& r, uint64_t u, const Info& me)
{
    const uint64_t n_ends = 2 * g.n_unitigs;
    const uint32_t f0 = g.links[me.end[0].at].to, f1 = g.links[me.end[1].at].to;  // (both ends have a record)
    if (f0 >= n_ends || f1 >= n_ends || (f0 >> 1) == u || (f1 >> 1) == u) return false;
    const End back = end_between(g.link_offsets[f1 ^ 1u], g.link_offsets[(f1 ^ 1u) + 1], g.n_links);
    uint32_t x[4];
    load_records(g, back, x);
    Info w[4];
    BL_UNROLL
    for (uint32_t i = 0; i < 4; ++i) w[i] = x[i] < n_ends && (x[i] >> 1) != u ? info_of(g, r.k, x[i] >> 1) : no_info();
    uint32_t ahead[4], behind[4];  // out(x)[0] and out(x ^ 1)[0] where both ends of w have one record
    BL_UNROLL
    for (uint32_t i = 0; i < 4; ++i) {
        ahead[i] = behind[i] = NO_END;
        if (w[i].end[0].deg == 1 && w[i].end[1].deg == 1) {  // (no_info: degree 0)
            const uint32_t p = g.links[w[i].end[0].at].to, m = g.links[w[i].end[1].at].to;
            ahead[i] = (x[i] & 1u) ? m : p;
            behind[i] = (x[i] & 1u) ? p : m;
        }
    }
    bool marked = false;
    BL_UNROLL
    for (uint32_t i = 0; i < 4; ++i) {
        if (ahead[i] != f0 || behind[i] != f1 || w[i].keys > r.max_bubble_keys) continue;  // (f0, f1 < n_ends: never NO_END)
        const uint64_t diff = w[i].keys > me.keys ? w[i].keys - me.keys : me.keys - w[i].keys;
        if (diff <= r.max_bubble_diff && precedes(w[i], x[i] >> 1, me, u)) marked = true;
    }
    return marked;
}

// ---- bl_unitigs_mark: unitig u < n_unitigs -> its mark; keys / sum: its L and S for the statistics
BL_DEV uint8_t mark_thread(const Graph& g, const Rule& r, uint64_t u, uint64_t& keys, uint64_t& sum)
{
    const Info me = info_of(g, r.k, u);
    keys = me.keys;
    sum = me.sum;
    const bool dead0 = me.end[0].deg == 0, dead1 = me.end[1].deg == 0;
    if (dead0 && dead1) {
        const bool hit = (r.flags & ISOLATED) && me.keys <= r.max_isolated_keys && (u128)me.sum <= (u128)r.max_isolated_mean * me.keys;
        return hit ? ISLAND : KEEP;
    }
    if (dead0 || dead1) {
        if (!(r.flags & TIPS)) return KEEP;
        const uint32_t e = tip_live_end(me, u, r.max_tip_keys);
        return e != NO_END && tip_rule(g, r, u, me, e) ? TIP : KEEP;
    }
    if (!(r.flags & BUBBLES) || me.end[0].deg != 1 || me.end[1].deg != 1 || me.keys > r.max_bubble_keys) return KEEP;
    return bubble_rule(g, r, u, me) ? BUBBLE : KEEP;
}

// ---- bl_table_remove_unitigs.  Tile t of R rows: lane l reads slot t * 64 R + row * 64 + l in row `row`.
template <int R>
BL_DEV uint64_t tile_slot(uint64_t tile, int row, int lane)
{
    return tile * (uint64_t)(64 * R) + (uint64_t)row * 64 + (uint64_t)lane;
}

template <int R>
BL_DEV uint64_t tiles_of(uint64_t n)
{
    return (n + 64 * R - 1) / (64 * R);
}

// slot i < n stays: its node names no unitig below n_unitigs, or one whose mark is 0
BL_DEV bool keeps(const bllnk::Node* nodes, const uint8_t* marks, uint64_t n_unitigs, uint64_t i)
{
    const uint32_t u = nodes[i].unitig;
    return u >= n_unitigs || marks[u] == 0;
}

// the lanes below `lane` that keep their key in this row
BL_DEV uint32_t rank_in_row(uint64_t ballot, int lane)
{
    return (uint32_t)__builtin_popcountll(ballot & (((uint64_t)1 << lane) - 1));
}

template <int W>
BL_DEV void move_key(const uint64_t* keys, const uint32_t* counts, uint64_t from, uint64_t* out_keys, uint32_t* out_counts, uint64_t to)
{
    if (W == 2) reinterpret_cast<bllk::Key2*>(out_keys)[to] = reinterpret_cast<const bllk::Key2*>(keys)[from];  // one 16-byte load and store
    else out_keys[to] = keys[from];
    out_counts[to] = counts[from];
}

}  // namespace blcl
