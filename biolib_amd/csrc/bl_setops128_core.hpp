// bl_setops128_core.hpp — per-thread bodies of the two intersection kernels for 16-byte keys (bl_jaccard_sorted_u128).  Compiled two
// ways like the other *_core.hpp files: by hipcc for gfx950 (bl_setops128.hip) and by a host compiler under BL_CPU_EMU for
// tests/emu/emu_setops128.cpp, which runs them lane by lane over a plain array standing for LDS.
//
// A key is the object representation of __uint128_t: low word, then high word; the order is the numeric order of the 128-bit value.
//
// The merge form (merge path).  The merged order of two sorted sets A and B puts A[i] before B[j] iff A[i] <= B[j]: ties go A first.
// Diagonal d (0 .. na+nb) is split at i = the number of A elements among the first d merged elements, j = d - i.  A tile is TILE merged
// elements: its A range [a0, a1) and B range [b0, b1) come from the splits of diagonals t*TILE and (t+1)*TILE (partition kernel, binary
// search in global memory); a thread's 8 merged elements come from the split of its own diagonal inside the tile (binary search in LDS).
// COUNTING RULE: a thread that takes A[i] with its B cursor at j counts one iff j < nb and B[j] == A[i].  Every B element before j is
// strictly smaller than A[i] (it was merged in front of it), B[j] is not (it is merged behind it), so B[j] is the only candidate and every
// common key is found exactly once — each A element is taken by exactly one thread.  B[j] may be the first element BEHIND the thread's or
// the tile's own B range (the ranges end where the diagonal falls, and it falls between an equal pair whenever the A element of the pair
// is the last one in front of it): the tile therefore stages B[b0, min(b1 + 1, nb)), one element more than it merges.
// Nothing here depends on the inputs being duplicate-free or even sorted for its memory safety: every index is bounded by the range
// lengths, whatever the keys compare like.  With duplicates the count is unspecified.
#pragma once
#include "bl_scan_core.hpp"

namespace bl128s {

constexpr int TPB = 256;           // threads per workgroup
constexpr int ITEMS = 8;           // merged elements per thread
constexpr int TILE = TPB * ITEMS;  // merged elements per tile
constexpr int LDS_KEYS = TILE + 1; // A range and B range back to back, plus the one B element behind the range

struct alignas(16) Key {
    uint64_t lo, hi;
};

BL_DEV bool key_lt(const Key& a, const Key& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
BL_DEV bool key_le(const Key& a, const Key& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo <= b.lo); }
BL_DEV bool key_eq(const Key& a, const Key& b) { return ((a.lo ^ b.lo) | (a.hi ^ b.hi)) == 0; }

// number of A elements among the first d merged elements, 0 <= d <= na + nb.  Reads A[i] for max(0, d - nb) <= i < min(d, na) and
// B[d - 1 - i] for the same i: indices inside [0, na) and [0, nb).
template <typename Index>
BL_DEV Index diag_split(const Key* a, Index na, const Key* b, Index nb, Index d)
{
    Index lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const Index mid = lo + ((hi - lo) >> 1);
        // A[mid] is among the first d iff fewer than d elements are merged in front of it: mid + #{B < A[mid]} <= d - 1, that is
        // B[d - 1 - mid] >= A[mid]
        if (key_le(a[mid], b[d - 1 - mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the ranges of tile t, from splits[t] and splits[t + 1] (splits[t] = diag_split at min(t * TILE, na + nb))
struct TileRange {
    unsigned long long a0, b0;
    uint32_t la, lb;   // elements merged by the tile: la + lb <= TILE
    uint32_t lbx;      // B elements staged: lb, or lb + 1 when an element follows the range
};

BL_DEV TileRange tile_range(const unsigned long long* splits, unsigned long long t, unsigned long long na, unsigned long long nb)
{
    const unsigned long long total = na + nb;
    const unsigned long long d0 = t * (unsigned long long)TILE;
    const unsigned long long d1 = d0 + TILE < total ? d0 + TILE : total;
    const unsigned long long a0 = splits[t], a1 = splits[t + 1];
    const unsigned long long b0 = d0 - a0, b1 = d1 - a1;
    TileRange r;
    r.a0 = a0;
    r.b0 = b0;
    r.la = (uint32_t)(a1 - a0);
    r.lb = (uint32_t)(b1 - b0);
    r.lbx = r.lb + (b1 < nb ? 1u : 0u);
    if (a1 < a0 || b1 < b0 || a1 > na || b1 > nb) r.la = r.lb = r.lbx = 0;  // (unsorted input: the splits need not rise; merge nothing)
    return r;
}

// One thread of the tile kernel: sa[0 .. la) and sb[0 .. lbx) are the staged ranges; returns the common keys found by the thread's
// (at most) 8 merge steps from local diagonal tid * 8.  Both heads are kept in registers: a step reads one 16-byte element.
BL_DEV uint32_t tile_thread_count(const Key* sa, uint32_t la, const Key* sb, uint32_t lb, uint32_t lbx, uint32_t tid)
{
    const uint32_t total = la + lb;
    const uint32_t d0 = tid * ITEMS < total ? tid * ITEMS : total;
    const uint32_t d1 = d0 + ITEMS < total ? d0 + ITEMS : total;
    uint32_t i = diag_split<uint32_t>(sa, la, sb, lb, d0);
    uint32_t j = d0 - i;
    Key ha = {0, 0}, hb = {0, 0};
    if (i < la) ha = sa[i];
    if (j < lbx) hb = sb[j];
    uint32_t found = 0;
    for (uint32_t d = d0; d < d1; ++d) {
        const bool take_a = i < la && (j >= lb || key_le(ha, hb));
        if (take_a) {
            found += (j < lbx && key_eq(ha, hb)) ? 1u : 0u;
            ++i;
            if (i < la) ha = sa[i];
        } else {
            if (j >= lb) break;  // (cannot happen: the tile holds la + lb elements)
            ++j;
            if (j < lbx) hb = sb[j];
        }
    }
    return found;
}

// The search form: 1 iff `key` is in the sorted b[0 .. nb)
BL_DEV uint32_t search_count(const Key& key, const Key* b, unsigned long long nb)
{
    unsigned long long lo = 0, hi = nb;  // first element of b that is >= key
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (key_lt(b[mid], key)) lo = mid + 1;
        else hi = mid;
    }
    return (lo < nb && key_eq(b[lo], key)) ? 1u : 0u;
}

// Which kernel option value 0 takes: the merge kernel while the larger set is less than MERGE_MAX_RATIO times the smaller one.  The
// load-count model (n_small * log2(n_large) 16-byte loads against na + nb) puts the crossing near 16; measured on an MI355X
// (profiles/setops128_bench.json, 2^24 and 2^26 keys in the larger set) the merge kernel wins at ratio 1 (1.02 against 1.89 ms) and the
// search kernel at ratio 4 already (0.575 against 0.648 ms) — sorted queries walk the same top of the search tree, which stays in
// cache — and the times cross near ratio 3: 4 is the nearest power of two.
constexpr unsigned long long MERGE_MAX_RATIO = 4;
BL_DEV bool choose_merge(unsigned long long na, unsigned long long nb)
{
    const unsigned long long small = na < nb ? na : nb, large = na < nb ? nb : na;
    return large < MERGE_MAX_RATIO * small;
}

}  // namespace bl128s
