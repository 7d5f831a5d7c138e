// bl_table_ops_core.hpp — per-thread bodies of the count-table algebra (bl_table_combine, bl_table_filter): union, intersection and the
// two subtractions of two count tables, with a count rule and count bounds, as one linear merge with ordered output.  Compiled two ways
// like the other *_core.hpp files: by hipcc for gfx950 (bl_table_ops.hip) and by a host compiler under BL_CPU_EMU for
// tests/emu/emu_table_ops.cpp, which runs the stages lane by lane over heap arrays of exactly the staged lengths.
//
// A table is n sorted distinct keys of one or two 64-bit words (low word first; the 128-bit order, high word first) with n 32-bit counts.
//
// The merge path is bl_setops128_core.hpp's, over either key width.  The merged order of A and B puts A[i] before B[j] iff A[i] <= B[j]:
// ties go A first.  Diagonal d (0 .. na + nb) is split at i = the number of A elements among the first d merged elements, j = d - i.  A
// tile is TILE merged elements between the splits of two neighbouring tile diagonals (partition: binary search in global memory); a
// thread's ITEMS merged elements start at the split of its own diagonal inside the tile (binary search in LDS).
//
// THE RULE THAT DECIDES CORRECTNESS.  An equal pair is merged as A[i], B[j], adjacent and in this order, and either kind of diagonal — a
// thread's or a tile's — may fall between the two.
//   * The thread that takes A[i] finds the partner at its B cursor j: every B element in front of j is strictly smaller than A[i], B[j]
//     is not, so B[j] is the only candidate.  B[j] may be the first element BEHIND the thread's or the tile's B range: the tile stages
//     B[b0, min(b1 + 1, nb)), one element (key and count) more than it merges.
//   * The thread that takes B[j] finds the partner as A[i - 1] at its A cursor i: every A element in front of i is <= B[j], A[i] is not,
//     so A[i - 1] is the only candidate.  A[i - 1] may be the last element IN FRONT OF the thread's or the tile's A range: the tile
//     stages A[max(a0 - 1, 0), a1), one key more in front (the key only: the pair's count is worked out on the A side).
//   * A matched pair is emitted ONCE, from the A side, with f(a, b).  A B element emits only when it is unmatched, and only for UNION.
//   * Every index is bounded by the range lengths, whatever the keys compare like: i < la before sa[i] is read, j < lbx before sb[j] and
//     cb[j], and sa[-1] only where the tile staged a front element.  Unsorted input gives unspecified results, never a stray access.
// Both passes make the same walk (tile_thread_walk): the count pass keeps its statistics, the write pass its record of which steps took
// A and which emitted, and replays it (tile_thread_write) once the workgroup's prefix of the emit counts has given the thread its rank.
// Placement uses no atomic: a result is bit-reproducible.
#pragma once
#include "bl_scan_core.hpp"

namespace bltop {

constexpr int TPB = 256;                        // threads per workgroup
constexpr int ITEMS_U64 = 8;                    // merged elements per thread, one-word keys
constexpr int ITEMS_U128 = 8;                   // merged elements per thread, two-word keys
constexpr int TILE_U64 = TPB * ITEMS_U64;       // merged elements per tile, one-word keys
constexpr int TILE_U128 = TPB * ITEMS_U128;     // merged elements per tile, two-word keys

// include/biolib_amd.h: BL_TABLE_* and BL_COUNT_*
constexpr uint32_t OP_UNION = 0, OP_INTERSECT = 1, OP_SUBTRACT = 2, OP_COUNT_SUBTRACT = 3, N_OPS = 4;
constexpr uint32_t MODE_SUM = 0, MODE_MIN = 1, MODE_MAX = 2, MODE_LEFT = 3, MODE_RIGHT = 4, N_MODES = 5;

constexpr uint64_t MAX_OUT = 1ull << 32;  // a table holds fewer entries than this
BL_DEV bool fits_table(uint64_t n_out, uint64_t limit) { return n_out < limit; }

struct Key1 {
    uint64_t lo;
};
struct alignas(16) Key2 {
    uint64_t lo, hi;
};

BL_DEV bool key_le(const Key1& a, const Key1& b) { return a.lo <= b.lo; }
BL_DEV bool key_eq(const Key1& a, const Key1& b) { return a.lo == b.lo; }
BL_DEV bool key_le(const Key2& a, const Key2& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo <= b.lo); }
BL_DEV bool key_eq(const Key2& a, const Key2& b) { return ((a.lo ^ b.lo) | (a.hi ^ b.hi)) == 0; }

template <typename K> struct Geo;
template <> struct Geo<Key1> { static constexpr int ITEMS = ITEMS_U64, TILE = TILE_U64; };
template <> struct Geo<Key2> { static constexpr int ITEMS = ITEMS_U128, TILE = TILE_U128; };

// what is staged of a tile: the front A key, the A range, the B range and the B element behind it; the counts of all but the front key
template <typename K> constexpr int lds_keys() { return Geo<K>::TILE + 2; }
template <typename K> constexpr int lds_counts() { return Geo<K>::TILE + 1; }

// number of A elements among the first d merged elements, 0 <= d <= na + nb.  Reads A[i] for max(0, d - nb) <= i < min(d, na) and
// B[d - 1 - i] for the same i: indices inside [0, na) and [0, nb).
template <typename K, typename Index>
BL_DEV Index diag_split(const K* a, Index na, const K* b, Index nb, Index d)
{
    Index lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const Index mid = lo + ((hi - lo) >> 1);
        if (key_le(a[mid], b[d - 1 - mid])) lo = mid + 1;  // A[mid] is among the first d iff B[d - 1 - mid] >= A[mid]
        else hi = mid;
    }
    return lo;
}

// the ranges of tile t, from splits[t] and splits[t + 1] (splits[t] = diag_split at min(t * TILE, na + nb))
struct TileRange {
    unsigned long long a0, b0;
    uint32_t la, lb;  // elements merged by the tile: la + lb <= TILE
    uint32_t laf;     // 1: A[a0 - 1] is staged in front of the A range
    uint32_t lbx;     // B elements staged: lb, or lb + 1 when an element follows the range
};

template <typename K>
BL_DEV TileRange tile_range(const unsigned long long* splits, unsigned long long t, unsigned long long na, unsigned long long nb)
{
    const unsigned long long total = na + nb;
    const unsigned long long d0 = t * (unsigned long long)Geo<K>::TILE;
    const unsigned long long d1 = d0 + Geo<K>::TILE < total ? d0 + Geo<K>::TILE : total;
    const unsigned long long a0 = splits[t], a1 = splits[t + 1];
    const unsigned long long b0 = d0 - a0, b1 = d1 - a1;
    TileRange r;
    r.a0 = a0;
    r.b0 = b0;
    r.la = (uint32_t)(a1 - a0);
    r.lb = (uint32_t)(b1 - b0);
    r.laf = a0 > 0 ? 1u : 0u;
    r.lbx = r.lb + (b1 < nb ? 1u : 0u);
    if (a1 < a0 || b1 < b0 || a1 > na || b1 > nb || a0 > d0) r.la = r.lb = r.laf = r.lbx = 0;  // (unsorted input: the splits need not rise; merge nothing)
    return r;
}

// One thread's share of staging tile r: keys[0 .. laf + la + lbx) = [front A key] A range, B range [B element behind];
// counts[0 .. la + lbx) = A range, B range [B element behind].  At most TILE + 2 keys and TILE + 1 counts.
template <typename K>
BL_DEV void tile_stage_thread(const TileRange& r, const K* a, const uint32_t* ca, const K* b, const uint32_t* cb, K* keys, uint32_t* counts, uint32_t tid)
{
    const uint32_t lax = r.laf + r.la;
    for (uint32_t x = tid; x < lax; x += TPB) keys[x] = a[r.a0 - r.laf + x];
    for (uint32_t x = tid; x < r.lbx; x += TPB) keys[lax + x] = b[r.b0 + x];
    for (uint32_t x = tid; x < r.la; x += TPB) counts[x] = ca[r.a0 + x];
    for (uint32_t x = tid; x < r.lbx; x += TPB) counts[r.la + x] = cb[r.b0 + x];
}

struct Rule {
    uint32_t op, mode;
    uint32_t count_lo, count_hi;  // a key is kept iff count_lo <= c <= count_hi
};

// op and mode are known, and the mode is one the op takes
BL_DEV bool rule_ok(uint32_t op, uint32_t mode)
{
    if (op >= N_OPS || mode >= N_MODES) return false;
    return (op != OP_SUBTRACT && op != OP_COUNT_SUBTRACT) || mode == MODE_LEFT;
}

BL_DEV uint32_t sat_add(uint32_t a, uint32_t b)
{
    const uint32_t s = a + b;
    return s < a ? 0xffffffffu : s;
}

BL_DEV uint32_t combine_counts(uint32_t mode, uint32_t a, uint32_t b)
{
    switch (mode) {
    case MODE_SUM: return sat_add(a, b);
    case MODE_MIN: return a < b ? a : b;
    case MODE_MAX: return a > b ? a : b;
    case MODE_LEFT: return a;
    default: return b;
    }
}

// the A element with count a; matched: its key is in B with count b.  c: the result's count.  Returns whether the key is in the result.
BL_DEV bool decide_a(const Rule& r, uint32_t a, bool matched, uint32_t b, uint32_t& c)
{
    bool keep;
    switch (r.op) {
    case OP_UNION:
        keep = true;
        c = matched ? combine_counts(r.mode, a, b) : a;
        break;
    case OP_INTERSECT:
        keep = matched;
        c = combine_counts(r.mode, a, b);
        break;
    case OP_SUBTRACT:
        keep = !matched;
        c = a;
        break;
    default: {  // OP_COUNT_SUBTRACT
        const uint32_t bb = matched ? b : 0u;
        keep = a > bb;
        c = a - bb;
        break;
    }
    }
    return keep && r.count_lo <= c && c <= r.count_hi;
}

// the B element with count b whose key is not in A
BL_DEV bool decide_b(const Rule& r, uint32_t b, uint32_t& c)
{
    c = b;
    return r.op == OP_UNION && r.count_lo <= b && b <= r.count_hi;
}

// bl_table_stats, one thread's share (a thread merges ITEMS elements: 32 bits hold its numbers of keys)
struct ThreadStats {
    uint32_t n_a_only, n_b_only, n_both, n_out;
    uint64_t sum_min, sum_max, sum_out;
};

// what the write pass keeps of the walk
template <typename K>
struct Walk {
    uint32_t i0, j0;   // the thread's first A and B element inside the staged ranges
    uint32_t steps;    // merged elements of the thread, 0 .. ITEMS
    uint32_t take_a;   // bit d: step d took an A element
    uint32_t emit;     // bit d: step d's element is in the result ...
    uint32_t c[Geo<K>::ITEMS];  // ... with this count
};

// One thread of either pass.  sa[-laf .. la) and ca[0 .. la) are the staged A keys and counts, sb[0 .. lbx) and cb[0 .. lbx) the B side.
// The thread merges the (at most) ITEMS elements from local diagonal tid * ITEMS; both heads and the last A key stay in registers.
template <typename K>
BL_DEV void tile_thread_walk(const Rule& rule, const K* sa, const uint32_t* ca, uint32_t la, uint32_t laf, const K* sb, const uint32_t* cb, uint32_t lb,
                             uint32_t lbx, uint32_t tid, ThreadStats& st, Walk<K>& w)
{
    constexpr uint32_t ITEMS = (uint32_t)Geo<K>::ITEMS;
    const uint32_t total = la + lb;
    const uint32_t d0 = tid * ITEMS < total ? tid * ITEMS : total;
    const uint32_t d1 = d0 + ITEMS < total ? d0 + ITEMS : total;
    uint32_t i = diag_split<K, uint32_t>(sa, la, sb, lb, d0);
    uint32_t j = d0 - i;
    w.i0 = i;
    w.j0 = j;
    w.steps = d1 - d0;
    w.take_a = w.emit = 0;
    K ha{}, hb{}, pa{};  // A head, B head, the A key in front of the A head
    bool has_pa = false;
    if (w.steps) {
        if (i < la) ha = sa[i];
        if (j < lbx) hb = sb[j];
        if (i > 0 || laf) {
            pa = *(sa + i - 1);
            has_pa = true;
        }
    }
    BL_UNROLL
    for (uint32_t d = 0; d < ITEMS; ++d) {
        w.c[d] = 0;
        if (d >= w.steps) continue;
        const bool take_a = i < la && (j >= lb || key_le(ha, hb));
        uint32_t c = 0;
        bool keep = false;
        if (take_a) {
            const bool matched = j < lbx && key_eq(ha, hb);
            const uint32_t a = ca[i];
            const uint32_t b = matched ? cb[j] : 0u;
            keep = decide_a(rule, a, matched, b, c);
            st.n_both += matched ? 1u : 0u;
            st.n_a_only += matched ? 0u : 1u;
            st.sum_min += matched ? (a < b ? a : b) : 0u;
            st.sum_max += a > b ? a : b;
            w.take_a |= 1u << d;
            pa = ha;
            has_pa = true;
            ++i;
            if (i < la) ha = sa[i];
        } else if (j < lb) {
            const bool matched = has_pa && key_eq(pa, hb);
            const uint32_t b = cb[j];
            if (!matched) {
                keep = decide_b(rule, b, c);
                st.n_b_only += 1u;
                st.sum_max += b;
            }
            ++j;
            if (j < lbx) hb = sb[j];
        }  // (neither cannot happen: the tile holds la + lb elements)
        if (keep) {
            w.emit |= 1u << d;
            w.c[d] = c;
            st.n_out += 1u;
            st.sum_out += c;
        }
    }
}

// The write pass's second half: the kept elements of the walk go to out_keys / out_counts[0 ..), the thread's own slots of the result.
template <typename K>
BL_DEV uint32_t tile_thread_write(const Walk<K>& w, const K* sa, const K* sb, K* out_keys, uint32_t* out_counts)
{
    constexpr uint32_t ITEMS = (uint32_t)Geo<K>::ITEMS;
    uint32_t i = w.i0, j = w.j0, r = 0;
    BL_UNROLL
    for (uint32_t d = 0; d < ITEMS; ++d) {
        if (d >= w.steps) continue;
        const bool from_a = (w.take_a >> d) & 1u;
        if ((w.emit >> d) & 1u) {
            out_keys[r] = from_a ? sa[i] : sb[j];
            out_counts[r] = w.c[d];
            ++r;
        }
        if (from_a) ++i;
        else ++j;
    }
    return r;
}

}  // namespace bltop
