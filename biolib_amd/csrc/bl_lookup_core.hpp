// bl_lookup_core.hpp — per-thread bodies of the count-table calls (bl_table_*, bl_scan_kmer_counts): the prefix of a key, the fill of
// the prefix index, the search for both key widths and the thread of the fused scan.  Compiled two ways like bl_kmers128_core.hpp: by
// hipcc for gfx950 (bl_lookup.hip) and by a host compiler under BL_CPU_EMU for tests/emu/emu_lookup.cpp, which runs them lane by lane
// over arrays of exactly the table's lengths.
//
// A table is n sorted distinct keys (one or two 64-bit words each, low word first; the 128-bit order of bl_sort_u128), n 32-bit counts
// and a prefix index of 2^P + 1 words: index[j] = the first slot whose key has key >> (key_bits - P) >= j, index[2^P] = n.  A search
// reads index[j] and index[j + 1] of its own prefix j and bisects inside [index[j], index[j + 1]) only: log2 of the bucket's length
// dependent loads instead of log2(n).  The answer does not depend on P: the bucket of prefix j holds every key of that prefix and no
// other, so the first key >= the query is inside it or the query is absent.
// A query with a bit at or above key_bits is absent and is answered before anything is indexed: its prefix would lie behind the index.
//
// Several searches per lane.  The keys a lane looks up (the k-mers of neighbouring positions, or unrelated queries) share nothing, so a
// single search is a chain of dependent loads with nothing to overlap.  search_group runs G searches in lockstep: every round issues the
// (up to) G loads of the group's middle elements before any of them is compared, so G loads are in flight per lane.  A search whose
// range is empty takes no further part; the loop ends when all G are done.
#pragma once
#include "bl_kmers128_core.hpp"

namespace bllk {

constexpr int MAX_PREFIX_BITS = 24;
constexpr int G = 4;  // searches in flight per lane: the scan's 16 positions go in four groups (its position loop stays rolled over the groups)

// The launch shapes of the table kernels (bl_lookup.hip).  Every kernel strides over its input from a capped grid.
constexpr int LTPB = 256;                    // threads per workgroup of the table kernels
constexpr int HIST_LDS_BINS = 8192;          // bins a workgroup keeps in LDS (32 KB)
constexpr int HIST_LDS_KEYS_MIN = 16 * LTPB; // keys a workgroup of the LDS histogram gets at least (and at least n_bins)
constexpr int LOOKUP_GRID_MAX = 256 * 32;    // workgroups of lookup_kernel at most, LTPB * G queries each per step
constexpr int HIST_LDS_GRID_MAX = 256 * 8;   // workgroups of histogram_lds_kernel at most
constexpr int TABLE_GRID_MAX = 256 * 16;     // workgroups of the one-thread-per-key kernels at most (capped_blocks_for): OR reduction, global histogram

struct alignas(16) Key2 {
    uint64_t lo, hi;
};

struct TableView {
    const uint64_t* keys;    // n * key_words words, sorted, distinct
    const uint32_t* counts;  // n
    const uint32_t* index;   // 2^prefix_bits + 1
    uint32_t n;
    uint32_t key_words;      // 1 or 2
    uint32_t key_bits;       // 1 .. 64 * key_words
    uint32_t prefix_bits;    // 0 .. min(key_bits, 24)
};

// a bit at or above key_bits (1 .. 128) is set
BL_DEV bool above_key_bits(uint64_t lo, uint64_t hi, uint32_t key_bits)
{
    if (key_bits >= 128) return false;
    if (key_bits >= 64) return key_bits == 64 ? hi != 0 : (hi >> (key_bits - 64)) != 0;
    return hi != 0 || (lo >> key_bits) != 0;
}

// key >> (key_bits - prefix_bits) of a key below 2^key_bits: below 2^prefix_bits
BL_DEV uint32_t prefix_of(uint64_t lo, uint64_t hi, uint32_t key_bits, uint32_t prefix_bits)
{
    if (prefix_bits == 0) return 0;
    const uint32_t sh = key_bits - prefix_bits;  // 0 .. 127
    if (sh >= 64) return (uint32_t)(hi >> (sh - 64));
    if (sh == 0) return (uint32_t)lo;
    return (uint32_t)((lo >> sh) | (hi << (64 - sh)));  // (the bits of hi that matter are below 2^(key_bits - 64): they land inside the prefix)
}

BL_DEV void load_key(const TableView& t, uint32_t slot, uint64_t& lo, uint64_t& hi)
{
    if (t.key_words == 2) {
        const Key2 k = reinterpret_cast<const Key2*>(t.keys)[slot];  // one 16-byte load
        lo = k.lo;
        hi = k.hi;
    } else {
        lo = t.keys[slot];
        hi = 0;
    }
}

// Index fill, one thread per word j in [0, 2^P]: the first slot whose key has a prefix >= j — a bisection of the whole table per word
// (the prefixes of sorted keys do not fall), the same work for every thread whatever the keys are; index[2^P] = n.
BL_DEV uint32_t index_entry(const TableView& t, uint32_t j)
{
    uint32_t b = 0, e = t.n;
    while (b < e) {
        const uint32_t mid = b + ((e - b) >> 1);
        uint64_t lo, hi;
        load_key(t, mid, lo, hi);
        if (prefix_of(lo, hi, t.key_bits, t.prefix_bits) < j) b = mid + 1;
        else e = mid;
    }
    return b;
}

// G searches in lockstep.  live bit g: search g takes part; the others answer 0 and read nothing.  out[g]: the stored count, 0 if absent.
// Returns the mask of the keys found.  SLOTS: out[g] is the slot of the found key instead (0 if absent: the mask tells), and no count is
// read (bl_steps_core.hpp gathers the key's node from it).
template <bool SLOTS = false>
BL_DEV uint32_t search_group(const TableView& t, const uint64_t* lo, const uint64_t* hi, uint32_t live, uint32_t* out)
{
    uint32_t b[G], e[G], e0[G];
    BL_UNROLL
    for (int g = 0; g < G; ++g) {
        b[g] = e[g] = e0[g] = 0;
        out[g] = 0;
        const bool in = ((live >> g) & 1u) && !above_key_bits(lo[g], hi[g], t.key_bits) && (t.key_words == 2 || hi[g] == 0);
        if (in) {
            const uint32_t j = prefix_of(lo[g], hi[g], t.key_bits, t.prefix_bits);
            b[g] = t.index[j];
            e[g] = e0[g] = t.index[j + 1];
        }
    }
    for (;;) {
        bool more = false;
        uint32_t mid[G];
        uint64_t mlo[G], mhi[G];
        BL_UNROLL
        for (int g = 0; g < G; ++g) {  // the round's loads, all issued before the first compare
            mid[g] = b[g] + ((e[g] - b[g]) >> 1);
            mlo[g] = mhi[g] = 0;
            if (b[g] < e[g]) load_key(t, mid[g], mlo[g], mhi[g]);
        }
        BL_UNROLL
        for (int g = 0; g < G; ++g) {
            if (b[g] < e[g]) {
                const bool less = mhi[g] < hi[g] || (mhi[g] == hi[g] && mlo[g] < lo[g]);  // table key < query
                if (less) b[g] = mid[g] + 1;
                else e[g] = mid[g];
                more = more || b[g] < e[g];
            }
        }
        if (!more) break;
    }
    // b[g]: the first slot of the bucket whose key is >= the query, or the bucket's end
    uint32_t found = 0;
    BL_UNROLL
    for (int g = 0; g < G; ++g) {
        if (b[g] < e0[g]) {
            uint64_t klo, khi;
            load_key(t, b[g], klo, khi);
            if (klo == lo[g] && khi == hi[g]) {
                out[g] = SLOTS ? b[g] : t.counts[b[g]];
                found |= 1u << g;
            }
        }
    }
    return found;
}

// bl_table_lookup_*: queries i = first, first + stride, .. (G of them) of q[0 .. nq)
BL_DEV void lookup_thread(const TableView& t, const uint64_t* q, uint64_t nq, uint64_t first, uint64_t stride, uint32_t* out)
{
    uint64_t lo[G], hi[G];
    uint32_t live = 0, c[G];
    BL_UNROLL
    for (int g = 0; g < G; ++g) {
        const uint64_t i = first + (uint64_t)g * stride;
        lo[g] = hi[g] = 0;
        if (i < nq) {
            live |= 1u << g;
            if (t.key_words == 2) {
                const Key2 k = reinterpret_cast<const Key2*>(q)[i];
                lo[g] = k.lo;
                hi[g] = k.hi;
            } else {
                lo[g] = q[i];
            }
        }
    }
    search_group(t, lo, hi, live, c);
    BL_UNROLL
    for (int g = 0; g < G; ++g) {
        const uint64_t i = first + (uint64_t)g * stride;
        if (i < nq) out[i] = c[g];
    }
}

// The fused scan: bl_scan_kmers128's tile, k-mers, validity and range rules (km), no hash; every position's k-mer is looked up.
struct ScanCountParams {
    bl::Kmer128Params km;  // staging, range, k, strand and drop_last; out_* and the sampler's fields stay NULL; shards: the digest
    TableView table;
    uint32_t* out_counts;  // indexed by position - first (nullable: digest only)
    uint8_t* out_valid;    // nullable
};

// acc: cnt, xlo, xhi as bl_scan_kmers128; xh := NUMBER of valid k-mers found in the table, sx := wrapping SUM of the counts looked up
BL_DEV void scan_counts_thread(const ScanCountParams& p, const uint32_t* codes, const uint32_t* flags, int tid, int64_t q0, bl::Kmer128Acc& acc)
{
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    uint32_t inrange;
    const uint32_t ok = bl::kmer128_ok_mask(p.km, flags, tid, j0, inrange);
    bl::Kmer128Lane L;
    bl::kmer128_lane_start(L, codes + tid, p.km.unit, p.km.canonical != 0);
    BL_ROLLED
    for (int s0 = 0; s0 < bl::S; s0 += G) {
        uint64_t lo[G], hi[G];
        uint32_t c[G];
        const uint32_t live = (ok >> s0) & ((1u << G) - 1u);
        BL_UNROLL
        for (int g = 0; g < G; ++g) {
            bl::kmer128_at(L, s0 + g, p.km.canonical != 0, lo[g], hi[g]);
            const uint32_t m32 = 0u - ((live >> g) & 1u);
            const uint64_t m = ((uint64_t)m32 << 32) | m32;
            acc.xlo ^= lo[g] & m;
            acc.xhi ^= hi[g] & m;
        }
        const uint32_t found = search_group(p.table, lo, hi, live, c);
        acc.xh += (unsigned)__builtin_popcount(found);
        BL_UNROLL
        for (int g = 0; g < G; ++g) {
            acc.sx += c[g];
            if ((inrange >> (s0 + g)) & 1u) {
                const int64_t o = j0 + s0 + g - p.km.first;
                if (p.out_counts) p.out_counts[o] = c[g];
                if (p.out_valid) p.out_valid[o] = (uint8_t)((live >> g) & 1u);
            }
        }
    }
    acc.cnt += (unsigned)__builtin_popcount(ok);
}

// bl_table_histogram: the bin of a count
BL_DEV uint32_t histogram_bin(uint32_t count, uint32_t n_bins) { return count < n_bins - 1 ? count : n_bins - 1; }

// The prefix width of a table of n distinct keys.  option: "table_prefix_bits" (-1 automatic, 0 .. 24 forced); clamped to key_bits.
// Automatic: floor(log2 n) + 4 — sixteen index words to a key, so that most searches end at the index pair — up to the cap of 24.
// Measured (profiles/lookup_bench.json): the fastest forced width was 20 at 2^16 keys and 24, the cap, at 2^22, 2^26
// and 2^28 keys; a first rule of floor(log2 n) - 4 (sixteen keys to a bucket) lost to it at every size below 2^28.  The sizes between
// and below the measured ones follow the same line unmeasured.  The index costs 64 bytes per key until the cap (64 MiB) holds it.
BL_DEV uint32_t choose_prefix_bits(int option, uint64_t n, uint32_t key_bits)
{
    const uint32_t cap = key_bits < (uint32_t)MAX_PREFIX_BITS ? key_bits : (uint32_t)MAX_PREFIX_BITS;
    uint32_t want;
    if (option >= 0) {
        want = (uint32_t)option;
    } else if (n == 0) {
        want = 0;
    } else {
        uint32_t lg = 0;
        while ((n >> (lg + 1)) != 0) ++lg;  // floor(log2 n)
        want = lg + 4;
    }
    return want < cap ? want : cap;
}

}  // namespace bllk
