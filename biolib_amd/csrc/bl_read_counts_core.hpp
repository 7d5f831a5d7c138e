// bl_read_counts_core.hpp — per-thread bodies of bl_scan_read_counts: bl_scan_kmer_counts's tile, k-mers, validity and searches
// (bl_lookup_core.hpp), with the 16 counts of a lane reduced per SEQUENCE on the chip instead of being stored per position.  Compiled two
// ways like bl_lookup_core.hpp: by hipcc for gfx950 (bl_read_counts.hip) and by a host compiler under BL_CPU_EMU for
// tests/emu/emu_read_counts.cpp, which runs the lanes as loops, the wave's shuffles over arrays and the atomics as plain operations.
//
// Segments.  The start bits of a lane's 16 positions (gather_flags) cut them into segments; a segment carries a Part, the seven partial
// statistics with the weak span in tile-relative positions.  A lane without a start bit is one open segment (`run`).  A lane with start
// bits has a head (in front of its first start bit: the end of a sequence that began in an earlier lane), segments closed on both sides
// (a whole sequence of 1 .. 14 bases, or empty ones: flushed by the lane itself) and a tail (`run`, from its last start bit on).
// Across the wave the `run` parts go through a segmented inclusive scan (wave_scan_takes: a lane with a start bit begins a segment), after
// which lane i holds the sum S(i) of the runs from the last lane with a start bit at or below i.  A lane with a start bit closes the
// segment in front of it: S(i - 1) + head.  Lane 63 closes what is still open at the wave's end.  So a wave flushes once per start bit it
// holds and once more, and a sequence is flushed at most once per wave it spans plus once: by its length only through the waves.
// Parts without a valid k-mer are not flushed: the identity record of bl_scan_read_counts's INIT pass is what they would leave.
//
// A flush is up to eight integer atomics on the sequence's record: they commute, so the records do not depend on the order of the waves.
//
// Which sequence.  With offsets: the last sequence whose offset is <= a position of the segment (empty sequences in front of it share the
// offset and are skipped by that rule), found by bisection.  Two lanes of a wave bisect all of [0, n_seqs) once per tile, for the wave's
// first and last position; every flush bisects only between those two, which is no load at all inside a long read.  Every index read is
// in [0, n_seqs) whatever the array holds: a wrong array gives wrong statistics and nothing else.  Without offsets: position / read_len
// (clamped to the last sequence), or sequence 0.
#pragma once
#include "bl_lookup_core.hpp"

namespace blrc {

// include/biolib_amd.h: bl_read_counts
struct alignas(16) Record {
    uint32_t n_kmers, n_found, n_solid, min_count, max_count, reserved;
    uint64_t sum_counts, weak_begin, weak_end;
};
static_assert(sizeof(Record) == 48, "three 16-byte stores");

BL_DEV Record identity_record() { return Record{0, 0, 0, 0xffffffffu, 0, 0, 0, ~0ull, 0}; }

struct ReadCountParams {
    bl::Kmer128Params km;  // as ScanCountParams::km
    bllk::TableView table;
    uint32_t min_count;       // >= 1
    const uint64_t* offsets;  // n_seqs + 1 words, or NULL: sequence = position / read_len (read_len != 0) or 0
    uint64_t n_seqs;          // >= 1
    uint64_t read_len;
    Record* records;          // n_seqs
};

// the statistics of a segment inside one tile; wb / we: tile-relative position of the first weak k-mer / 1 + that of the last
struct Part {
    uint32_t n, found, solid, mn, mx, wb, we;
    uint64_t sum;
};

BL_DEV Part identity_part() { return Part{0, 0, 0, 0xffffffffu, 0, 0xffffffffu, 0, 0}; }

BL_DEV Part merge(const Part& a, const Part& b)
{
    Part r;
    r.n = a.n + b.n;
    r.found = a.found + b.found;
    r.solid = a.solid + b.solid;
    r.mn = a.mn < b.mn ? a.mn : b.mn;
    r.mx = a.mx > b.mx ? a.mx : b.mx;
    r.wb = a.wb < b.wb ? a.wb : b.wb;
    r.we = a.we > b.we ? a.we : b.we;
    r.sum = a.sum + b.sum;
    return r;
}

// The part of the lane's positions [from, to) out of the lane's bit masks — ok: a valid k-mer starts there, fm: its key is in the table,
// sm: its count >= min_count — and the three running values of those positions.  tp0: tile-relative position of the lane's position 0.
BL_DEV Part make_part(uint32_t ok, uint32_t fm, uint32_t sm, int from, int to, uint32_t mn, uint32_t mx, uint64_t sum, uint32_t tp0)
{
    const uint32_t okm = ok & ((1u << to) - 1u) & ~((1u << from) - 1u);
    const uint32_t weak = okm & ~sm;
    Part r;
    r.n = (uint32_t)__builtin_popcount(okm);
    r.found = (uint32_t)__builtin_popcount(fm & okm);
    r.solid = (uint32_t)__builtin_popcount(sm & okm);
    r.mn = mn;
    r.mx = mx;
    r.wb = weak ? tp0 + (uint32_t)__builtin_ctz(weak) : 0xffffffffu;
    r.we = weak ? tp0 + 32u - (uint32_t)__builtin_clz(weak) : 0u;
    r.sum = sum;
    return r;
}

// the last q in [lo, hi] with offsets[q] <= pos; lo if there is none.  lo, hi < n_seqs: reads offsets[lo + 1 .. hi] only.
BL_DEV uint64_t seq_of(const uint64_t* offsets, uint64_t pos, uint64_t lo, uint64_t hi)
{
    uint64_t b = lo, e = hi + 1;
    while (b + 1 < e) {
        const uint64_t mid = b + ((e - b) >> 1);
        if (offsets[mid] <= pos) b = mid;
        else e = mid;
    }
    return b;
}

// the sequence of position pos and its first base; lo, hi: sequences the search stays between (with offsets only)
BL_DEV void locate(const ReadCountParams& p, uint64_t pos, uint64_t lo, uint64_t hi, uint64_t& seq, uint64_t& base)
{
    if (p.offsets) {
        seq = seq_of(p.offsets, pos, lo, hi);
        base = p.offsets[seq];
    } else if (p.read_len) {
        seq = pos / p.read_len;
        if (seq >= p.n_seqs) seq = p.n_seqs - 1;
        base = seq * p.read_len;
    } else {
        seq = 0;
        base = 0;
    }
}

// The records a call touches: those of the sequences from the one that holds `first` to the one that holds `end - 1`, the empty ones
// between them included.  INIT sets exactly these to the identity.
BL_DEV void touched_span(const ReadCountParams& p, uint64_t& lo, uint64_t& hi)
{
    uint64_t base;
    locate(p, (uint64_t)p.km.first, 0, p.n_seqs - 1, lo, base);
    locate(p, (uint64_t)p.km.end - 1, 0, p.n_seqs - 1, hi, base);
}

// The atomics of a flush (the emulation runs one lane at a time: plain operations there).
BL_DEV void rc_add32(uint32_t* w, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    atomicAdd(w, v);
#else
    *w += v;
#endif
}
BL_DEV void rc_min32(uint32_t* w, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    atomicMin(w, v);
#else
    *w = *w < v ? *w : v;
#endif
}
BL_DEV void rc_max32(uint32_t* w, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    atomicMax(w, v);
#else
    *w = *w > v ? *w : v;
#endif
}
BL_DEV void rc_add64(uint64_t* w, uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    atomicAdd(reinterpret_cast<unsigned long long*>(w), (unsigned long long)v);
#else
    *w += v;
#endif
}
BL_DEV void rc_min64(uint64_t* w, uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    atomicMin(reinterpret_cast<unsigned long long*>(w), (unsigned long long)v);
#else
    *w = *w < v ? *w : v;
#endif
}
BL_DEV void rc_max64(uint64_t* w, uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    atomicMax(reinterpret_cast<unsigned long long*>(w), (unsigned long long)v);
#else
    *w = *w > v ? *w : v;
#endif
}

// A closed segment into its sequence's record.  pos: any position of the segment (its sequence is looked for between lo and hi).
// Nothing is located or written for a part without a k-mer; an atomic that could not change its word is left out.
BL_DEV void flush(const ReadCountParams& p, const Part& a, int64_t q0, uint64_t pos, uint64_t lo, uint64_t hi)
{
    if (a.n == 0) return;
    uint64_t seq, base;
    locate(p, pos, lo, hi, seq, base);
    Record* r = p.records + seq;
    rc_add32(&r->n_kmers, a.n);
    if (a.found) rc_add32(&r->n_found, a.found);
    if (a.solid) rc_add32(&r->n_solid, a.solid);
    rc_min32(&r->min_count, a.mn);
    if (a.mx) rc_max32(&r->max_count, a.mx);
    if (a.sum) rc_add64(&r->sum_counts, a.sum);
    if (a.we) {
        rc_min64(&r->weak_begin, (uint64_t)q0 + a.wb - base);
        rc_max64(&r->weak_end, (uint64_t)q0 + a.we - base);
    }
}

// What the wave's two searching lanes look for: lane 0 the wave's first position, lane 1 its last, both inside the batch.
BL_DEV uint64_t wave_bound_position(const ReadCountParams& p, int64_t q0, int wv, int lane)
{
    const int64_t pos = q0 + (int64_t)wv * (64 * bl::S) + (lane == 0 ? 0 : 64 * bl::S - 1);
    return (uint64_t)(pos < p.km.n_bases ? pos : p.km.n_bases - 1);
}

// A lane's 16 positions.  acc: the digest of scan_counts_thread, word for word.  start16: the lane's start bits; head: the part in front
// of the first of them (identity without one); run: the part behind the last of them, or of the whole lane.  Segments closed on both
// sides are flushed here; lo, hi: the wave's first and last sequence.
BL_DEV void read_counts_lane(const ReadCountParams& p, const uint32_t* codes, const uint32_t* flags, int tid, int64_t q0, uint64_t lo_seq, uint64_t hi_seq,
                             bl::Kmer128Acc& acc, uint32_t& start16, Part& head, Part& run)
{
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    uint32_t inrange;
    const uint32_t ok = bl::kmer128_ok_mask(p.km, flags, tid, j0, inrange);
    bl::Bits128 good, start;
    bl::gather_flags(flags, tid, good, start);
    start16 = (uint32_t)start.lo & 0xffffu;
    bl::Kmer128Lane L;
    bl::kmer128_lane_start(L, codes + tid, p.km.unit, p.km.canonical != 0);
    // What the loop carries: two more bit masks beside ok, and the minimum, maximum and sum since the last start bit (r_*) and in front
    // of the first one (h_*).  The counters and the weak span of a segment come out of the masks when it is closed (make_part).
    uint32_t fm = 0, sm = 0;
    uint32_t h_mn = 0xffffffffu, h_mx = 0, r_mn = 0xffffffffu, r_mx = 0;
    uint64_t h_sum = 0, r_sum = 0;
    const uint32_t tp0 = (uint32_t)(16 * tid);
    BL_ROLLED
    for (int s0 = 0; s0 < bl::S; s0 += bllk::G) {
        uint64_t lo[bllk::G], hi[bllk::G];
        uint32_t c[bllk::G];
        const uint32_t live = (ok >> s0) & ((1u << bllk::G) - 1u);
        BL_UNROLL
        for (int g = 0; g < bllk::G; ++g) {
            bl::kmer128_at(L, s0 + g, p.km.canonical != 0, lo[g], hi[g]);
            const uint32_t m32 = 0u - ((live >> g) & 1u);
            const uint64_t m = ((uint64_t)m32 << 32) | m32;
            acc.xlo ^= lo[g] & m;
            acc.xhi ^= hi[g] & m;
        }
        const uint32_t found = bllk::search_group(p.table, lo, hi, live, c);  // (c is 0 where live is)
        acc.xh += (unsigned)__builtin_popcount(found);
        fm |= found << s0;
        BL_UNROLL
        for (int g = 0; g < bllk::G; ++g) {
            const int s = s0 + g;
            if ((start16 >> s) & 1u) {  // a sequence starts at s: what ran up to s - 1 is closed
                const uint32_t before = start16 & ((1u << s) - 1u);
                if (before == 0) {
                    h_mn = r_mn;
                    h_mx = r_mx;
                    h_sum = r_sum;
                } else {  // closed on both sides inside the lane
                    flush(p, make_part(ok, fm, sm, 31 - __builtin_clz(before), s, r_mn, r_mx, r_sum, tp0), q0, (uint64_t)(j0 + s - 1), lo_seq, hi_seq);
                }
                r_mn = 0xffffffffu;
                r_mx = 0;
                r_sum = 0;
            }
            const uint32_t okb = (live >> g) & 1u;
            const uint32_t lowest = c[g] | (okb - 1u);  // all ones where no k-mer starts
            acc.sx += c[g];
            sm |= (okb & (c[g] >= p.min_count ? 1u : 0u)) << s;
            r_mn = r_mn < lowest ? r_mn : lowest;
            r_mx = r_mx > c[g] ? r_mx : c[g];
            r_sum += c[g];
        }
    }
    acc.cnt += (unsigned)__builtin_popcount(ok);
    if (start16) {
        head = make_part(ok, fm, sm, 0, __builtin_ctz(start16), h_mn, h_mx, h_sum, tp0);
        run = make_part(ok, fm, sm, 31 - __builtin_clz(start16), bl::S, r_mn, r_mx, r_sum, tp0);
    } else {
        head = identity_part();
        run = make_part(ok, fm, sm, 0, bl::S, r_mn, r_mx, r_sum, tp0);
    }
}

// The segmented scan over the wave's `run` parts.  starts: bit i = lane i has a start bit.  The lane that begins lane's segment:
BL_DEV int wave_seg_head(uint64_t starts, int lane)
{
    const uint64_t below = starts & (~0ull >> (63 - lane));  // lanes 0 .. lane
    return below ? 63 - __builtin_clzll(below) : 0;
}
// step d (1, 2, 4 .. 32): the lane adds the part lane - d holds, merge(theirs, mine)
BL_DEV bool wave_scan_takes(int lane, int d, int seg_head) { return lane - d >= seg_head; }

// After the scan.  mine: S(lane); below: S(lane - 1), the identity for lane 0.
BL_DEV void wave_close(const ReadCountParams& p, int tid, int64_t q0, uint32_t start16, const Part& head, const Part& mine, const Part& below, uint64_t lo_seq,
                       uint64_t hi_seq)
{
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    if (start16) flush(p, merge(below, head), q0, (uint64_t)(j0 + __builtin_ctz(start16) - 1), lo_seq, hi_seq);
    if ((tid & 63) == 63) {
        const int64_t last = j0 + bl::S - 1;
        flush(p, mine, q0, (uint64_t)(last < p.km.end ? last : p.km.end - 1), lo_seq, hi_seq);
    }
}

}  // namespace blrc
