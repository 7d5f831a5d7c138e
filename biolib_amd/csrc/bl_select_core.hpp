// bl_select_core.hpp — per-thread bodies of bl_batch_select (a new batch from per-read spans) and bl_read_spans (spans from whole-read
// bl_read_counts records).  Compiled two ways like bl_read_counts_core.hpp: by hipcc for gfx950 (bl_select.hip) and by a host compiler
// under BL_CPU_EMU for tests/emu/emu_select.cpp, which runs the threads as loops over arrays of exactly their sizes.
//
// bl_batch_select in four stages:
//   1  span_lengths    per source read: its span clamped to the read, the span's length, its absolute first base, a keep flag
//   2  (rocPRIM)       exclusive sums of the lengths (the result's offsets, by source read) and of the keep flags (the compacted index)
//   3  place_sequence  per kept read: its row of the result — output offset, absolute source start, source index
//   4  the gather      per 16 output bytes: the bytes (the wave's search, window_load / window_shift, gather_pieces)
//
// Safety.  The caller's offsets and spans are trusted for content only.  Stage 1 clamps every boundary to [0, n_bases] and takes
// offsets[i + 1] < offsets[i] as length 0, so start + len <= n_bases for every read whatever the two arrays hold; everything behind
// stage 1 reads only arrays the library wrote.  Wrong offsets give a wrong batch (spans may overlap in the source), nothing else.
//
// The gather is output-centric: a wave produces WAVE_BYTES contiguous output bytes, a lane CHUNKS_PER_LANE chunks of 16.  The wave first
// finds the sequence that holds its first byte — the LAST one whose offset is <= the byte, which skips the empty ones — by a 64-ary
// search over all of [0, n_out) with all its lanes, then keeps the next 64 offsets and source starts in its lanes' registers.  Where
// those cover the wave's last byte (sequences of 64 bytes or more on average), a chunk finds its sequence, its begin, end and source
// by shuffles alone: no load stands between a lane and its source bytes.  Otherwise a chunk bisects the offsets in memory between the
// wave's first and last sequence.  A chunk that lies whole inside one sequence takes the aligned source dwords that cover its 16
// bytes (four, or five where the source is not dword aligned) and shifts them into place with funnel shifts; the loads of all of a
// lane's chunks are issued before the first is used.  That path is taken only where the last of those dwords ends at or in front of
// n_bases: no byte at or behind n_bases is read (a bl_batch_from_device source has no slack).  Every other chunk — a sequence seam,
// the result's last partial chunk, the source's tail — goes piece by piece (gather_pieces): seventeen one-byte sequences in one chunk
// are sixteen pieces.  Bytes behind the result's total are stored as 0 (the zeroed slack of a batch buffer).
#pragma once
#include "bl_scan_core.hpp"

namespace blsel {

constexpr int TPB = 256;                          // threads of a workgroup, every kernel
constexpr int CHUNK = 16;                         // output bytes per store
constexpr int CHUNKS_PER_LANE = 4;                // chunks a lane of the gather produces: loads of four chunks in flight
constexpr int WAVE_BYTES = 64 * CHUNK * CHUNKS_PER_LANE;  // output bytes of a wave of the gather: 4 KiB, 1 KiB per step
constexpr uint32_t KEEP_EMPTY = 1u;               // include/biolib_amd.h: BL_SELECT_KEEP_EMPTY

struct SelectParams {
    // the source
    const uint8_t* bases;     // [n_bases], 16-byte aligned, nothing behind it
    uint64_t n_bases;
    const uint64_t* offsets;  // n_seqs + 1 words, or NULL: read i = [i * read_len, (i + 1) * read_len) cut at n_bases
    uint64_t n_seqs;
    uint64_t read_len;        // >= 1 where offsets is NULL (a single sequence: max(n_bases, 1))
    const uint64_t* spans;    // [n_seqs][2]
    uint32_t flags;
    // stage 1 -> 2 (by source read; entry n_seqs is 0, so that an exclusive sum over n_seqs + 1 entries ends in the total)
    uint64_t* len;            // [n_seqs + 1]
    uint64_t* keep;           // [n_seqs + 1]
    uint64_t* start;          // [n_seqs]: absolute first base of the span
    // stage 2 -> 3
    const uint64_t* len_sum;  // [n_seqs + 1]
    const uint64_t* keep_sum; // [n_seqs + 1]
    // the result (n_out and total are known on the host after stage 2)
    uint64_t n_out, total;
    uint64_t* out_offsets;    // [n_out + 1]: the library's, handed over with the batch
    uint64_t* src_start;      // [n_out]
    uint64_t* user_offsets;   // [n_out + 1] or NULL
    uint64_t* source_index;   // [n_out] or NULL
    uint8_t* out;             // [(total + 15) / 16 * 16] at least
};

// boundary j of the source, j in [0, n_seqs], clamped to [0, n_bases]
BL_DEV uint64_t boundary(const uint64_t* offsets, uint64_t read_len, uint64_t n_bases, uint64_t j)
{
    if (offsets) {
        const uint64_t b = offsets[j];
        return b < n_bases ? b : n_bases;
    }
    if (read_len != 0 && j > n_bases / read_len) return n_bases;  // (no wrap in the product below)
    const uint64_t b = j * read_len;
    return b < n_bases ? b : n_bases;
}

// read i < n_seqs: its first base and its length; first + len <= n_bases
BL_DEV void read_extent(const uint64_t* offsets, uint64_t read_len, uint64_t n_bases, uint64_t i, uint64_t& first, uint64_t& len)
{
    first = boundary(offsets, read_len, n_bases, i);
    const uint64_t e = boundary(offsets, read_len, n_bases, i + 1);
    len = e > first ? e - first : 0;
}

// ---- stage 1: thread i in [0, n_seqs]
BL_DEV void span_lengths(const SelectParams& p, uint64_t i)
{
    if (i > p.n_seqs) return;
    if (i == p.n_seqs) {
        p.len[i] = 0;
        p.keep[i] = 0;
        return;
    }
    uint64_t first, L;
    read_extent(p.offsets, p.read_len, p.n_bases, i, first, L);
    const uint64_t b0 = p.spans[2 * i], e0 = p.spans[2 * i + 1];
    const uint64_t b = b0 < L ? b0 : L, e = e0 < L ? e0 : L;
    const uint64_t n = e > b ? e - b : 0;
    p.len[i] = n;
    p.start[i] = first + b;  // (+ n <= first + L <= n_bases)
    p.keep[i] = (n != 0 || (p.flags & KEEP_EMPTY)) ? 1 : 0;
}

// ---- stage 3: thread i in [0, n_seqs]; the keep sums are the library's own: keep_sum[i] < n_out where keep[i] is set
BL_DEV void place_sequence(const SelectParams& p, uint64_t i)
{
    if (i > p.n_seqs) return;
    if (i == p.n_seqs) {
        p.out_offsets[p.n_out] = p.total;
        if (p.user_offsets) p.user_offsets[p.n_out] = p.total;
        return;
    }
    if (!p.keep[i]) return;
    const uint64_t j = p.keep_sum[i];
    if (j >= p.n_out) return;  // (never)
    const uint64_t at = p.len_sum[i];
    p.out_offsets[j] = at;
    p.src_start[j] = p.start[i];
    if (p.user_offsets) p.user_offsets[j] = at;
    if (p.source_index) p.source_index[j] = i;
}

// ---- stage 4

// the last q in [lo, hi] with out_offsets[q] <= x; lo if there is none.  lo <= hi < n_out: reads out_offsets[lo + 1 .. hi] only.
BL_DEV uint64_t seq_of(const uint64_t* out_offsets, uint64_t x, uint64_t lo, uint64_t hi)
{
    uint64_t b = lo, e = hi + 1;
    while (b + 1 < e) {
        const uint64_t mid = b + ((e - b) >> 1);
        if (out_offsets[mid] <= x) b = mid;
        else e = mid;
    }
    return b;
}

// the first output byte of wave `wave` of the grid, and of its step u
BL_DEV uint64_t wave_first_byte(uint64_t wave) { return wave * (uint64_t)WAVE_BYTES; }
BL_DEV uint64_t chunk_first_byte(uint64_t wave, int u, int lane) { return wave_first_byte(wave) + (uint64_t)(u * 64 + lane) * CHUNK; }

// ---- the wave's search.  The kernel (and the emulation) run these steps over the 64 lanes; a ballot joins them.
//
// The sequence of the wave's first byte x: the last q in [0, n_out) with out_offsets[q] <= x, by a 64-ary search — every step the 64
// lanes probe 64 evenly spaced entries of [b, e) and the count of probes at or below x (a prefix of the lanes: the offsets are the
// library's own, non-decreasing) narrows the interval 64-fold: three dependent loads for 10^5 sequences, four for 10^7.
BL_DEV uint64_t kary_step(uint64_t b, uint64_t e) { return (e - b + 63) / 64; }  // e - b >= 2
BL_DEV bool kary_probe(const uint64_t* out_offsets, uint64_t b, uint64_t e, int lane, uint64_t x)
{
    const uint64_t q = b + (uint64_t)(lane + 1) * kary_step(b, e);
    return q < e && out_offsets[q] <= x;
}
BL_DEV void kary_narrow(uint64_t& b, uint64_t& e, uint64_t probes_below)  // probes_below: the ballot's popcount
{
    const uint64_t step = kary_step(b, e);
    b += probes_below * step;
    e = e < b + step ? e : b + step;
}

// What a lane keeps in registers for the wave whose first sequence is lo: the offset of sequence lo + 1 + lane (all ones behind the
// array: entry n_out, the total, is the last) and the source start of sequence lo + lane.
BL_DEV uint64_t lane_offset(const SelectParams& p, uint64_t lo, int lane)
{
    const uint64_t q = lo + 1 + (uint64_t)lane;
    return q <= p.n_out ? p.out_offsets[q] : ~0ull;
}
BL_DEV uint64_t lane_source(const SelectParams& p, uint64_t lo, int lane)
{
    const uint64_t q = lo + (uint64_t)lane;
    return q < p.n_out ? p.src_start[q] : 0;
}
// the last byte of the wave inside the result
BL_DEV uint64_t wave_last_byte(const SelectParams& p, uint64_t wave)
{
    const uint64_t x = wave_first_byte(wave) + (uint64_t)WAVE_BYTES - 1;
    return x < p.total ? x : p.total - 1;
}
// With fewer than 64 lane offsets at or below the wave's last byte, every sequence of the wave is in the lanes' registers: the
// sequence of byte x is lo + the number of lane offsets <= x, found by six shuffles (count_step), and its begin, end and source are
// shuffles too.  Otherwise (sequences shorter than 64 bytes on average) the chunks look them up in memory: seq_of between lo and hi.
BL_DEV void count_step(uint32_t& cnt, uint32_t step, uint64_t probed, uint64_t x)  // probed: the offset lane cnt + step - 1 holds
{
    if (probed <= x) cnt += step;
}

// the sequence a chunk starts in
struct SeqAt {
    uint64_t j, begin, end, src;  // index, first and one-past-last output byte, source byte of `begin`
};
BL_DEV SeqAt seq_from_memory(const SelectParams& p, uint64_t x, uint64_t lo, uint64_t hi)
{
    SeqAt s;
    s.j = seq_of(p.out_offsets, x, lo, hi);
    s.begin = p.out_offsets[s.j];
    s.end = p.out_offsets[s.j + 1];
    s.src = p.src_start[s.j];
    return s;
}

// ---- the bytes.  A window is the 16 source bytes from (virtual) source byte vsrc on, taken as the aligned dwords that cover them —
// four, or five where vsrc is not a multiple of 4 — and shifted into place.  bases is 16-byte aligned, so these are aligned loads.
// Loadable only where all of them lie inside [0, n_bases).
BL_DEV bool window_loadable(uint64_t n_bases, int64_t vsrc)
{
    if (vsrc < 0) return false;
    const uint64_t a = (uint64_t)vsrc & ~3ull;
    return a + (((uint64_t)vsrc & 3u) ? 20u : 16u) <= n_bases;
}
BL_DEV void window_load(const uint8_t* bases, uint64_t vsrc, uint32_t v[5])
{
    const uint32_t* d = reinterpret_cast<const uint32_t*>(bases + (vsrc & ~3ull));
    BL_UNROLL
    for (int i = 0; i < 4; ++i) v[i] = d[i];
    v[4] = (vsrc & 3u) ? d[4] : 0u;
}
BL_DEV void window_shift(const uint32_t v[5], uint64_t vsrc, uint32_t w[4])
{
    const int sh = 8 * (int)(vsrc & 3u);
    BL_UNROLL
    for (int i = 0; i < 4; ++i) w[i] = bl::funnel_shr(v[i + 1], v[i], sh);  // (sh = 0: the low word)
}
// the bytes [t0, t1) of a chunk (0 <= t0 < t1 <= 16) as a mask of its dword i
BL_DEV uint32_t piece_mask(int i, int t0, int t1)
{
    int lo = t0 - 4 * i, hi = t1 - 4 * i;
    lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
    hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
    return (uint32_t)(((1ull << (8 * hi)) - 1) & ~((1ull << (8 * lo)) - 1));
}

// does the chunk at x0 lie whole inside s, with a loadable window?  Then its bytes are window_load / window_shift of chunk_vsrc.
BL_DEV int64_t chunk_vsrc(const SeqAt& s, uint64_t x0) { return (int64_t)(s.src + (x0 - s.begin)); }
BL_DEV bool chunk_is_one_window(const SelectParams& p, const SeqAt& s, uint64_t x0)
{
    return x0 >= s.begin && x0 + CHUNK <= s.end && window_loadable(p.n_bases, chunk_vsrc(s, x0));
}

// Every other chunk at output byte x0 (a multiple of 16, < total) — a sequence seam, the result's end, the source's head or tail — piece
// by piece: a piece is the run of the chunk's bytes that one sequence holds.  s: the sequence that holds x0; the following ones come
// from memory, empty ones skipped.  A piece takes its window where that is loadable (the bytes of the window outside the piece belong
// to the source's neighbouring reads and are masked off) and byte loads otherwise.  Seventeen one-byte sequences are sixteen pieces.
BL_DEV void gather_pieces(const SelectParams& p, uint64_t x0, SeqAt s, uint32_t w[4])
{
    w[0] = w[1] = w[2] = w[3] = 0;
    int t = 0;
    while (t < CHUNK && x0 + (uint64_t)t < p.total) {
        const uint64_t x = x0 + (uint64_t)t;
        while (x >= s.end && s.j + 1 < p.n_out) {  // (x < total = out_offsets[n_out]: ends at the sequence that holds x)
            ++s.j;
            s.begin = s.end;
            s.end = p.out_offsets[s.j + 1];
            s.src = p.src_start[s.j];
        }
        if (!(x >= s.begin && x < s.end)) break;  // (never: the arrays are the library's)
        uint64_t stop = s.end < p.total ? s.end : p.total;
        const int t1 = stop - x0 < (uint64_t)CHUNK ? (int)(stop - x0) : CHUNK;  // (> t)
        const uint64_t src = s.src + (x - s.begin);
        const int64_t vsrc = (int64_t)src - t;
        if (window_loadable(p.n_bases, vsrc)) {
            uint32_t v[5], piece[4];
            window_load(p.bases, (uint64_t)vsrc, v);
            window_shift(v, (uint64_t)vsrc, piece);
            BL_UNROLL
            for (int i = 0; i < 4; ++i) w[i] |= piece[i] & piece_mask(i, t, t1);
        } else {
            for (int tt = t; tt < t1; ++tt) {
                const uint64_t at = src + (uint64_t)(tt - t);
                const uint32_t byte = at < p.n_bases ? p.bases[at] : 0u;  // (always inside)
                w[tt >> 2] |= byte << (8 * (tt & 3));
            }
        }
        t = t1;
    }
}

// does entry r of the result's offsets (0 .. n_out, the total included) break "every sequence holds exactly `len` bases"?  The
// parser's rule (bl_parse_core.hpp: breaks_uniform_length), which makes the result a fixed-length batch.
BL_DEV bool breaks_uniform(const uint64_t* out_offsets, uint64_t n_out, uint64_t len, uint64_t r)
{
    return r <= n_out && out_offsets[r] != r * len;
}

// ---- bl_read_spans

enum { TRIM_NONE = 0, TRIM_PREFIX = 1, TRIM_SUFFIX = 2, TRIM_LONGER = 3 };

// include/biolib_amd.h: bl_read_counts, bl_span_rule
struct alignas(16) Record {
    uint32_t n_kmers, n_found, n_solid, min_count, max_count, reserved;
    uint64_t sum_counts, weak_begin, weak_end;
};
struct SpanRule {
    uint32_t trim, k;
    uint64_t min_len;
    uint32_t min_kmers;
    uint32_t solid_min_num, solid_min_den, solid_max_num, solid_max_den;
    uint32_t stat_lo, stat_hi;
    uint32_t reserved;
};

struct SpanParams {
    const uint64_t* offsets;  // as SelectParams
    uint64_t n_seqs, read_len, n_bases;
    const Record* records;    // [n_seqs]
    const uint32_t* stat;     // [n_seqs] or NULL
    SpanRule rule;
    uint64_t* spans;          // [n_seqs][2]
};

BL_DEV bool rule_valid(const SpanRule& r)
{
    return r.trim <= (uint32_t)TRIM_LONGER && r.k >= 1 && r.k <= 64 && r.solid_min_den >= 1 && r.solid_max_den >= 1 && r.solid_min_num <= r.solid_min_den &&
           r.solid_max_num <= r.solid_max_den && r.reserved == 0;
}

BL_DEV bool read_kept(const SpanRule& r, const Record& rec, const uint32_t* stat, uint64_t i)
{
    if (rec.n_kmers < r.min_kmers) return false;
    if ((uint64_t)rec.n_solid * r.solid_min_den < (uint64_t)rec.n_kmers * r.solid_min_num) return false;
    if ((uint64_t)rec.n_solid * r.solid_max_den > (uint64_t)rec.n_kmers * r.solid_max_num) return false;
    if (stat) {
        const uint32_t s = stat[i];
        if (s < r.stat_lo || s > r.stat_hi) return false;
    }
    return true;
}

// the span of a read of L bases before the keep conditions and min_len
BL_DEV void trimmed_span(const SpanRule& r, const Record& rec, uint64_t L, uint64_t& b, uint64_t& e)
{
    b = 0;
    e = L;
    if (rec.weak_begin == ~0ull || r.trim == (uint32_t)TRIM_NONE) return;
    const uint64_t cut = r.k - 1;                                                          // khmer: all of the first weak k-mer but its last base
    const uint64_t pe = rec.weak_begin >= L ? L : (rec.weak_begin + cut < L ? rec.weak_begin + cut : L);  // (no wrap: weak_begin < L)
    const uint64_t sb = rec.weak_end < L ? rec.weak_end : L;
    const bool prefix = r.trim == (uint32_t)TRIM_PREFIX || (r.trim == (uint32_t)TRIM_LONGER && pe >= L - sb);
    if (prefix) e = pe;
    else b = sb;
}

// thread i < n_seqs
BL_DEV void read_span(const SpanParams& p, uint64_t i)
{
    if (i >= p.n_seqs) return;
    uint64_t first, L, b = 0, e = 0;
    read_extent(p.offsets, p.read_len, p.n_bases, i, first, L);
    const Record rec = p.records[i];
    if (read_kept(p.rule, rec, p.stat, i)) {
        trimmed_span(p.rule, rec, L, b, e);
        if (e - b < p.rule.min_len) b = e = 0;
    }
    p.spans[2 * i] = b;
    p.spans[2 * i + 1] = e;
}

}  // namespace blsel
