// bl_read_quantiles_core.hpp — per-thread bodies of bl_select_read_counts: the k-th smallest of the valid counts of every sequence that
// lies whole inside a range, for up to four quantiles, by radix SELECTION: nothing is moved and nothing is written but the answers.
// Compiled two ways like bl_read_counts_core.hpp: by hipcc for gfx950 (bl_read_quantiles.hip) and by a host compiler under BL_CPU_EMU
// for tests/emu/emu_read_quantiles.cpp, which runs the lanes as loops, the ballots and shuffles over arrays and the LDS as a plain array.
//
// Selection.  The k-th smallest (k from 0) of m unsigned words, from the most significant digit down: among the candidates — the words
// that share the prefix fixed so far — count per next digit, step into the digit that holds rank k, subtract the candidates of the digits
// below it from k (narrow_bit, narrow_digit).  No word is compared with another one: the order is that of the digits, unsigned.
//
// Two forms.  A sequence of at most WAVE_MAX positions is taken by ONE WAVE: lane l holds the positions l, 64 + l, 128 + l .. of the
// sequence in registers (consecutive lanes read consecutive words whatever the array's alignment) with a bit mask of the valid ones,
// and narrows bit by bit from the highest bit set in any valid count; a step is a compare per slot and a ballot.  Every quantile is
// answered from the same registers.  A longer sequence is taken by ONE WORKGROUP: a first pass counts the valid positions and ORs their
// counts, then one pass per 8-bit digit (the leading zero digits skipped) fills a 256-bin histogram per quantile in LDS and wave j finds
// quantile j's bin; the values are read again in every pass, WG_CHUNK positions per step of the workgroup.
//
// Which sequences.  Work is handed out per sequence: the span of a sequence is offsets[i], offsets[i + 1] (or i * read_len, or the whole
// batch).  A sequence is taken iff first <= begin <= end <= range end: whatever the offsets hold, every position read is then inside
// the range, i.e. inside d_counts and d_valid, and every index into the offsets is in [0, n_seqs].
#pragma once
#include "bl_scan_core.hpp"

namespace blrq {

constexpr int MAX_Q = 4;                       // quantiles per call
constexpr int WAVE_SLOTS = 16;                 // positions a lane of the wave form holds: the scans' 16 per lane
constexpr int WAVE_MAX = 64 * WAVE_SLOTS;      // the longest sequence (in positions) of the wave form; a longer one goes to a workgroup
constexpr int WAVE_SLOTS_SHORT = 4;            // the wave form's body for sequences of at most 64 * 4 positions (short reads): 4 slots
constexpr int WG_TPB = 256;                    // threads of a workgroup, both kernels
constexpr int WG_UNROLL = 4;                   // loads a thread of the workgroup form has in flight
constexpr int WG_CHUNK = WG_TPB * WG_UNROLL;   // positions per step of a workgroup-form pass
constexpr int WAVE_GRID_MAX = 2048;            // workgroups of the wave kernel at most (WG_TPB / 64 waves each): a wave strides over the sequences
constexpr int WG_GRID_MAX = 1024;              // workgroups of the workgroup kernel at most: a workgroup strides over the listed sequences

struct SelectParams {
    const uint32_t* counts;   // [n]: position p of the batch at p - first
    const uint8_t* valid;     // [n]
    const uint64_t* offsets;  // n_seqs + 1 words, or NULL: sequence i = [i * read_len, (i + 1) * read_len) cut at n_bases
    uint64_t first, end;      // the range; end - first <= 2^31
    uint64_t n_bases;
    uint64_t n_seqs;          // >= 1
    uint64_t read_len;        // >= 1 where offsets is NULL (a single sequence: n_bases)
    uint32_t n_q;             // 1 .. MAX_Q
    uint32_t q_num[MAX_Q], q_den[MAX_Q];
    uint32_t* quantiles;      // [n_seqs][n_q]
    uint32_t* n_kmers;        // [n_seqs] or NULL
    uint64_t* long_list;      // sequences the wave kernel leaves to the workgroup kernel
    uint64_t long_cap;        // entries of long_list
    unsigned long long* long_count;  // appended so far (may exceed long_cap with wrong offsets: the surplus is dropped)
};

// offsets[j], j in [0, n_seqs]
BL_DEV uint64_t boundary(const SelectParams& p, uint64_t j)
{
    if (p.offsets) return p.offsets[j];
    const uint64_t b = j * p.read_len;  // (j <= n_seqs and n_seqs * read_len < n_bases + read_len: no wrap)
    return b < p.n_bases ? b : p.n_bases;
}

// The sequences that can lie whole inside the range: [lo, hi).  lo: the first boundary at or behind `first`; hi: the last boundary at or
// in front of `end`.  Bisections over [0, n_seqs]; with wrong offsets any lo, hi in that interval come out and sequence_span decides.
BL_DEV uint64_t first_boundary_from(const SelectParams& p, uint64_t pos)
{
    uint64_t b = 0, e = p.n_seqs + 1;  // the answer is in [b, e]; e = n_seqs + 1: none
    while (b < e) {
        const uint64_t mid = b + ((e - b) >> 1);
        if (boundary(p, mid) >= pos) e = mid;
        else b = mid + 1;
    }
    return b;
}
BL_DEV uint64_t last_boundary_upto(const SelectParams& p, uint64_t pos)
{
    uint64_t b = 0, e = p.n_seqs + 1;  // boundaries [0, b) are <= pos
    while (b < e) {
        const uint64_t mid = b + ((e - b) >> 1);
        if (boundary(p, mid) <= pos) b = mid + 1;
        else e = mid;
    }
    return b ? b - 1 : 0;
}
// side 0: lo, side 1: hi (two lanes search side by side)
BL_DEV uint64_t work_bound(const SelectParams& p, int side)
{
    if (side == 0) {
        const uint64_t lo = first_boundary_from(p, p.first);
        return lo < p.n_seqs ? lo : p.n_seqs;
    }
    return last_boundary_upto(p, p.end);
}

// Sequence i < n_seqs: is it whole inside the range, and where.  r0: its first position relative to `first`; len <= 2^31.
BL_DEV bool sequence_span(const SelectParams& p, uint64_t i, uint64_t& r0, uint64_t& len)
{
    const uint64_t b = boundary(p, i), e = boundary(p, i + 1);
    if (!(p.first <= b && b <= e && e <= p.end)) return false;
    r0 = b - p.first;
    len = e - b;
    return true;
}

// the rank of quantile num / den among m >= 1 sorted values
BL_DEV uint64_t rank_of(uint64_t m, uint32_t num, uint32_t den)
{
    const uint64_t r = m * (uint64_t)num / den;  // m <= 2^31, num < 2^32
    return r < m - 1 ? r : m - 1;
}

BL_DEV int highest_bit(uint32_t x) { return 31 - __builtin_clz(x); }  // x != 0

// ---- the wave form

template <int NS>
struct LaneVals {
    uint32_t v[NS];  // position s * 64 + lane of the sequence
    uint32_t ok;     // bit s: that position exists and is valid
};

template <int NS>
BL_DEV void wave_load_lane(const SelectParams& p, uint64_t r0, uint32_t len, int lane, LaneVals<NS>& L)
{
    L.ok = 0;
    BL_UNROLL
    for (int s = 0; s < NS; ++s) {
        const uint32_t j = (uint32_t)(s * 64 + lane);
        L.v[s] = 0;
        if (j < len) {
            L.v[s] = p.counts[r0 + j];
            L.ok |= (p.valid[r0 + j] != 0 ? 1u : 0u) << s;
        }
    }
}

// OR of the lane's valid counts
template <int NS>
BL_DEV uint32_t lane_or(const LaneVals<NS>& L)
{
    uint32_t x = 0;
    BL_UNROLL
    for (int s = 0; s < NS; ++s) x |= ((L.ok >> s) & 1u) ? L.v[s] : 0u;
    return x;
}

// Slot s is a candidate whose bit `bit` is 0: valid, and equal to the prefix in every bit above `bit` (the prefix's lower bits are 0)
template <int NS>
BL_DEV bool slot_in_zero_half(const LaneVals<NS>& L, int s, uint32_t prefix, int bit)
{
    return ((L.ok >> s) & 1u) && ((L.v[s] ^ prefix) >> bit) == 0;
}

// One step of the wave form.  zeros: the candidates whose bit `bit` is 0.
BL_DEV void narrow_bit(uint64_t& k, uint32_t& prefix, int bit, uint64_t zeros)
{
    if (k >= zeros) {
        k -= zeros;
        prefix |= 1u << bit;
    }
}

// ---- the workgroup form

// A pass walks the sequence in steps of WG_CHUNK positions, the last one partial: thread tid's u-th position of a step (u < WG_UNROLL)
// is step * WG_CHUNK + u * WG_TPB + tid, so that the threads of a wave read consecutive words.  False behind the sequence's end.
BL_DEV uint64_t wg_steps(uint64_t len) { return (len + WG_CHUNK - 1) / WG_CHUNK; }
BL_DEV bool wg_position(uint64_t len, uint64_t step, int u, int tid, uint64_t& j)
{
    j = step * WG_CHUNK + (uint64_t)(u * WG_TPB + tid);
    return j < len;
}

// the first pass at position j of the sequence: valid count and OR
BL_DEV void wg_census(const SelectParams& p, uint64_t r0, uint64_t j, bool inside, uint32_t& m, uint32_t& ors)
{
    if (inside && p.valid[r0 + j]) {
        ++m;
        ors |= p.counts[r0 + j];
    }
}

// the digit passes run from this shift down to 0 in steps of 8 (ors != 0)
BL_DEV int top_shift(uint32_t ors) { return highest_bit(ors) & ~7; }

// Is the count a candidate of a quantile whose prefix holds the digits above `shift`
BL_DEV bool digit_candidate(uint32_t v, uint32_t prefix, int shift) { return shift == 24 || ((v ^ prefix) >> (shift + 8)) == 0; }
BL_DEV uint32_t digit_of(uint32_t v, int shift) { return (v >> shift) & 255u; }

// a digit pass at position j: the count and whether it is valid (0, false behind the end)
BL_DEV void wg_fetch(const SelectParams& p, uint64_t r0, uint64_t j, bool inside, uint32_t& v, bool& ok)
{
    v = 0;
    ok = false;
    if (inside) {
        v = p.counts[r0 + j];
        ok = p.valid[r0 + j] != 0;
    }
}

// Wave j of the workgroup finds quantile j's bin: lane l holds bins 4l .. 4l + 3 (h) and `below`, the candidates in the bins in front of
// 4l.  The one lane that holds rank k steps into its bin; returns false for every other lane.
BL_DEV bool narrow_digit(const uint32_t h[4], uint64_t below, int lane, int shift, uint64_t& k, uint32_t& prefix)
{
    uint64_t c = below;
    for (int d = 0; d < 4; ++d) {
        if (k >= c && k < c + h[d]) {
            k -= c;
            prefix |= (uint32_t)(4 * lane + d) << shift;
            return true;
        }
        c += h[d];
    }
    return false;
}

}  // namespace blrq
