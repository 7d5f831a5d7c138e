// bl_steps_core.hpp — per-thread bodies of bl_scan_read_steps (reads threaded through the compacted graph: one record per unitig visit),
// bl_link_support (how many reads crossed every link record) and bl_steps_format_gaf (the walks as GAF text).  Compiled two ways like
// bl_correct_core.hpp and bl_lookup_core.hpp: by hipcc for gfx950 (bl_steps.hip) and by a host compiler under BL_CPU_EMU for
// tests/emu/emu_steps.cpp, which runs the lanes as loops over arrays of exactly their lengths.
//
// The rule (include/biolib_amd.h).  The canonical k-mer c of the forward k-mer f at position p, found at slot i of the
// table, has the node d_nodes[i] = (u, rank r, flip fl).  With s = (f != c): o = s XOR fl, off = r where o = 0 and L(u) - 1 - r where
// o = 1, so that the k bases at p are oriented(u, o)[off : off + k].  p + 1 continues p iff both lie in one sequence, both have nodes,
// u and o agree and off(p + 1) = off(p) + 1.  A step is a maximal run of positions of the range in which each continues its predecessor.
//
// Passes of bl_scan_read_steps:
//   1  node_thread    the tile of bl_scan_kmer_counts (16 positions per lane, G searches in lockstep, search_group<true>: the slot, not the
//                     count): per position one 8-byte node load (and two offset loads where o = 1) and ONE packed word, (end << 32) | off
//                     or NO_NODE, for the range and the halo position first - 1 in front of it
//   2  classify       one lane per position: HEAD iff it has a node and does not continue its predecessor or is `first`; TAIL iff it has
//                     a node and its successor does not continue it or it is the range's last.  Heads and tails alternate, so the j-th
//                     head and the j-th tail are step j: one count -> exclusive sum -> write compacts both, nobody walks a step
//   3  make_step      one lane per step: the record from its head's word, the word in front of it (the two flags) and the sequence
// No atomic decides a placement; the only atomics add to (or maximise) the statistics words.
//
// Safety.  nodes, unitig_offsets, steps and links are trusted for content only: a node whose unitig is at or above n_unitigs is no node
// (so unitig_offsets[u + 1] is inside its n_unitigs + 1 words), offsets are only subtracted and compared, an `end` at or above
// 2 * n_unitigs names no record, link offsets are clamped to n_links, and the text writer only ever prints the numbers it is given.
#pragma once
#include "bl_format_core.hpp"
#include "bl_lookup_core.hpp"
#include "bl_unitig_records.hpp"

namespace blst {

constexpr int STPB = 256;                 // threads of a workgroup of the one-lane-per-item kernels
constexpr uint64_t NO_NODE = ~0ull;       // (an end is below 2^32 - 2: n_unitigs < 2^31)
constexpr uint32_t LINKED = 1u, CONTINUED = 2u;  // include/biolib_amd.h: BL_STEP_*
constexpr uint32_t HEAD = 1u, TAIL = 2u;

using blrec::LinkWords;
using blrec::Node;
struct alignas(16) Step {  // bl_read_step
    uint64_t pos, seq;
    uint32_t end, offset, n_kmers, flags;
};
static_assert(sizeof(Step) == 32, "two 16-byte stores");

// the device words of the statistics
enum : int { STAT_VALID = 0, STAT_FOUND, STAT_CHAINS, STAT_LINKED, STAT_LONGEST, STAT_WORDS = 8 };

// BL_ERR_INVALID reasons that need no device, behind blgr::refuse's: 0 = fine
BL_DEV int refuse(uint32_t k, uint64_t n, uint64_t n_unitigs)
{
    if (k < 3) return 5;
    if (n_unitigs > n) return 7;  // (so that (unitig << 1) | orientation fits 32 bits: n < 2^31)
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- pass 1: the nodes
struct NodeParams {
    bl::Kmer128Params km;            // staging, k; [km.first, km.end) = the halo position (first - 1, where first > 0) and the range
    bllk::TableView table;
    const Node* nodes;               // [table.n]
    const uint64_t* unitig_offsets;  // [n_unitigs + 1]
    uint64_t n_unitigs;
    int64_t first;                   // the statistics count the positions from here on
    uint64_t* words;                 // indexed by position - km.first
};

// bl::kmer128_at's canonical form with the strand it took: swapped = 1 where the reverse complement is the smaller one
BL_DEV void canonical_at(const bl::Kmer128Lane& L, int s, uint64_t& lo, uint64_t& hi, uint32_t& swapped)
{
    uint32_t f[4], c[4];
    const int fs = 30 - 2 * s;
    BL_UNROLL
    for (int j = 0; j < 4; ++j) f[j] = bl::funnel_shr(L.u[j + 1], L.u[j], fs) & L.m[j];
    BL_UNROLL
    for (int j = 0; j < 4; ++j) c[j] = bl::funnel_shr(L.r[j + 1], L.r[j], 2 * s) & L.m[j];
    lo = ((uint64_t)f[1] << 32) | f[0];
    hi = ((uint64_t)f[3] << 32) | f[2];
    const uint64_t rlo = ((uint64_t)c[1] << 32) | c[0], rhi = ((uint64_t)c[3] << 32) | c[2];
    const bool less = rhi < hi || (rhi == hi && rlo < lo);
    lo = less ? rlo : lo;
    hi = less ? rhi : hi;
    swapped = less ? 1u : 0u;
}

// the packed word of the key at `slot` (< table.n), read on strand `swapped`
BL_DEV uint64_t node_word(const NodeParams& p, uint32_t slot, uint32_t swapped)
{
    const Node nd = p.nodes[slot];  // one 8-byte load
    if (nd.unitig >= p.n_unitigs) return NO_NODE;
    const uint32_t o = swapped ^ (nd.rank_flip & 1u), r = nd.rank_flip >> 1;
    uint32_t off = r;
    if (o) {  // L(u) - 1 - r; L is needed on this strand only
        const uint32_t keys = (uint32_t)(p.unitig_offsets[nd.unitig + 1] - p.unitig_offsets[nd.unitig]) - (uint32_t)(p.km.unit - 1);
        off = keys - 1u - r;
    }
    return ((uint64_t)((nd.unitig << 1) | o) << 32) | off;
}

// A lane's 16 positions; n_valid / n_found: the valid k-mers and the nodes among the positions at or behind p.first
BL_DEV void node_thread(const NodeParams& p, const uint32_t* codes, const uint32_t* flags, int tid, int64_t q0, uint32_t& n_valid, uint32_t& n_found)
{
    const int64_t j0 = q0 + 16 * (int64_t)tid;
    uint32_t inrange;
    const uint32_t ok = bl::kmer128_ok_mask(p.km, flags, tid, j0, inrange);
    if (inrange == 0) return;
    const uint32_t counted = inrange & bl::range_mask(p.first - j0, p.km.end - j0);
    bl::Kmer128Lane L;
    bl::kmer128_lane_start(L, codes + tid, p.km.unit, true);
    BL_ROLLED
    for (int s0 = 0; s0 < bl::S; s0 += bllk::G) {
        uint64_t lo[bllk::G], hi[bllk::G];
        uint32_t slot[bllk::G], sw = 0;
        const uint32_t live = (ok >> s0) & ((1u << bllk::G) - 1u);
        BL_UNROLL
        for (int g = 0; g < bllk::G; ++g) {
            uint32_t x;
            canonical_at(L, s0 + g, lo[g], hi[g], x);
            sw |= x << g;
        }
        const uint32_t found = bllk::search_group<true>(p.table, lo, hi, live, slot);
        BL_UNROLL
        for (int g = 0; g < bllk::G; ++g) {
            const int s = s0 + g;
            if ((inrange >> s) & 1u) {
                const uint64_t w = ((found >> g) & 1u) ? node_word(p, slot[g], (sw >> g) & 1u) : NO_NODE;
                p.words[j0 + s - p.km.first] = w;
                if ((counted >> s) & 1u) n_found += w != NO_NODE ? 1u : 0u;
            }
        }
        n_valid += (uint32_t)__builtin_popcount(live & (counted >> s0));
    }
}

// ---------------------------------------------------------------------------------------------------------------- pass 2: heads and tails
struct StepParams {
    const uint64_t* words;       // the words of [s0, end): s0 = first - 1 where first > 0, else 0
    int64_t s0;
    const uint32_t* start_bits;  // bit p: a sequence starts at p (NULL: the batch is one sequence)
    int64_t first, end;
};

BL_DEV bool starts_at(const StepParams& p, int64_t pos) { return p.start_bits ? ((p.start_bits[pos >> 5] >> (pos & 31)) & 1u) != 0 : pos == 0; }

// does position pos (word cur) continue pos - 1 (word prev)?
BL_DEV bool continues(const StepParams& p, int64_t pos, uint64_t prev, uint64_t cur)
{
    if (prev == NO_NODE || cur == NO_NODE || starts_at(p, pos)) return false;
    return (cur >> 32) == (prev >> 32) && (uint32_t)cur == (uint32_t)prev + 1u;
}

// position pos in [first, end)
BL_DEV uint32_t classify(const StepParams& p, int64_t pos)
{
    const uint64_t cur = p.words[pos - p.s0];
    if (cur == NO_NODE) return 0;
    uint32_t c = 0;
    if (pos == p.first || !continues(p, pos, p.words[pos - 1 - p.s0], cur)) c |= HEAD;
    if (pos == p.end - 1 || !continues(p, pos + 1, cur, p.words[pos + 1 - p.s0])) c |= TAIL;
    return c;
}

// the head and the tail of step j as range-relative positions (a range holds at most 2^31)
BL_DEV void emit_ends(const StepParams& p, int64_t pos, uint32_t cls, uint64_t heads_before, uint64_t n_steps, uint32_t* heads, uint32_t* tails)
{
    if ((cls & HEAD) && heads_before < n_steps) heads[heads_before] = (uint32_t)(pos - p.first);
    if (cls & TAIL) {
        const uint64_t j = heads_before + (cls & HEAD) - 1;  // (a tail has a head at or in front of it)
        if (j < n_steps) tails[j] = (uint32_t)(pos - p.first);
    }
}

// ---------------------------------------------------------------------------------------------------------------- pass 3: the records
struct FinishParams {
    StepParams sp;
    const uint32_t* heads;        // [n_steps]
    const uint32_t* tails;        // [n_steps]
    uint64_t n_steps;
    const uint64_t* seq_offsets;  // n_seqs + 1 words, or NULL: sequence = position / read_len (read_len != 0) or 0
    uint64_t n_seqs, read_len;
};

// the last q in [0, n_seqs) with offsets[q] <= pos (the empty sequences in front of it share the offset and are skipped); reads
// offsets[1 .. n_seqs - 1] only
BL_DEV uint64_t sequence_of(const FinishParams& p, uint64_t pos)
{
    if (p.seq_offsets) {
        uint64_t b = 0, e = p.n_seqs;
        while (b + 1 < e) {
            const uint64_t mid = b + ((e - b) >> 1);
            if (p.seq_offsets[mid] <= pos) b = mid;
            else e = mid;
        }
        return b;
    }
    if (p.read_len) {
        const uint64_t q = pos / p.read_len;
        return q < p.n_seqs ? q : p.n_seqs - 1;
    }
    return 0;
}

BL_DEV Step make_step(const FinishParams& p, uint64_t j)
{
    const StepParams& sp = p.sp;
    const int64_t pos = sp.first + (int64_t)p.heads[j];
    const uint64_t cur = sp.words[pos - sp.s0];
    Step st;
    st.pos = (uint64_t)pos;
    st.seq = sequence_of(p, (uint64_t)pos);
    st.end = (uint32_t)(cur >> 32);
    st.offset = (uint32_t)cur;
    st.n_kmers = p.tails[j] - p.heads[j] + 1u;
    st.flags = 0;
    if (pos > 0 && !starts_at(sp, pos)) {  // pos - 1 lies in the same sequence (and at or behind s0)
        const uint64_t prev = sp.words[pos - 1 - sp.s0];
        if (prev != NO_NODE) st.flags = continues(sp, pos, prev, cur) ? CONTINUED : LINKED;  // (continued: only the head at `first`)
    }
    return st;
}

// ---------------------------------------------------------------------------------------------------------------- bl_link_support
BL_DEV void add32(uint32_t* w, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BL_CPU_EMU)
    atomicAdd(w, v);
#else
    *w += v;
#endif
}

struct SupportParams {
    const Step* steps;
    uint64_t n_steps;
    const uint64_t* link_offsets;  // [2 * n_unitigs + 1]
    const LinkWords* links;        // [n_links]
    uint64_t n_links, n_unitigs;
    uint32_t* support;             // [n_links], zeroed
};

// the record e -> to among the first four of out(e): its index, or n_links
BL_DEV uint64_t find_record(const SupportParams& p, uint32_t e, uint32_t to)
{
    uint64_t b = p.link_offsets[e], x = p.link_offsets[e + 1];
    b = b < p.n_links ? b : p.n_links;
    x = x < p.n_links ? x : p.n_links;
    if (x > b + 4) x = b + 4;
    for (uint64_t r = b; r < x; ++r)
        if (p.links[r].to == to) return r;
    return p.n_links;
}

// thread i: the transition steps[i] -> steps[i + 1].  0: none, 1: counted on a record, 2: matched no record
BL_DEV int support_thread(const SupportParams& p, uint64_t i)
{
    if (i + 1 >= p.n_steps) return 0;
    const Step a = p.steps[i], b = p.steps[i + 1];
    if (!(b.flags & LINKED) || a.seq != b.seq) return 0;
    if (a.end >= 2 * p.n_unitigs || b.end >= 2 * p.n_unitigs) return 0;
    const uint64_t r0 = find_record(p, a.end, b.end), r1 = find_record(p, b.end ^ 1u, a.end ^ 1u);
    if (r0 < p.n_links) add32(&p.support[r0], 1u);
    if (r1 < p.n_links && r1 != r0) add32(&p.support[r1], 1u);  // (a self-reverse record is found twice and gets the 1 once)
    return (r0 < p.n_links || r1 < p.n_links) ? 1 : 2;
}

// ---------------------------------------------------------------------------------------------------------------- bl_steps_format_gaf
// One line per chain — a step without LINKED and every following step with it:
//   <qname>\t<qlen>\t<qstart>\t<qend>\t+\t<path>\t<plen>\t<pstart>\t<pend>\t<m>\t<m>\t255\n
// Stages:
//   1  measure_step   per step: its k-mers, its unitig's keys, the bytes of its path piece and whether it begins a chain
//   2  (rocPRIM)      the four exclusive sums over the steps: a chain's aggregates are differences of them, nobody walks a chain
//   3  chain_first / chain_length   per chain head: the step it begins at; per chain: the bytes of its line
//   4  (rocPRIM)      the exclusive sum of the line lengths: every line's first byte, the last entry the total
//   5  write_step     one lane per step: its path piece; a chain's first step also writes the fields in front of and behind the path
struct GafParams {
    const Step* steps;
    uint64_t n_steps;
    const uint64_t* unitig_offsets;  // [n_unitigs + 1]
    uint64_t n_unitigs;
    const uint64_t* seq_offsets;     // as FinishParams
    uint64_t n_seqs, read_len, n_bases;
    uint32_t k;
    uint64_t read_prefix[2], seg_prefix[2];  // byte i in bits 8 * (i & 7) of word i >> 3
    uint32_t read_prefix_len, seg_prefix_len;
    uint64_t read_first, seg_first;
    // stage 1 -> 2, [n_steps + 1] each (entry n_steps is 0); the sums lie in arrays of the same shape
    uint64_t *kmers, *keys, *path, *head;
    const uint64_t *kmers_sum, *keys_sum, *path_sum, *head_sum;
    // stage 3 -> 5
    uint64_t n_chains;
    uint64_t* chain_begin;           // [n_chains + 1]: the chain's first step; entry n_chains = n_steps
    uint64_t* line_len;              // [n_chains + 1] (entry n_chains is 0)
    const uint64_t* line_off;        // [n_chains + 1]
    uint64_t total;
    uint8_t* out;                    // [total]
};

BL_DEV uint64_t unitig_keys(const GafParams& p, uint32_t end)
{
    const uint64_t u = end >> 1;
    return u < p.n_unitigs ? p.unitig_offsets[u + 1] - p.unitig_offsets[u] - (uint64_t)(p.k - 1) : 0;
}

BL_DEV bool begins_chain(const GafParams& p, uint64_t i) { return i == 0 || !(p.steps[i].flags & LINKED); }

// thread i in [0, n_steps]; returns the step's CONTINUED bit
BL_DEV uint32_t measure_step(const GafParams& p, uint64_t i)
{
    if (i > p.n_steps) return 0;
    if (i == p.n_steps) {
        p.kmers[i] = p.keys[i] = p.path[i] = p.head[i] = 0;
        return 0;
    }
    const Step s = p.steps[i];
    p.kmers[i] = s.n_kmers;
    p.keys[i] = unitig_keys(p, s.end);
    p.path[i] = 1ull + p.seg_prefix_len + blfmt::digits10(p.seg_first + (s.end >> 1));
    p.head[i] = begins_chain(p, i) ? 1 : 0;
    return s.flags & CONTINUED;
}

// thread i in [0, n_steps]
BL_DEV void chain_first(const GafParams& p, uint64_t i)
{
    if (i > p.n_steps) return;
    if (i == p.n_steps) p.chain_begin[p.n_chains] = p.n_steps;
    else if (p.head[i]) p.chain_begin[p.head_sum[i]] = i;
}

struct Chain {
    uint64_t first, next;  // its steps
    uint64_t number[9];    // qname's number, qlen, qstart, qend, plen, pstart, pend, m, m
    uint32_t digits[9];
    uint64_t path_bytes, front_bytes, total;
};

BL_DEV Chain describe_chain(const GafParams& p, uint64_t c)
{
    Chain d;
    d.first = p.chain_begin[c];
    d.next = p.chain_begin[c + 1];
    const Step s = p.steps[d.first];
    uint64_t base = 0, qlen = 0;
    if (s.seq < p.n_seqs) {
        if (p.seq_offsets) {
            base = p.seq_offsets[s.seq];
            qlen = p.seq_offsets[s.seq + 1] - base;
        } else if (p.read_len) {
            base = s.seq * p.read_len;
            qlen = base < p.n_bases ? (p.n_bases - base < p.read_len ? p.n_bases - base : p.read_len) : 0;
        } else {
            qlen = p.n_bases;
        }
    }
    const uint64_t K = p.kmers_sum[d.next] - p.kmers_sum[d.first], m = K + p.k - 1;
    d.number[0] = p.read_first + s.seq;
    d.number[1] = qlen;
    d.number[2] = s.pos - base;
    d.number[3] = d.number[2] + m;
    d.number[4] = p.keys_sum[d.next] - p.keys_sum[d.first] + p.k - 1;
    d.number[5] = s.offset;
    d.number[6] = d.number[5] + m;
    d.number[7] = d.number[8] = m;
    d.path_bytes = p.path_sum[d.next] - p.path_sum[d.first];
    d.front_bytes = p.read_prefix_len + 2;  // the prefix, "+\t"
    uint64_t back = 1 + 4;                  // '\t' behind the path, "255\n"
    BL_UNROLL
    for (int j = 0; j < 9; ++j) {
        d.digits[j] = blfmt::digits10(d.number[j]);
        if (j < 4) d.front_bytes += d.digits[j] + 1;
        else back += d.digits[j] + 1;
    }
    d.total = d.front_bytes + d.path_bytes + back;
    return d;
}

// thread c in [0, n_chains]
BL_DEV void chain_length(const GafParams& p, uint64_t c)
{
    if (c > p.n_chains) return;
    p.line_len[c] = c < p.n_chains ? describe_chain(p, c).total : 0;
}

// v in nd decimal digits and a terminator; returns the byte behind them
BL_DEV uint64_t put_number(uint8_t* out, uint64_t at, uint64_t v, uint32_t nd, uint8_t term)
{
    for (uint32_t i = nd; i-- > 0;) {
        out[at + i] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    out[at + nd] = term;
    return at + nd + 1;
}

// thread i < n_steps
BL_DEV void write_step(const GafParams& p, uint64_t i)
{
    if (i >= p.n_steps) return;
    const uint64_t c = p.head_sum[i] + p.head[i] - 1;  // (step 0 begins a chain)
    const Chain d = describe_chain(p, c);
    const uint64_t line = p.line_off[c];
    if (line + d.total > p.total) return;  // (never: the sums are the library's)
    const Step s = p.steps[i];
    // the path piece
    uint64_t at = line + d.front_bytes + (p.path_sum[i] - p.path_sum[d.first]);
    const uint64_t piece = p.path[i];
    if (at + piece > line + d.front_bytes + d.path_bytes) return;  // (never)
    p.out[at++] = (s.end & 1u) ? '<' : '>';
    for (uint32_t b = 0; b < p.seg_prefix_len; ++b) p.out[at++] = (uint8_t)blfmt::packed_byte(p.seg_prefix, b);
    uint64_t number = p.seg_first + (s.end >> 1);
    for (uint32_t b = (uint32_t)(piece - 1 - p.seg_prefix_len); b-- > 0;) {
        p.out[at + b] = (uint8_t)('0' + number % 10);
        number /= 10;
    }
    if (i != d.first) return;
    // the fields in front of the path and behind it
    at = line;
    for (uint32_t b = 0; b < p.read_prefix_len; ++b) p.out[at++] = (uint8_t)blfmt::packed_byte(p.read_prefix, b);
    for (int j = 0; j < 4; ++j) at = put_number(p.out, at, d.number[j], d.digits[j], '\t');
    p.out[at++] = '+';
    p.out[at++] = '\t';
    at += d.path_bytes;
    p.out[at++] = '\t';
    for (int j = 4; j < 9; ++j) at = put_number(p.out, at, d.number[j], d.digits[j], '\t');
    p.out[at++] = '2';
    p.out[at++] = '5';
    p.out[at++] = '5';
    p.out[at++] = '\n';
}

// BL_ERR_INVALID reasons of the rule that need no device: 0 = fine (a prefix length < 0: no NUL inside the 16 bytes)
BL_DEV int refuse_rule(uint32_t flags, uint32_t k, int read_prefix_len, int seg_prefix_len, uint64_t reserved)
{
    if (flags != 0) return 1;
    if (k < 3 || k > 63 || (k & 1u) == 0) return 2;
    if (read_prefix_len < 0 || seg_prefix_len < 0) return 3;
    if (reserved != 0) return 4;
    return 0;
}

}  // namespace blst
