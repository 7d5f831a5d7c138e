// bl_links_core.hpp — per-thread bodies of bl_unitig_links: the edges between the ends of the unitigs bl_table_unitigs made, as a CSR pair.
// The definitions are stated in full in include/biolib_amd.h.  Compiled two ways like bl_graph_core.hpp: by hipcc for gfx950
// (bl_links.hip) and by a host compiler under BL_CPU_EMU for tests/emu/emu_links.cpp, which runs every body lane by lane over arrays of
// exactly their lengths.
//
// Three passes around one rocPRIM exclusive sum:
//   1  end_key_thread   per key: where its rank is 0 or L - 1 it is an end of its unitig and writes its slot into end_key[2u + o]
//   2  end_search       the hot one, per end: the side the end leaves its key by, that side's four successors looked up with the lockstep
//                       searches of the mask pass (blgr::lower_bound_group) — but keeping every neighbour's slot, not only the last — then
//                       one 8-byte load of the neighbour's node per set bit.  The (up to four) `to` words that pass the ONCE filter are
//                       parked, 16 bytes per end, and their number is the end's degree
//   3  emit_thread      per end, behind the exclusive sum of the degrees: the parked words become records at the end's offset
// Searching once and parking was chosen over searching twice: a search is up to five dependent chains of about log2(bucket) key loads
// per end, parking is one 16-byte store and one 16-byte load per end, both coalesced.
//
// Safety.  d_nodes and d_unitig_offsets are trusted for content only: a node whose unitig is at or above n_unitigs names no end and no
// `to` word (it is ignored), a rank is only ever compared, and the flip bit is a bit.  end_key is the library's own: an entry is a slot
// below n or END_NONE.  Nothing outside [0, n) of the nodes, [0, n_unitigs] of the offsets and the table's own arrays is read.
#pragma once
#include "bl_graph_core.hpp"
#include "bl_unitig_records.hpp"

namespace bllnk {

using blgr::K128;
using blgr::TableView;

constexpr int LTPB = 256;  // threads per workgroup of every kernel of bl_links.hip: one thread per key or per end, no grid is capped
constexpr uint32_t ONCE = 1u;             // include/biolib_amd.h: BL_LINKS_ONCE
constexpr uint32_t END_NONE = 0xFFFFFFFFu;
constexpr uint32_t MIN_K = 3;

using blrec::Node;
using Link = blrec::LinkWords;
struct alignas(16) Parked {
    uint32_t to[4];
};

// BL_ERR_INVALID reasons that need no device, behind blgr::refuse: 0 = fine
BL_DEV int refuse(uint32_t k, uint32_t flags, uint64_t n, uint64_t n_unitigs)
{
    if (k < MIN_K) return 5;
    if (flags & ~ONCE) return 6;
    if (n_unitigs > n) return 7;  // (so that (unitig << 1) | orientation fits 32 bits: n < 2^31)
    return 0;
}

// ---- pass 1: key i < n.  end_key holds 2 * n_unitigs words, all END_NONE before the pass.
BL_DEV void end_key_thread(const Node* nodes, const uint64_t* offsets, uint64_t n_unitigs, uint32_t k, uint32_t i, uint32_t* end_key)
{
    const Node nd = nodes[i];
    if (nd.unitig >= n_unitigs) return;
    const uint64_t keys = offsets[nd.unitig + 1] - offsets[nd.unitig] - (k - 1);  // L (wrong offsets: some number, only compared)
    const uint64_t rank = nd.rank_flip >> 1;
    if (rank == 0) end_key[2 * (uint64_t)nd.unitig + 1] = i;         // the - end: the side the walk entered its first key by
    if (rank + 1 == keys) end_key[2 * (uint64_t)nd.unitig] = i;      // the + end: the side the walk leaves its last key by
}

// The four successors of z (rz = rc(z)), as blgr::side_successors finds them, but every one kept: nb[c] = (slot << 1) | entered side of
// the key that is canon(((z << 2) | c) mod 4^k), blgr::LINK_NONE where that is no key.  For k >= 3 the four are different keys.
template <int W>
BL_DEV void side_neighbours(const TableView& t, const K128& z, const K128& rz, uint32_t k, uint32_t nb[4])
{
    const K128 base = blgr::shift_in<W>(z, k);
    const K128 tail = blgr::shift_out(rz);
    K128 q[blgr::NS];
    uint32_t b[blgr::NS];
    uint32_t live = 1u;
    q[0] = base;
    BL_UNROLL
    for (uint32_t c = 0; c < 4; ++c) {
        const K128 top = blgr::top_base<W>(3 - c, k);
        K128 r, f;
        r.lo = top.lo | tail.lo;
        r.hi = top.hi | tail.hi;
        f.lo = base.lo | c;
        f.hi = base.hi;
        q[1 + c].lo = q[1 + c].hi = 0;
        if (blgr::less(r, f)) {  // the reverse form is searched only where it is the smaller one
            q[1 + c] = r;
            live |= 2u << c;
        }
    }
    blgr::lower_bound_group<W>(t, q, live, b);
    // the forward block's four slots and the reverse forms' one each: eight loads at most, issued together
    K128 fk[4], rk[4];
    uint32_t have = 0;
    BL_UNROLL
    for (uint32_t j = 0; j < 4; ++j) {
        fk[j].lo = fk[j].hi = rk[j].lo = rk[j].hi = 0;
        if (b[0] + j < t.n) {
            fk[j] = blgr::load_key<W>(t, b[0] + j);
            have |= 1u << j;
        }
        if (((live >> (1 + j)) & 1u) && b[1 + j] < t.n) {
            rk[j] = blgr::load_key<W>(t, b[1 + j]);
            have |= 16u << j;
        }
    }
    BL_UNROLL
    for (uint32_t c = 0; c < 4; ++c) nb[c] = blgr::LINK_NONE;
    BL_UNROLL
    for (uint32_t j = 0; j < 4; ++j) {
        if (((have >> j) & 1u) && fk[j].hi == base.hi && (fk[j].lo ^ base.lo) < 4) {  // a key of the block base .. base + 3
            const uint32_t c = (uint32_t)(fk[j].lo & 3u);
            BL_UNROLL
            for (uint32_t d = 0; d < 4; ++d)  // (no runtime index into the register array)
                if (d == c) nb[d] = (b[0] + j) << 1;
        }
        if (((have >> (4 + j)) & 1u) && blgr::same(rk[j], q[1 + j])) nb[j] = (b[1 + j] << 1) | 1u;
    }
}

struct EndStats {
    uint32_t degree;        // records of the end before the ONCE filter
    uint32_t kept;          // records behind it
    uint32_t self_reverse;  // records equal to their own reverse
};

// ---- pass 2: end e < 2 * n_unitigs.  parked[e] gets the end's kept `to` words in record order (ascending base c of the side's nibble).
template <int W>
BL_DEV EndStats end_search(const TableView& t, uint32_t k, const Node* nodes, uint64_t n_unitigs, const uint32_t* end_key, uint32_t flags, uint32_t e,
                           Parked& park)
{
    EndStats st{0, 0, 0};
    park.to[0] = park.to[1] = park.to[2] = park.to[3] = 0;
    const uint32_t i = end_key[e];
    if (i == END_NONE || i >= t.n) return st;  // (the second: never)
    const uint32_t flip = nodes[i].rank_flip & 1u;
    const bool left = ((e & 1u) ^ flip) != 0;  // orientation o = (side == left) XOR flip
    const K128 x = blgr::load_key<W>(t, i);
    const K128 rx = blgr::revcomp<W>(x, k);
    uint32_t nb[4];
    if (left) side_neighbours<W>(t, rx, x, k, nb);  // base c prepended to x is successor 3 - c of rc(x)
    else side_neighbours<W>(t, x, rx, k, nb);
    // the nodes of the neighbours: up to four 8-byte loads, issued together
    uint32_t at[4];
    Node nd[4];
    BL_UNROLL
    for (uint32_t c = 0; c < 4; ++c) {
        at[c] = left ? nb[3 - c] : nb[c];
        nd[c].unitig = nd[c].rank_flip = 0;
        if (at[c] != blgr::LINK_NONE) nd[c] = nodes[at[c] >> 1];
    }
    BL_UNROLL
    for (uint32_t c = 0; c < 4; ++c) {
        if (at[c] == blgr::LINK_NONE || nd[c].unitig >= n_unitigs) continue;
        const uint32_t to = (nd[c].unitig << 1) | ((at[c] & 1u) ^ (nd[c].rank_flip & 1u));  // (entered side == right) XOR flip
        ++st.degree;
        st.self_reverse += e == (to ^ 1u);
        if ((flags & ONCE) && e > (to ^ 1u)) continue;
        BL_UNROLL
        for (uint32_t d = 0; d < 4; ++d)
            if (d == st.kept) park.to[d] = to;
        ++st.kept;
    }
    return st;
}

// ---- pass 3: end e < 2 * n_unitigs; offsets: the exclusive sum of the kept degrees (2 * n_unitigs + 1 words, the library's own)
BL_DEV void emit_thread(const uint64_t* offsets, const Parked* parked, uint64_t n_links, uint32_t e, Link* links)
{
    const uint64_t at = offsets[e], n = offsets[e + 1] - at;
    const Parked p = parked[e];
    BL_UNROLL
    for (uint32_t r = 0; r < 4; ++r) {
        if (r < n && at + r < n_links) {  // (the second: always)
            Link l;
            l.from = e;
            l.to = p.to[r];
            links[at + r] = l;
        }
    }
}

}  // namespace bllnk
