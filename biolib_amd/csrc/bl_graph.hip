// bl_graph.hip — the graph on a count table's keys: bl_table_adjacency (one mask byte per key, the links between sides of degree 1, the
// statistics) and bl_table_unitigs (the non-branching paths and cycles as a device-resident batch, with offsets, count sums and the
// place of every key).  The definitions are in include/biolib_amd.h, the per-thread bodies in bl_graph_core.hpp.  Kernels, each one
// thread per key, per side or per state from an uncapped grid (n < 2^31 keys: at most 2^24 workgroups):
//   check_kernel        is every key below 4^k and not above its reverse complement: the first slot that is not (atomicMin)
//   mask_kernel         the hot one: eight neighbour questions per key as two groups of five lockstep searches; the mask byte and, for a
//                       side of degree 1, its neighbour (slot, entered side) — so that the link pass searches nothing
//   link_kernel         per side: the neighbour's mask byte decides whether the arc is a link
//   stats_kernel        arcs, isolated keys, dead-end, branch and linked sides: a wave reduction and five integer atomics per wave
//   label_init_kernel / label_step_kernel   pointer doubling over the 2n states (key, entered side), ping-pong records, one round per
//                       launch; the host stops at the first round in which no state was still on its way
//   cut_kernel          states unfinished after ceil(log2(2n)) + 1 rounds lie on cycles: the smallest slot of each cuts its left link
//   place_kernel        per key: start key, rank, flip and length from the records of its two states; the start flags
//   number_kernel       after rocPRIM's exclusive sum of the flags: bl_unitig_node per key, the string length per unitig
//   emit_kernel         after the exclusive sum of the lengths: every key's last oriented base (a start key: its first k - 1 too), the
//                       count sums by 64-bit integer atomics (order-independent)
//   uniform_kernel      is the result a fixed-length batch (the parser's rule)
// No atomic decides a placement: a rerun is bit-identical.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/biolib_amd.h"
#include "bl_graph_core.hpp"
#include "bl_host.hpp"
#include "bl_lookup_launch.hpp"

static_assert(BL_LINK_NONE == blgr::LINK_NONE, "the header's constant");
static_assert(sizeof(bl_unitig_node) == 8 && sizeof(bl_graph_stats) == 12 * sizeof(uint64_t), "the device words are the caller's");

namespace blgr {

typedef unsigned long long ull;

// the counter block (slot 6, 128 bytes): words 0-4 the key statistics, 5 cycles cut, 6 the longest unitig; then two 32-bit words
constexpr int C_CUTS = 5, C_LONGEST = 6, C_WORDS32 = 16;  // 32-bit word 16: the first bad slot, 17: the round's "a state was live"

__device__ __forceinline__ ull wave_sum(ull v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <int W>
__global__ __launch_bounds__(GTPB) void check_kernel(const TableView t, uint32_t k, uint32_t* first_bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    if (i < t.n && bad_key<W>(t, k, (uint32_t)i)) atomicMin(first_bad, (uint32_t)i);
}

template <int W>
__global__ __launch_bounds__(GTPB) void mask_kernel(const TableView t, uint32_t k, uint8_t* __restrict__ mask, uint2* __restrict__ nbr)
{
    const uint64_t i = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    if (i >= t.n) return;
    uint32_t left, right;
    mask[i] = (uint8_t)mask_thread<W>(t, k, (uint32_t)i, left, right);  // consecutive lanes, consecutive bytes
    if (nbr) nbr[i] = make_uint2(left, right);
}

__global__ __launch_bounds__(GTPB) void link_kernel(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ nbr, uint32_t* __restrict__ links, uint64_t n_sides)
{
    const uint64_t s = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    if (s < n_sides) links[s] = link_thread(mask, nbr, (uint32_t)s);
}

__global__ __launch_bounds__(GTPB) void stats_kernel(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ links, uint64_t n, ull* counters)
{
    const uint64_t i = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    KeyStats st{0, 0, 0, 0, 0};
    if (i < n) st = key_stats(mask, links, (uint32_t)i);
    ull v[5] = {st.arcs, st.isolated, st.dead_end_sides, st.branch_sides, st.linked_sides};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        v[j] = wave_sum(v[j]);
        if ((threadIdx.x & 63) == 0 && v[j]) atomicAdd(&counters[j], v[j]);  // integer sums: the order does not matter
    }
}

__global__ __launch_bounds__(GTPB) void label_init_kernel(const uint32_t* __restrict__ links, Rec* __restrict__ rec, uint64_t n_states)
{
    const uint64_t s = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    if (s < n_states) rec[s] = label_init(links, (uint32_t)s);
}

__global__ __launch_bounds__(GTPB) void label_step_kernel(const Rec* __restrict__ in, Rec* __restrict__ out, uint64_t n_states, uint32_t* any_live)
{
    const uint64_t s = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    bool live = false;
    if (s < n_states) out[s] = label_step(in, (uint32_t)s, live);
    if (__ballot(live) && (threadIdx.x & 63) == 0) atomicOr(any_live, 1u);
}

__global__ __launch_bounds__(GTPB) void cut_kernel(const Rec* __restrict__ rec, uint32_t* links, uint64_t n, ull* counters)
{
    const uint64_t i = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    const ull cut = wave_sum(i < n && cut_cycle_thread(rec, links, (uint32_t)i) ? 1ull : 0ull);
    if ((threadIdx.x & 63) == 0 && cut) atomicAdd(&counters[C_CUTS], cut);
}

__global__ __launch_bounds__(GTPB) void place_kernel(const Rec* __restrict__ rec, uint64_t n, Placed* __restrict__ placed, uint64_t* __restrict__ is_start)
{
    const uint64_t i = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        is_start[n] = 0;  // (the sum behind the last key is the number of unitigs)
        return;
    }
    const Placed pl = place_thread(rec, (uint32_t)i);
    placed[i] = pl;
    is_start[i] = (pl.rank_flip >> 1) == 0;
}

__global__ __launch_bounds__(GTPB) void number_kernel(const Placed* __restrict__ placed, const uint64_t* __restrict__ number, uint64_t n, uint32_t k,
                                                      bl_unitig_node* __restrict__ nodes, uint64_t* __restrict__ lengths, ull* counters)
{
    const uint64_t i = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    ull longest = 0;
    if (i < n) {
        const Placed pl = placed[i];
        bl_unitig_node node;
        node.unitig = (uint32_t)number[pl.start];
        node.rank_flip = pl.rank_flip;
        nodes[i] = node;
        if ((pl.rank_flip >> 1) == 0) {
            lengths[number[i]] = (uint64_t)pl.length + k - 1;
            longest = pl.length;
        }
    } else if (i == n) {
        lengths[number[n]] = 0;  // (the sum behind the last unitig is the number of bases)
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const ull other = __shfl_xor(longest, d, 64);
        longest = other > longest ? other : longest;
    }
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(&counters[C_LONGEST], longest);
}

template <int W>
__global__ __launch_bounds__(GTPB) void emit_kernel(const TableView t, uint32_t k, const bl_unitig_node* __restrict__ nodes, const uint64_t* __restrict__ offsets,
                                                    uint8_t* __restrict__ bases, ull* __restrict__ sums)
{
    const uint64_t i = (uint64_t)blockIdx.x * GTPB + threadIdx.x;
    const bool live = i < t.n;
    bl_unitig_node node{0, 0};
    if (live) node = nodes[i];
    if (live && bases) emit_thread<W>(t, k, (uint32_t)i, node.rank_flip, offsets[node.unitig], bases);
    if (!sums) return;
    // Integer sums: any order.  A wave whose live keys all lie in one unitig (a genome's table is a few very long ones: every wave)
    // adds once; lane 0 is live wherever a lane of the wave is.
    ull count = live ? (ull)t.counts[i] : 0ull;
    const uint32_t first = (uint32_t)__shfl((int)node.unitig, 0, 64);
    if (__ballot(live && node.unitig != first) == 0) {  // (wave-uniform)
        count = wave_sum(count);
        if ((threadIdx.x & 63) == 0 && count) atomicAdd(&sums[first], count);
    } else if (live) {
        atomicAdd(&sums[node.unitig], count);
    }
}

__global__ __launch_bounds__(GTPB) void uniform_kernel(const uint64_t* offsets, uint64_t n_unitigs, uint64_t len, uint32_t* flag)
{
    if (breaks_uniform(offsets, n_unitigs, len, (uint64_t)blockIdx.x * GTPB + threadIdx.x)) atomicOr(flag, 1u);
}

namespace {

using blh::blocks_for;
using blh::exclusive_sum;
using blh::hip_rc;
using blh::invalid;

// what both calls refuse before anything runs
int check_arguments(bl_ctx* ctx, const bl_table* table, uint32_t k)
{
    if (!ctx || !table) return invalid("ctx or table is NULL");
    BLH_OK(blh::table_owner(table->ctx, ctx));
    switch (refuse(k, table->view.key_words, table->view.key_bits, table->view.n)) {
    case 1: return invalid("k must be odd and 1 .. 63 (an even k has k-mers that are their own reverse complement)");
    case 2: return invalid("2k exceeds the table's key_bits");
    case 3: return invalid("a table of one-word keys takes k <= 31");
    case 4: return invalid("the table has 2^31 keys or more: a link word holds a slot and a side");
    default: return BL_OK;
    }
}

// pieces of one scratch allocation, each 256-byte aligned
struct Arena {
    char* base = nullptr;
    size_t used = 0;
    template <typename T>
    T* take(size_t count)
    {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

struct AdjBuffers {
    uint8_t* mask;
    uint32_t* nbr;    // 2n, nullable: no link pass
    uint32_t* links;  // 2n, nullable
};

// the key check, the mask pass, the link pass and the first six statistics (n > 0; the device is set); waits for the stream
template <int W>
int adjacency(const TableView& t, uint32_t k, const AdjBuffers& b, ull* d_counters, bl_graph_stats* stats, hipStream_t s)
{
    const uint64_t n = t.n;
    uint32_t* d_words = reinterpret_cast<uint32_t*>(d_counters) + C_WORDS32;
    BLH_TRY(hipMemsetAsync(d_counters, 0, 8 * sizeof(ull), s));
    BLH_TRY(hipMemsetAsync(d_words, 0xFF, sizeof(uint32_t), s));
    hipLaunchKernelGGL(check_kernel<W>, dim3(blocks_for(n, GTPB)), dim3(GTPB), 0, s, t, k, d_words);
    BLH_TRY(hipGetLastError());
    uint32_t first_bad = 0;
    BLH_TRY(hipMemcpyAsync(&first_bad, d_words, sizeof(first_bad), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (first_bad != LINK_NONE)
        return invalid(("the key at slot " + std::to_string(first_bad) + " has a bit at or above 2k or exceeds its own reverse complement: not a table of canonical k-mers of this k").c_str());
    hipLaunchKernelGGL(mask_kernel<W>, dim3(blocks_for(n, GTPB)), dim3(GTPB), 0, s, t, k, b.mask, reinterpret_cast<uint2*>(b.nbr));
    BLH_TRY(hipGetLastError());
    if (b.links) {
        hipLaunchKernelGGL(link_kernel, dim3(blocks_for(2 * n, GTPB)), dim3(GTPB), 0, s, b.mask, b.nbr, b.links, 2 * n);
        BLH_TRY(hipGetLastError());
    }
    if (stats) {
        hipLaunchKernelGGL(stats_kernel, dim3(blocks_for(n, GTPB)), dim3(GTPB), 0, s, b.mask, b.links, n, d_counters);
        BLH_TRY(hipGetLastError());
        ull host[5] = {};
        BLH_TRY(hipMemcpyAsync(host, d_counters, sizeof(host), hipMemcpyDeviceToHost, s));
        BLH_TRY(hipStreamSynchronize(s));
        stats->n_keys = n;
        stats->n_arcs = host[0];
        stats->n_isolated = host[1];
        stats->n_dead_end_sides = host[2];
        stats->n_branch_sides = host[3];
        stats->n_linked_sides = host[4];
    }
    return BL_OK;
}

// pointer doubling until a round finds every state at its chain's end, at most `rounds` rounds; cur: the records of the last round
int label(const uint32_t* links, Rec*& cur, Rec*& nxt, uint64_t n_states, uint32_t rounds, uint32_t* d_flag, bool& settled, hipStream_t s)
{
    hipLaunchKernelGGL(label_init_kernel, dim3(blocks_for(n_states, GTPB)), dim3(GTPB), 0, s, links, cur, n_states);
    BLH_TRY(hipGetLastError());
    settled = false;
    for (uint32_t r = 0; r < rounds && !settled; ++r) {
        BLH_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(label_step_kernel, dim3(blocks_for(n_states, GTPB)), dim3(GTPB), 0, s, cur, nxt, n_states, d_flag);
        BLH_TRY(hipGetLastError());
        uint32_t any = 0;
        BLH_TRY(hipMemcpyAsync(&any, d_flag, sizeof(any), hipMemcpyDeviceToHost, s));
        BLH_TRY(hipStreamSynchronize(s));
        Rec* swap = cur;
        cur = nxt;
        nxt = swap;
        settled = any == 0;
    }
    return BL_OK;
}

// the empty table's result: a valid batch of 0 bases and 0 sequences, as bl_batch_select makes one
int empty_result(bl_ctx* ctx, bl_batch** out, uint64_t* d_out_offsets, hipStream_t s)
{
    if (d_out_offsets) BLH_TRY(hipMemsetAsync(d_out_offsets, 0, sizeof(uint64_t), s));
    if (out) {
        blh::Pooled<uint8_t> d_bases(ctx, 64);
        blh::Pooled<uint64_t> d_offs(ctx, sizeof(uint64_t));
        if (!d_bases || !d_offs) return hip_rc(hipErrorOutOfMemory);
        BLH_TRY(hipMemsetAsync(d_bases.get(), 0, 64, s));
        BLH_TRY(hipMemsetAsync(d_offs.get(), 0, sizeof(uint64_t), s));
        BLH_TRY(hipStreamSynchronize(s));
        return bl_batch_adopt_device(ctx, d_bases.release(), 0, d_offs.release(), 0, 0, out);  // takes ownership of both
    }
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}

template <int W>
int unitigs(bl_ctx* ctx, const bl_table* table, uint32_t k, bl_batch** out, uint64_t* d_out_offsets, uint64_t* d_count_sums, bl_unitig_node* d_nodes,
            uint64_t* n_unitigs_out, uint64_t* n_bases_out, bl_graph_stats* stats, hipStream_t s)
{
    const TableView& t = table->view;
    const uint64_t n = t.n;
    Arena a;  // first without a base: the size
    a.take<uint8_t>(n);
    a.take<uint32_t>(2 * n);
    a.take<uint32_t>(2 * n);
    a.take<Rec>(2 * n);
    a.take<Rec>(2 * n);
    a.take<Placed>(n);
    a.take<uint64_t>(4 * (n + 1));
    if (!d_nodes) a.take<bl_unitig_node>(n);
    a.base = static_cast<char*>(bl_ctx_scratch(ctx, 4, a.used));
    if (!a.base) return bl_set_error(BL_ERR_OOM, "scratch allocation failed (about 133 bytes per key)");
    a.used = 0;
    AdjBuffers b;
    b.mask = a.take<uint8_t>(n);
    b.nbr = a.take<uint32_t>(2 * n);
    b.links = a.take<uint32_t>(2 * n);
    Rec* cur = a.take<Rec>(2 * n);
    Rec* nxt = a.take<Rec>(2 * n);
    Placed* placed = a.take<Placed>(n);
    uint64_t* is_start = a.take<uint64_t>(4 * (n + 1));
    uint64_t* number = is_start + (n + 1);
    uint64_t* lengths = number + (n + 1);
    uint64_t* offsets = lengths + (n + 1);
    bl_unitig_node* nodes = d_nodes ? d_nodes : a.take<bl_unitig_node>(n);
    ull* d_counters = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 128));
    if (!d_counters) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    uint32_t* d_flag = reinterpret_cast<uint32_t*>(d_counters) + C_WORDS32 + 1;

    BLH_OK(adjacency<W>(t, k, b, d_counters, stats, s));

    // labelling; where states are still on their way after the bound they lie on cycles: cut each at its smallest slot and label again
    const uint32_t bound = max_rounds((uint32_t)n);
    bool settled = false;
    ull cuts = 0;
    BLH_OK(label(b.links, cur, nxt, 2 * n, bound, d_flag, settled, s));
    if (!settled) {
        hipLaunchKernelGGL(cut_kernel, dim3(blocks_for(n, GTPB)), dim3(GTPB), 0, s, cur, b.links, n, d_counters);
        BLH_TRY(hipGetLastError());
        BLH_TRY(hipMemcpyAsync(&cuts, d_counters + C_CUTS, sizeof(cuts), hipMemcpyDeviceToHost, s));
        BLH_TRY(hipStreamSynchronize(s));
        if (cuts) {
            BLH_OK(label(b.links, cur, nxt, 2 * n, bound + 1, d_flag, settled, s));
            if (!settled) return bl_set_error(BL_ERR_INTERNAL, "states are still on their way after every cycle was cut");
        }
    }

    hipLaunchKernelGGL(place_kernel, dim3(blocks_for(n + 1, GTPB)), dim3(GTPB), 0, s, cur, n, placed, is_start);
    BLH_TRY(hipGetLastError());
    BLH_OK(exclusive_sum(ctx, is_start, number, (size_t)(n + 1), s));
    hipLaunchKernelGGL(number_kernel, dim3(blocks_for(n + 1, GTPB)), dim3(GTPB), 0, s, placed, number, n, k, nodes, lengths, d_counters);
    BLH_TRY(hipGetLastError());
    ull n_unitigs = 0, longest = 0;
    BLH_TRY(hipMemcpyAsync(&n_unitigs, number + n, sizeof(n_unitigs), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipMemcpyAsync(&longest, d_counters + C_LONGEST, sizeof(longest), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    uint64_t total = 0;
    BLH_OK(blh::exclusive_sum_total(ctx, lengths, offsets, (size_t)(n_unitigs + 1), s, &total));
    if (stats) {
        stats->n_unitigs = n_unitigs;
        stats->n_cycles = cuts;
        stats->longest_unitig = longest;
    }
    if (d_out_offsets) BLH_TRY(hipMemcpyAsync(d_out_offsets, offsets, (size_t)(n_unitigs + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));

    blh::Pooled<uint8_t> d_bases;  // (both stay empty without `out`)
    blh::Pooled<uint64_t> d_offs;
    if (out) {
        d_bases = blh::Pooled<uint8_t>(ctx, (size_t)total + 64);
        d_offs = blh::Pooled<uint64_t>(ctx, (size_t)(n_unitigs + 1) * sizeof(uint64_t));
        if (!d_bases || !d_offs) return bl_set_error(BL_ERR_OOM, "device allocation failed (batch)");
        BLH_TRY(hipMemsetAsync(d_bases.get() + total, 0, 64, s));  // the zero padding every batch has behind its bases
        BLH_TRY(hipMemcpyAsync(d_offs.get(), offsets, (size_t)(n_unitigs + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    }
    if (d_count_sums) BLH_TRY(hipMemsetAsync(d_count_sums, 0, (size_t)n_unitigs * sizeof(uint64_t), s));
    if (out || d_count_sums) {
        hipLaunchKernelGGL(emit_kernel<W>, dim3(blocks_for(n, GTPB)), dim3(GTPB), 0, s, t, k, nodes, offsets, d_bases.get(), reinterpret_cast<ull*>(d_count_sums));
        BLH_TRY(hipGetLastError());
    }
    // unitigs of one length make a fixed-length batch (the parser's rule), any other result carries start bits
    uint64_t fixed_len = out && n_unitigs > 1 && total % n_unitigs == 0 ? total / n_unitigs : 0;
    uint32_t ragged = 0;
    if (fixed_len) {
        BLH_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(uniform_kernel, dim3(blocks_for(n_unitigs, GTPB)), dim3(GTPB), 0, s, offsets, (uint64_t)n_unitigs, fixed_len, d_flag);
        BLH_TRY(hipGetLastError());
        BLH_TRY(hipMemcpyAsync(&ragged, d_flag, sizeof(ragged), hipMemcpyDeviceToHost, s));
    }
    BLH_TRY(hipStreamSynchronize(s));
    if (ragged) fixed_len = 0;
    if (out) {
        BLH_OK(bl_batch_adopt_device(ctx, d_bases.release(), total, d_offs.release(), n_unitigs, fixed_len, out));  // takes ownership of both
    }
    if (n_unitigs_out) *n_unitigs_out = n_unitigs;
    if (n_bases_out) *n_bases_out = total;
    return BL_OK;
}

}  // namespace

}  // namespace blgr

extern "C" int bl_table_adjacency(bl_ctx* ctx, const bl_table* table, uint32_t k, uint8_t* d_mask, uint32_t* d_links, bl_graph_stats* stats)
{
    using namespace blgr;
    BLH_OK(check_arguments(ctx, table, k));
    if (stats) *stats = bl_graph_stats{};
    const TableView& t = table->view;
    const uint64_t n = t.n;
    if (n == 0) return BL_OK;
    if (!d_mask) return invalid("d_mask is NULL");
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    // slot 4: the one neighbour of every side of degree 1 and, where the caller takes no links but the statistics, the links
    const bool linking = d_links || stats;
    Arena a;
    uint32_t* nbr = nullptr;
    uint32_t* links = d_links;
    if (linking) {
        const size_t words = 2 * n;
        a.take<uint32_t>(words);
        if (!d_links) a.take<uint32_t>(words);
        a.base = static_cast<char*>(bl_ctx_scratch(ctx, 4, a.used));
        if (!a.base) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        a.used = 0;
        nbr = a.take<uint32_t>(words);
        if (!d_links) links = a.take<uint32_t>(words);
    }
    ull* d_counters = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 128));
    if (!d_counters) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    const AdjBuffers b{d_mask, nbr, links};
    BLH_OK(t.key_words == 2 ? adjacency<2>(t, k, b, d_counters, stats, s) : adjacency<1>(t, k, b, d_counters, stats, s));
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}

extern "C" int bl_table_unitigs(bl_ctx* ctx, const bl_table* table, uint32_t k, bl_batch** out, uint64_t* d_out_offsets, uint64_t* d_count_sums,
                                bl_unitig_node* d_nodes, uint64_t* n_unitigs, uint64_t* n_bases, bl_graph_stats* stats)
{
    using namespace blgr;
    if (out) *out = nullptr;
    BLH_OK(check_arguments(ctx, table, k));
    if (stats) *stats = bl_graph_stats{};
    if (n_unitigs) *n_unitigs = 0;
    if (n_bases) *n_bases = 0;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    if (table->view.n == 0) return empty_result(ctx, out, d_out_offsets, s);
    return table->view.key_words == 2 ? unitigs<2>(ctx, table, k, out, d_out_offsets, d_count_sums, d_nodes, n_unitigs, n_bases, stats, s)
                                      : unitigs<1>(ctx, table, k, out, d_out_offsets, d_count_sums, d_nodes, n_unitigs, n_bases, stats, s);
}
