// bl_clean.hip — cleaning the compacted graph: bl_unitigs_mark (which unitigs are tips, islands or the lesser branches of bubbles, decided
// from the link records alone) and bl_table_remove_unitigs (the table without the marked unitigs' keys, an ordinary table again).  The
// definitions are in include/biolib_amd.h, the per-thread bodies in bl_clean_core.hpp.  Kernels, every grid sized by the work:
//   mark_kernel     one lane per unitig, no stride loop, no LDS: the chain of dependent gathers of mark_thread; writes the mark byte and
//                   adds the statistics (a wave reduction and five integer atomics per wave that marked anything, order-independent; the
//                   counters are striped over STRIPES cache lines by workgroup, since on a table of islands every wave adds)
//   count_kernel    one wave per tile of 64 * ROWS keys: the kept keys of the tile (ballots), one word per tile
//   write_kernel    behind rocPRIM's exclusive sum of the tile totals: the same ballots place the kept keys and counts
// No atomic decides a mark or a placement: a rerun is bit-identical.
#include <hip/hip_runtime.h>

#include "../../include/biolib_amd.h"
#include "bl_clean_core.hpp"
#include "bl_host.hpp"
#include "bl_lookup_launch.hpp"

static_assert(sizeof(bl_clean_rule) == sizeof(blcl::Rule) && sizeof(bl_clean_rule) == 56 && sizeof(bl_clean_stats) == 8 * sizeof(uint64_t), "the header's structs");
static_assert((uint32_t)BL_CLEAN_TIPS == blcl::TIPS && (uint32_t)BL_CLEAN_ISOLATED == blcl::ISOLATED && (uint32_t)BL_CLEAN_BUBBLES == blcl::BUBBLES &&
                  BL_MARK_KEEP == blcl::KEEP && BL_MARK_TIP == blcl::TIP && BL_MARK_ISOLATED == blcl::ISLAND && BL_MARK_BUBBLE == blcl::BUBBLE,
              "the header's constants");
static_assert(sizeof(bl_unitig_link) == sizeof(bllnk::Link) && sizeof(bl_unitig_node) == sizeof(bllnk::Node), "the device words are the caller's");

namespace blcl {

typedef unsigned long long ull;

__device__ __forceinline__ ull wave_sum(ull v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// counters: 0 tips, 1 islands, 2 bubble branches, 3 their keys, 4 their count sums — STRIPES copies of STRIPE_WORDS words (128 bytes, a
// cache line of their own), the workgroup's number picks one, the host adds them up
constexpr int STRIPES = 64, STRIPE_WORDS = 16;

__global__ __launch_bounds__(CTPB) void mark_kernel(const Graph g, const Rule r, uint8_t* __restrict__ marks, ull* counters)
{
    const uint64_t u = (uint64_t)blockIdx.x * CTPB + threadIdx.x;
    uint8_t m = KEEP;
    uint64_t keys = 0, sum = 0;
    if (u < g.n_unitigs) {
        m = mark_thread(g, r, u, keys, sum);
        marks[u] = m;
    }
    if (__ballot(m != KEEP) == 0) return;  // (wave-uniform) nearly every wave of a genome's graph
    ull v[5] = {(ull)(m == TIP), (ull)(m == ISLAND), (ull)(m == BUBBLE), m != KEEP ? (ull)keys : 0ull, m != KEEP ? (ull)sum : 0ull};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        v[j] = wave_sum(v[j]);
        if ((threadIdx.x & 63) == 0 && v[j]) atomicAdd(&counters[(blockIdx.x % STRIPES) * STRIPE_WORDS + j], v[j]);  // integer sums: the order does not matter
    }
}

template <int R>
__global__ __launch_bounds__(CTPB) void count_kernel(const bllnk::Node* __restrict__ nodes, const uint8_t* __restrict__ marks, uint64_t n_unitigs, uint64_t n,
                                                     uint64_t n_tiles, uint64_t* __restrict__ totals)
{
    const int lane = threadIdx.x & 63;
    const uint64_t tile = (uint64_t)blockIdx.x * (CTPB / 64) + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;  // (wave-uniform)
    bool keep[R];
#pragma unroll
    for (int row = 0; row < R; ++row) {  // R node loads, then R mark bytes, in flight together
        const uint64_t i = tile_slot<R>(tile, row, lane);
        keep[row] = i < n && keeps(nodes, marks, n_unitigs, i);
    }
    uint64_t total = 0;
#pragma unroll
    for (int row = 0; row < R; ++row) total += (uint64_t)__popcll(__ballot(keep[row]));
    if (lane == 0) totals[tile] = total;
}

template <int W, int R>
__global__ __launch_bounds__(CTPB) void write_kernel(const bllnk::Node* __restrict__ nodes, const uint8_t* __restrict__ marks, uint64_t n_unitigs,
                                                     const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, uint64_t n, uint64_t n_tiles,
                                                     const uint64_t* __restrict__ bases, uint64_t n_out, uint64_t* __restrict__ out_keys,
                                                     uint32_t* __restrict__ out_counts)
{
    const int lane = threadIdx.x & 63;
    const uint64_t tile = (uint64_t)blockIdx.x * (CTPB / 64) + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    bool keep[R];
#pragma unroll
    for (int row = 0; row < R; ++row) {
        const uint64_t i = tile_slot<R>(tile, row, lane);
        keep[row] = i < n && keeps(nodes, marks, n_unitigs, i);
    }
    uint64_t base = bases[tile];
#pragma unroll
    for (int row = 0; row < R; ++row) {
        const uint64_t ballot = __ballot(keep[row]);
        const uint64_t to = base + rank_in_row(ballot, lane);
        // (the count pass made the same decisions over the same data: to < n_out.  Checked all the same)
        if (keep[row] && to < n_out) move_key<W>(keys, counts, tile_slot<R>(tile, row, lane), out_keys, out_counts, to);
        base += (uint64_t)__popcll(ballot);
    }
}

namespace {

using blh::blocks_for;
using blh::hip_rc;
using blh::invalid;

template <int W>
int remove_marked(bl_ctx* ctx, const bl_table* table, const bllnk::Node* nodes, const uint8_t* marks, uint64_t n_unitigs, bl_table** out, uint64_t* n_removed)
{
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    const uint64_t n = table->view.n;
    const uint64_t n_tiles = tiles_of<ROWS>(n);
    uint64_t n_out = 0;
    uint64_t* totals = nullptr;
    uint64_t* bases = nullptr;
    if (n_tiles) {
        // slot 4: the tile totals (one word more: 0) and their exclusive sums (the last: the number of kept keys)
        totals = static_cast<uint64_t*>(bl_ctx_scratch(ctx, 4, 2 * (n_tiles + 1) * sizeof(uint64_t)));
        if (!totals) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        bases = totals + n_tiles + 1;
        BLH_TRY(hipMemsetAsync(totals + n_tiles, 0, sizeof(uint64_t), s));
        hipLaunchKernelGGL(count_kernel<ROWS>, dim3(blocks_for(n_tiles * 64, CTPB)), dim3(CTPB), 0, s, nodes, marks, n_unitigs, n, n_tiles, totals);
        BLH_TRY(hipGetLastError());
        BLH_OK(blh::exclusive_sum_total(ctx, totals, bases, (size_t)(n_tiles + 1), s, &n_out));
        if (n_out > n) return bl_set_error(BL_ERR_INTERNAL, "the count pass kept more keys than the table holds");
    }
    bl_table* t = nullptr;
    BLH_OK(bllk::new_table(ctx, table->view.key_words, table->view.key_bits, n_out, &t));
    hipError_t e = hipSuccess;
    if (n_out) {
        hipLaunchKernelGGL((write_kernel<W, ROWS>), dim3(blocks_for(n_tiles * 64, CTPB)), dim3(CTPB), 0, s, nodes, marks, n_unitigs, table->view.keys,
                           table->view.counts, n, n_tiles, bases, (uint64_t)n_out, const_cast<uint64_t*>(t->view.keys), const_cast<uint32_t*>(t->view.counts));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = bllk::finish_table(ctx, t, s);
    if (e != hipSuccess) {
        bllk::free_table(t);
        return hip_rc(e);
    }
    *out = t;
    if (n_removed) *n_removed = n - n_out;
    return BL_OK;
}

}  // namespace

}  // namespace blcl

extern "C" int bl_unitigs_mark(bl_ctx* ctx, const uint64_t* d_unitig_offsets, const uint64_t* d_count_sums, uint64_t n_unitigs, const uint64_t* d_link_offsets,
                               const bl_unitig_link* d_links, uint64_t n_links, const bl_clean_rule* rule, uint8_t* d_marks, bl_clean_stats* stats)
{
    using namespace blcl;
    if (stats) *stats = bl_clean_stats{};
    if (!ctx || !rule) return invalid("ctx or rule is NULL");
    switch (refuse(rule->flags, rule->k, rule->reserved, n_unitigs)) {
    case 1: return invalid("bl_clean_rule: k must be odd and 3 .. 63");
    case 2: return invalid("bl_clean_rule: unknown flag bits (BL_CLEAN_TIPS | BL_CLEAN_ISOLATED | BL_CLEAN_BUBBLES)");
    case 3: return invalid("bl_clean_rule: reserved must be 0");
    case 4: return invalid("n_unitigs is 2^31 or more: an end number holds a unitig and an orientation");
    default: break;
    }
    if (n_unitigs && (!d_unitig_offsets || !d_count_sums || !d_link_offsets || !d_marks))
        return invalid("d_unitig_offsets, d_count_sums, d_link_offsets or d_marks is NULL with n_unitigs > 0");
    if (n_links && !d_links) return invalid("d_links is NULL with n_links > 0");
    if (stats) stats->n_unitigs = n_unitigs;
    if (n_unitigs == 0) return BL_OK;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    ull* d_counters = static_cast<ull*>(bl_ctx_scratch(ctx, 6, STRIPES * STRIPE_WORDS * sizeof(ull)));
    if (!d_counters) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    Graph g{d_unitig_offsets, d_count_sums, d_link_offsets, reinterpret_cast<const bllnk::Link*>(d_links), n_unitigs, n_links};
    Rule r{rule->flags, rule->k, rule->max_tip_keys, rule->max_isolated_keys, rule->max_isolated_mean, rule->max_bubble_keys, rule->max_bubble_diff, 0};
    ull stripes[STRIPES * STRIPE_WORDS] = {}, host[5] = {};
    BLH_TRY(hipMemsetAsync(d_counters, 0, sizeof(stripes), s));
    hipLaunchKernelGGL(mark_kernel, dim3(blocks_for(n_unitigs, CTPB)), dim3(CTPB), 0, s, g, r, d_marks, d_counters);
    BLH_TRY(hipGetLastError());
    BLH_TRY(hipMemcpyAsync(stripes, d_counters, sizeof(stripes), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < STRIPES; ++i)
        for (int j = 0; j < 5; ++j) host[j] += stripes[i * STRIPE_WORDS + j];
    if (stats) {
        stats->n_tips = host[0];
        stats->n_isolated = host[1];
        stats->n_bubbles = host[2];
        stats->n_keys_marked = host[3];
        stats->count_sum_marked = host[4];
    }
    return BL_OK;
}

extern "C" int bl_table_remove_unitigs(bl_ctx* ctx, const bl_table* table, const bl_unitig_node* d_nodes, const uint8_t* d_marks, uint64_t n_unitigs, bl_table** out,
                                       uint64_t* n_removed)
{
    using namespace blcl;
    if (out) *out = nullptr;
    if (n_removed) *n_removed = 0;
    if (!ctx || !table) return invalid("ctx or table is NULL");
    if (!out) return invalid("out is NULL");
    BLH_OK(blh::table_owner(table->ctx, ctx));
    if (table->view.n && (!d_nodes || !d_marks)) return invalid("d_nodes or d_marks is NULL on a table that is not empty");
    const bllnk::Node* nodes = reinterpret_cast<const bllnk::Node*>(d_nodes);
    return table->view.key_words == 2 ? remove_marked<2>(ctx, table, nodes, d_marks, n_unitigs, out, n_removed)
                                      : remove_marked<1>(ctx, table, nodes, d_marks, n_unitigs, out, n_removed);
}
