// bl_links.hip — the compacted graph leaves as a graph: bl_unitig_links (the edges between unitig ends as a CSR pair) and
// bl_unitigs_format_gfa (the unitigs and those edges as GFA 1 text made on the device, downloaded by bl_text_write).  The definitions are
// in include/biolib_amd.h, the per-thread bodies in bl_links_core.hpp and bl_gfa_core.hpp.  Kernels, every grid sized by the work:
//   end_key_kernel      per key: an end key writes its slot into end_key[2u + o]
//   end_search_kernel   the hot one, one lane per end: the end side's four successors by the lockstep lower-bound searches of the mask
//                       pass, one 8-byte node load per neighbour; parks the kept `to` words (16 bytes per end), writes the degree and
//                       adds the statistics (a wave reduction and four integer atomics per wave: order-independent)
//   link_emit_kernel    behind rocPRIM's exclusive sum of the degrees: the parked words become records
//   line_length_kernel  per GFA line: its byte count
//   gfa_kernel          output-centric like bl_format.hip's format_kernel: a lane produces CHUNKS_PER_LANE 16-byte chunks with one 16-byte
//                       store each; the wave finds its first line with the 64-ary search: ballots and shuffles, no LDS, no barrier
// No atomic decides a placement: a rerun is bit-identical.
#include <hip/hip_runtime.h>

#include "../../include/biolib_amd.h"
#include "bl_gfa_core.hpp"
#include "bl_host.hpp"
#include "bl_links_core.hpp"
#include "bl_lookup_launch.hpp"

static_assert(sizeof(bl_unitig_link) == sizeof(bllnk::Link) && sizeof(bl_unitig_link) == sizeof(blgfa::LinkWords) && sizeof(bl_unitig_node) == sizeof(bllnk::Node),
              "the device words are the caller's");
static_assert(sizeof(bl_link_stats) == 8 * sizeof(uint64_t) && sizeof(bl_gfa_rule) == 40,"the header's structs");
static_assert((uint32_t)BL_LINKS_ONCE == bllnk::ONCE && (uint32_t)BL_GFA_NO_HEADER == blgfa::NO_HEADER, "the header's constants");

namespace bllnk {

typedef unsigned long long ull;

__device__ __forceinline__ ull wave_sum(ull v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(LTPB) void end_key_kernel(const Node* __restrict__ nodes, const uint64_t* __restrict__ offsets, uint64_t n_unitigs, uint32_t k, uint64_t n,
                                                       uint32_t* __restrict__ end_key)
{
    const uint64_t i = (uint64_t)blockIdx.x * LTPB + threadIdx.x;
    if (i < n) end_key_thread(nodes, offsets, n_unitigs, k, (uint32_t)i, end_key);
}

// counters: 0 self-reverse records, 1 dead ends, 2 branch ends, 3 records before the filter
template <int W>
__global__ __launch_bounds__(LTPB) void end_search_kernel(const TableView t, uint32_t k, const Node* __restrict__ nodes, uint64_t n_unitigs,
                                                          const uint32_t* __restrict__ end_key, uint32_t flags, uint64_t* __restrict__ degree,
                                                          Parked* __restrict__ parked, ull* counters)
{
    const uint64_t e = (uint64_t)blockIdx.x * LTPB + threadIdx.x;
    const uint64_t n_ends = 2 * n_unitigs;
    EndStats st{0, 0, 0};
    if (e < n_ends) {
        Parked park;
        st = end_search<W>(t, k, nodes, n_unitigs, end_key, flags, (uint32_t)e, park);
        parked[e] = park;  // one 16-byte store
        degree[e] = st.kept;
    } else if (e == n_ends) {
        degree[e] = 0;  // (the sum behind the last end is the number of records)
    }
    ull v[4] = {st.self_reverse, (ull)(e < n_ends && st.degree == 0), (ull)(st.degree >= 2), st.degree};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = wave_sum(v[j]);
        if ((threadIdx.x & 63) == 0 && v[j]) atomicAdd(&counters[j], v[j]);  // integer sums: the order does not matter
    }
}

__global__ __launch_bounds__(LTPB) void link_emit_kernel(const uint64_t* __restrict__ offsets, const Parked* __restrict__ parked, uint64_t n_ends, uint64_t n_links,
                                                         Link* __restrict__ links)
{
    const uint64_t e = (uint64_t)blockIdx.x * LTPB + threadIdx.x;
    if (e < n_ends) emit_thread(offsets, parked, n_links, (uint32_t)e, links);
}

namespace {

using blh::blocks_for;
using blh::exclusive_sum;
using blh::invalid;

size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

}  // namespace bllnk

extern "C" int bl_unitig_links(bl_ctx* ctx, const bl_table* table, uint32_t k, const bl_unitig_node* d_nodes, const uint64_t* d_unitig_offsets, uint64_t n_unitigs,
                               uint32_t flags, uint64_t* d_link_offsets, bl_unitig_link* d_links, uint64_t capacity, uint64_t* n_links, bl_link_stats* stats)
{
    using namespace bllnk;
    if (n_links) *n_links = 0;
    if (!ctx || !table) return invalid("ctx or table is NULL");
    BLH_OK(blh::table_owner(table->ctx, ctx));
    const TableView& t = table->view;
    const uint64_t n = t.n;
    switch (blgr::refuse(k, t.key_words, t.key_bits, n)) {
    case 1: return invalid("k must be odd and 3 .. 63");
    case 2: return invalid("2k exceeds the table's key_bits");
    case 3: return invalid("a table of one-word keys takes k <= 31");
    case 4: return invalid("the table has 2^31 keys or more: a link word holds a unitig and an orientation");
    default: break;
    }
    switch (refuse(k, flags, n, n_unitigs)) {
    case 5: return invalid("k = 1 is refused: two bases can lead to one key there, so link records would not be unique (k must be odd and 3 .. 63)");
    case 6: return invalid("unknown flag bits (BL_LINKS_ONCE is the only flag)");
    case 7: return invalid("n_unitigs exceeds the table's number of keys");
    default: break;
    }
    if (n && (!d_nodes || !d_unitig_offsets)) return invalid("d_nodes or d_unitig_offsets is NULL on a table that is not empty");
    if (stats) *stats = bl_link_stats{};
    const uint64_t n_ends = 2 * n_unitigs;
    if (stats) stats->n_ends = n_ends;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    if (n_ends == 0) {
        if (d_link_offsets) BLH_TRY(hipMemsetAsync(d_link_offsets, 0, sizeof(uint64_t), s));
        BLH_TRY(hipStreamSynchronize(s));
        return BL_OK;
    }
    // slot 4: the end keys, the degrees, their sums and the parked words: 36 bytes per end
    const size_t b_keys = aligned(n_ends * sizeof(uint32_t)), b_sum = aligned((n_ends + 1) * sizeof(uint64_t)), b_park = aligned(n_ends * sizeof(Parked));
    char* arena = static_cast<char*>(bl_ctx_scratch(ctx, 4, b_keys + 2 * b_sum + b_park));
    ull* d_counters = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 128));
    if (!arena || !d_counters) return bl_set_error(BL_ERR_OOM, "scratch allocation failed (36 bytes per unitig end)");
    uint32_t* end_key = reinterpret_cast<uint32_t*>(arena);
    uint64_t* degree = reinterpret_cast<uint64_t*>(arena + b_keys);
    uint64_t* offsets = reinterpret_cast<uint64_t*>(arena + b_keys + b_sum);
    Parked* parked = reinterpret_cast<Parked*>(arena + b_keys + 2 * b_sum);
    const Node* nodes = reinterpret_cast<const Node*>(d_nodes);

    BLH_TRY(hipMemsetAsync(end_key, 0xFF, n_ends * sizeof(uint32_t), s));
    BLH_TRY(hipMemsetAsync(d_counters, 0, 4 * sizeof(ull), s));
    hipLaunchKernelGGL(end_key_kernel, dim3(blocks_for(n, LTPB)), dim3(LTPB), 0, s, nodes, d_unitig_offsets, n_unitigs, k, n, end_key);
    BLH_TRY(hipGetLastError());
    if (t.key_words == 2)
        hipLaunchKernelGGL(end_search_kernel<2>, dim3(blocks_for(n_ends + 1, LTPB)), dim3(LTPB), 0, s, t, k, nodes, n_unitigs, end_key, flags, degree, parked, d_counters);
    else
        hipLaunchKernelGGL(end_search_kernel<1>, dim3(blocks_for(n_ends + 1, LTPB)), dim3(LTPB), 0, s, t, k, nodes, n_unitigs, end_key, flags, degree, parked, d_counters);
    BLH_TRY(hipGetLastError());
    BLH_OK(exclusive_sum(ctx, degree, offsets, (size_t)(n_ends + 1), s));
    ull total = 0, host[4] = {};
    BLH_TRY(hipMemcpyAsync(&total, offsets + n_ends, sizeof(total), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipMemcpyAsync(host, d_counters, sizeof(host), hipMemcpyDeviceToHost, s));
    if (d_link_offsets) BLH_TRY(hipMemcpyAsync(d_link_offsets, offsets, (size_t)(n_ends + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (n_links) *n_links = total;
    if (stats) {
        stats->n_links = total;
        stats->n_self_reverse = host[0];
        stats->n_dead_ends = host[1];
        stats->n_branch_ends = host[2];
    }
    if (!d_links) return BL_OK;  // sizing only
    if (capacity < total) return bl_set_error(BL_ERR_CAPACITY, "bl_unitig_links: d_links is smaller than the records (*n_links says how many there are)");
    if (total == 0) return BL_OK;
    hipLaunchKernelGGL(link_emit_kernel, dim3(blocks_for(n_ends, LTPB)), dim3(LTPB), 0, s, offsets, parked, n_ends, (uint64_t)total, reinterpret_cast<Link*>(d_links));
    BLH_TRY(hipGetLastError());
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}

namespace blgfa {

__global__ __launch_bounds__(TPB) void line_length_kernel(const GfaParams p) { line_length(p, (uint64_t)blockIdx.x * TPB + threadIdx.x); }

__global__ __launch_bounds__(TPB) void gfa_kernel(const GfaParams p)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    const uint64_t x_first = blsel::wave_first_byte(wave);
    if (x_first >= p.total) return;  // (wave-uniform, as everything up to the chunks)
    // the wave's first line: 64-ary search with all lanes
    uint64_t lo = 0, e = p.n_lines;
    while (e - lo > 1) blsel::kary_narrow(lo, e, (uint64_t)__popcll(__ballot(blsel::kary_probe(p.line_off, lo, e, lane, x_first))));
    // the next 64 offsets in registers; do they reach the wave's last byte?
    const uint64_t x_last = wave_last_byte(p, wave);
    const uint64_t o = lane_offset(p, lo, lane), o_lo = p.line_off[lo];
    const int inside = __popcll(__ballot(o <= x_last));
    const bool in_registers = inside < 64;
    const uint64_t hi = in_registers ? lo + (uint64_t)inside : blsel::seq_of(p.line_off, x_last, lo + 64, p.n_lines - 1);

    // the line that holds output byte x (wave-uniform control flow: every lane takes part in the shuffles)
    auto locate = [&](uint64_t x) {
        LineAt s;
        if (in_registers) {
            uint32_t cnt = 0;
#pragma unroll
            for (uint32_t step = 32; step >= 1; step >>= 1) blsel::count_step(cnt, step, __shfl(o, (int)(cnt + step - 1), 64), x);
            const uint64_t before = __shfl(o, (int)cnt - 1, 64);  // (cnt = 0: any lane's, not used)
            s.j = lo + cnt;
            s.begin = cnt ? before : o_lo;
            s.end = __shfl(o, (int)cnt, 64);
        } else {
            s = line_from_memory(p, x, lo, hi);
        }
        return s;
    };

    // Where every chunk lies: one that is a window issues its loads, every other one is assembled and stored at once, so that a chunk
    // finds its line only once; the windows are shifted and stored behind, their loads all in flight by then.
    uint32_t v[CHUNKS_PER_LANE][5];
    uint32_t one_window = 0, shifts = 0;
#pragma unroll
    for (int u = 0; u < CHUNKS_PER_LANE; ++u) {
        const uint64_t x0 = blsel::chunk_first_byte(wave, u, lane);
        const bool live = x0 < p.total;
        const LineAt s = locate(live ? x0 : p.total - 1);
        if (live) {
            uint64_t vsrc;
            if (x0 + CHUNK <= s.end && chunk_window(p, s.j, x0 - s.begin, vsrc)) {
                blsel::window_load(p.bases, vsrc, v[u]);
                one_window |= 1u << u;
                shifts |= (uint32_t)(vsrc & 3u) << (2 * u);
            } else {
                uint32_t w[4];
                gfa_pieces(p, x0, s, w);
                blfmt::store_chunk(p.out, p.total, x0, w);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CHUNKS_PER_LANE; ++u) {
        if ((one_window >> u) & 1u) {
            uint32_t w[4];
            blsel::window_shift(v[u], (shifts >> (2 * u)) & 3u, w);
            blfmt::store_chunk(p.out, p.total, blsel::chunk_first_byte(wave, u, lane), w);
        }
    }
}

namespace {

using blh::blocks_for;
using blh::invalid;
using blh::terminated_length;

}  // namespace

}  // namespace blgfa

extern "C" int bl_unitigs_format_gfa(bl_ctx* ctx, const bl_batch* unitigs, const uint64_t* d_unitig_offsets, uint64_t n_unitigs, const uint64_t* d_count_sums,
                                     const bl_unitig_link* d_links, uint64_t n_links, const bl_gfa_rule* rule, uint8_t* d_out, uint64_t capacity, uint64_t* n_bytes)
{
    using namespace blgfa;
    if (n_bytes) *n_bytes = 0;
    if (!ctx || !unitigs || !rule) return invalid("ctx, unitigs or rule is NULL");
    const int prefix_len = terminated_length(rule->name_prefix);
    switch (refuse(rule->flags, rule->k, prefix_len, rule->reserved)) {
    case 1: return invalid("bl_gfa_rule: unknown flag bits (BL_GFA_NO_HEADER is the only flag)");
    case 2: return invalid("bl_gfa_rule: k must be odd and 3 .. 63");
    case 3: return invalid("bl_gfa_rule: name_prefix is NUL-terminated inside its 16 bytes");
    case 4: return invalid("bl_gfa_rule: reserved must be 0");
    default: break;
    }
    if (blh::misaligned16(d_out)) return invalid("d_out must be 16-byte aligned");
    if (n_unitigs && !d_unitig_offsets) return invalid("d_unitig_offsets is NULL");
    if (n_links && !d_links) return invalid("d_links is NULL with n_links > 0");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, unitigs, view));
    GfaParams p{};
    p.n_bases = view.n_bases;
    p.bases = view.bases;
    p.offsets = d_unitig_offsets;
    p.n_unitigs = n_unitigs;
    p.sums = d_count_sums;
    p.links = reinterpret_cast<const LinkWords*>(d_links);
    p.n_links = n_links;
    p.n_head = (rule->flags & BL_GFA_NO_HEADER) ? 0u : 1u;
    p.overlap = rule->k - 1;
    p.overlap_digits = p.overlap >= 10 ? 2u : 1u;
    blh::pack_prefix(rule->name_prefix, prefix_len, p.prefix);
    p.prefix_len = (uint32_t)prefix_len;
    p.first_number = rule->first_number;
    p.n_lines = p.n_head + n_unitigs + n_links;
    if (p.n_lines == 0) return BL_OK;

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    const uint64_t n1 = p.n_lines + 1;
    uint64_t* arena = static_cast<uint64_t*>(bl_ctx_scratch(ctx, 4, (size_t)(2 * n1) * sizeof(uint64_t)));  // lengths and their sums
    if (!arena) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    p.line_len = arena;
    uint64_t* line_off = arena + n1;
    p.line_off = line_off;
    hipLaunchKernelGGL(line_length_kernel, dim3(blocks_for(n1, TPB)), dim3(TPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    uint64_t total = 0;
    BLH_OK(blh::exclusive_sum_total(ctx, p.line_len, line_off, (size_t)n1, s, &total));
    if (n_bytes) *n_bytes = total;
    if (!d_out) return BL_OK;  // sizing only
    if (capacity < total) return bl_set_error(BL_ERR_CAPACITY, "bl_unitigs_format_gfa: d_out is smaller than the text (*n_bytes says how large it is)");
    p.total = total;
    p.out = d_out;
    const uint64_t waves = (total + WAVE_BYTES - 1) / WAVE_BYTES;
    hipLaunchKernelGGL(gfa_kernel, dim3(blocks_for(waves * 64, TPB)), dim3(TPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}
