// bl_steps.hip — reads threaded through the compacted graph: bl_scan_read_steps (one record per unitig visit of a read), bl_link_support
// (the reads that crossed every link record) and bl_steps_format_gaf (the walks as GAF text made on the device).  The definitions are in
// include/biolib_amd.h, the per-thread bodies in bl_steps_core.hpp.  Kernels:
//   node_kernel          the hot one: the tile of bl_scan_kmer_counts (bl_tile128.hpp), the slot of every k-mer instead of its count, one
//                        8-byte node gather and one packed 8-byte word per position
//   ends_kernel<false>   one lane per position: the heads of a workgroup counted
//   ends_kernel<true>    after rocPRIM's exclusive sum of the workgroups' counts: the heads and the tails written in position order
//   step_kernel          one lane per step: the record, the statistics
//   support_kernel       one lane per pair of neighbouring steps: integer atomic adds on the records' counters (order-independent)
//   gaf_measure_kernel, gaf_chain_kernel, gaf_length_kernel, gaf_write_kernel   the text: one lane per step or chain
// No atomic decides where anything is stored.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/biolib_amd.h"
#include "bl_graph_core.hpp"
#include "bl_host.hpp"
#include "bl_lookup_launch.hpp"
#include "bl_steps_core.hpp"
#include "bl_tile128.hpp"

static_assert(sizeof(bl_read_step) == sizeof(blst::Step) && alignof(blst::Step) == 16, "Step is bl_read_step");
static_assert(sizeof(bl_unitig_node) == sizeof(blst::Node) && sizeof(bl_unitig_link) == sizeof(blst::LinkWords), "the device words are the caller's");
static_assert(sizeof(bl_step_stats) == 8 * sizeof(uint64_t) && sizeof(bl_support_stats) == 4 * sizeof(uint64_t) && sizeof(bl_gaf_rule) == 64, "the header's structs");
static_assert((uint32_t)BL_STEP_LINKED == blst::LINKED && (uint32_t)BL_STEP_CONTINUED == blst::CONTINUED, "the header's constants");

namespace blst {

typedef unsigned long long ull;

struct NodeShared {
    uint32_t codes[bl::NCHUNK_POS];
    uint32_t flags[bl::NCHUNK_POS];
};

__global__ __launch_bounds__(bl::TPB) void node_kernel(const NodeParams p, ull* stats)
{
    __shared__ NodeShared sh;
    const int tid = threadIdx.x;
    uint32_t n_valid = 0, n_found = 0;
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.km.origin + (int64_t)tile * bl::H;
        __syncthreads();  // the previous tile's codes and flags have been read
        bl::stage_tile128<bl::NCHUNK_POS>(p.km, sh.codes, sh.flags, tid, q0);
        __syncthreads();
        node_thread(p, sh.codes, sh.flags, tid, q0, n_valid, n_found);
    }
    const ull v = bl::wave_sum_u64(((ull)n_found << 32) | n_valid);  // (a call sees at most 2^31 + 1 positions: both sums of a wave fit their halves)
    if ((tid & 63) == 0) {
        if (v & 0xffffffffull) atomicAdd(&stats[STAT_VALID], v & 0xffffffffull);
        if (v >> 32) atomicAdd(&stats[STAT_FOUND], v >> 32);
    }
}

// EMIT = false: block_counts[workgroup] = its heads.  EMIT = true: block_base = the exclusive sum of the counts; the heads and the tails
// stored from there on in position order.
template <bool EMIT>
__global__ __launch_bounds__(STPB) void ends_kernel(const StepParams p, ull* block_counts, const ull* block_base, ull n_steps, uint32_t* heads, uint32_t* tails)
{
    __shared__ uint32_t wave_tot[STPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t pos = p.first + (int64_t)blockIdx.x * STPB + tid;
    const uint32_t cls = pos < p.end ? classify(p, pos) : 0u;
    const ull is_head = __ballot((cls & HEAD) != 0);
    if (lane == 0) wave_tot[wv] = (uint32_t)__popcll(is_head);
    __syncthreads();
    if (!EMIT) {
        if (tid == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int i = 0; i < STPB / 64; ++i) all += wave_tot[i];
            block_counts[blockIdx.x] = all;
        }
    } else if (cls) {
        ull before = block_base[blockIdx.x] + (ull)__popcll(is_head & ((1ull << lane) - 1));
#pragma unroll
        for (int i = 0; i < STPB / 64; ++i)
            if (i < wv) before += wave_tot[i];
        emit_ends(p, pos, cls, before, n_steps, heads, tails);
    }
}

__global__ __launch_bounds__(STPB) void step_kernel(const FinishParams p, Step* out, ull* stats)
{
    const ull j = (ull)blockIdx.x * STPB + threadIdx.x;
    Step st{};
    const bool live = j < p.n_steps;
    if (live) {
        st = make_step(p, j);
        if (out) out[j] = st;
    }
    const ull chains = __ballot(live && st.flags == 0), linked = __ballot(live && (st.flags & LINKED));
    ull longest = live ? st.n_kmers : 0;
    for (int d = 32; d >= 1; d >>= 1) {
        const ull o = __shfl_xor(longest, d, 64);
        longest = o > longest ? o : longest;
    }
    if ((threadIdx.x & 63) == 0) {
        if (chains) atomicAdd(&stats[STAT_CHAINS], (ull)__popcll(chains));
        if (linked) atomicAdd(&stats[STAT_LINKED], (ull)__popcll(linked));
        if (longest) atomicMax(&stats[STAT_LONGEST], longest);
    }
}

// counters: 0 transitions, 1 unmatched
__global__ __launch_bounds__(STPB) void support_kernel(const SupportParams p, ull* counters)
{
    const int r = support_thread(p, (ull)blockIdx.x * STPB + threadIdx.x);
    const ull any = __ballot(r != 0), un = __ballot(r == 2);
    if ((threadIdx.x & 63) == 0) {
        if (any) atomicAdd(&counters[0], (ull)__popcll(any));
        if (un) atomicAdd(&counters[1], (ull)__popcll(un));
    }
}

// counters[0]: OR of the steps' CONTINUED bits
__global__ __launch_bounds__(STPB) void gaf_measure_kernel(const GafParams p, ull* counters)
{
    const uint32_t c = measure_step(p, (ull)blockIdx.x * STPB + threadIdx.x);
    if (__ballot(c != 0) && (threadIdx.x & 63) == 0) atomicOr(&counters[0], 1ull);
}
__global__ __launch_bounds__(STPB) void gaf_chain_kernel(const GafParams p) { chain_first(p, (ull)blockIdx.x * STPB + threadIdx.x); }
__global__ __launch_bounds__(STPB) void gaf_length_kernel(const GafParams p) { chain_length(p, (ull)blockIdx.x * STPB + threadIdx.x); }
__global__ __launch_bounds__(STPB) void gaf_write_kernel(const GafParams p) { write_step(p, (ull)blockIdx.x * STPB + threadIdx.x); }

namespace {

using blh::blocks_for;
using blh::invalid;
using blh::pack_prefix;
using blh::round16;
using blh::terminated_length;
static_assert(sizeof(ull) == sizeof(uint64_t), "blh::exclusive_sum sums the unit's counters as the 8-byte words they are");

}  // namespace

}  // namespace blst

extern "C" int bl_scan_read_steps(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, const bl_table* table,
                                  const bl_unitig_node* d_nodes, const uint64_t* d_unitig_offsets, uint64_t n_unitigs, const uint64_t* d_offsets,
                                  bl_read_step* d_steps, uint64_t capacity, bl_step_stats* stats)
{
    using namespace blst;
    if (!ctx || !batch || !table) return invalid("ctx, batch or table is NULL");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    const uint64_t n_bases = view.n_bases, n_seqs = view.n_seqs, read_len = view.read_len;
    BLH_OK(blh::table_owner(table->ctx, ctx));
    const bllk::TableView& t = table->view;
    switch (blgr::refuse(k, t.key_words, t.key_bits, t.n)) {
    case 1: return invalid("k must be odd and 3 .. 63");
    case 2: return invalid(("2k = " + std::to_string(2 * k) + " exceeds the table's key_bits = " + std::to_string(t.key_bits)).c_str());
    case 3: return invalid("a table of one-word keys takes k <= 31");
    case 4: return invalid("the table has 2^31 keys or more: a step's end holds a unitig and an orientation");
    default: break;
    }
    switch (refuse(k, t.n, n_unitigs)) {
    case 5: return invalid("k must be odd and 3 .. 63");
    case 7: return invalid("n_unitigs exceeds the table's number of keys");
    default: break;
    }
    if (t.n && (!d_nodes || !d_unitig_offsets)) return invalid("d_nodes or d_unitig_offsets is NULL on a table that is not empty");
    BLH_OK(blh::offsets_needed(d_offsets, n_seqs, read_len));
    if (!d_steps && capacity != 0) return invalid("d_steps is NULL with a capacity: the sizing call passes capacity 0");
    if (blh::misaligned16(d_steps)) return invalid("d_steps must be 16-byte aligned");
    if (flags & ~(uint32_t)(BL_FLAG_CANONICAL | BL_FLAG_SYNC)) return invalid("flags: BL_FLAG_CANONICAL and BL_FLAG_SYNC only (the canonical form is always used)");
    uint64_t end = 0;
    BLH_OK(blh::range_end(n_bases, first, n, "a scan range", end));
    if (stats) *stats = bl_step_stats{};
    BLH_OK(bl_ctx_sync(ctx));  // the context's scans in flight
    if (end <= first) return BL_OK;

    const uint32_t* start_bits = nullptr;
    BLH_OK(bl_batch_scan_view(ctx, batch, 1, &start_bits));
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);

    // slot 4: the words of the range and of the position in front of it | the workgroups' head counts | their exclusive sum
    const int64_t s0 = first ? (int64_t)first - 1 : 0;
    const ull n_blocks = (end - first + STPB - 1) / STPB;
    const size_t word_bytes = (size_t)(end - s0) * sizeof(uint64_t);
    unsigned char* arena = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 4, word_bytes + 2 * (size_t)(n_blocks + 1) * sizeof(ull)));
    ull* d_stats = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 128));
    if (!arena || !d_stats) return bl_set_error(BL_ERR_OOM, "scratch allocation failed (8 bytes per position)");
    ull* block_counts = reinterpret_cast<ull*>(arena + word_bytes);
    ull* block_base = block_counts + (n_blocks + 1);

    NodeParams np{};
    np.km.bases = view.bases;
    np.km.n_bases = (int64_t)n_bases;
    np.km.start_bits = start_bits;
    bl::plan_kmers128(s0, (int64_t)end, np.km);
    np.km.unit = (int32_t)k;
    np.km.canonical = 1;
    np.table = t;
    np.nodes = reinterpret_cast<const Node*>(d_nodes);
    np.unitig_offsets = d_unitig_offsets;
    np.n_unitigs = n_unitigs;
    np.first = (int64_t)first;
    np.words = reinterpret_cast<uint64_t*>(arena);
    BLH_TRY(hipMemsetAsync(d_stats, 0, STAT_WORDS * sizeof(ull), s));
    BLH_TRY(hipMemsetAsync(block_counts + n_blocks, 0, sizeof(ull), s));
    BLH_OK(bl_ctx_kernel_event(ctx, s, 1));  // (bl_ctx_kernel_timing: the node pass alone)
    hipLaunchKernelGGL(node_kernel, dim3(bl::grid_for(np.km.n_tiles)), dim3(bl::TPB), 0, s, np, d_stats);
    BLH_TRY(hipGetLastError());
    BLH_OK(bl_ctx_kernel_event(ctx, s, 0));

    StepParams sp{};
    sp.words = np.words;
    sp.s0 = s0;
    sp.start_bits = start_bits;
    sp.first = (int64_t)first;
    sp.end = (int64_t)end;
    hipLaunchKernelGGL(ends_kernel<false>, dim3((unsigned)n_blocks), dim3(STPB), 0, s, sp, block_counts, (const ull*)nullptr, (ull)0, (uint32_t*)nullptr, (uint32_t*)nullptr);
    BLH_TRY(hipGetLastError());
    uint64_t n_steps = 0;
    BLH_OK(blh::exclusive_sum_total(ctx, reinterpret_cast<const uint64_t*>(block_counts), reinterpret_cast<uint64_t*>(block_base), (size_t)(n_blocks + 1), s, &n_steps));

    const bool store = d_steps && n_steps <= capacity;  // BL_ERR_CAPACITY leaves d_steps untouched
    if (n_steps) {
        // slot 0: the heads | the tails, four bytes each per step
        const size_t b_ends = round16((size_t)n_steps * sizeof(uint32_t));
        unsigned char* ends = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 0, 2 * b_ends));
        if (!ends) return bl_set_error(BL_ERR_OOM, "scratch allocation failed (8 bytes per step)");
        FinishParams fp{};
        fp.sp = sp;
        fp.heads = reinterpret_cast<const uint32_t*>(ends);
        fp.tails = reinterpret_cast<const uint32_t*>(ends + b_ends);
        fp.n_steps = n_steps;
        fp.seq_offsets = d_offsets;
        fp.n_seqs = n_seqs;
        fp.read_len = d_offsets ? 0 : read_len;
        hipLaunchKernelGGL(ends_kernel<true>, dim3((unsigned)n_blocks), dim3(STPB), 0, s, sp, (ull*)nullptr, (const ull*)block_base, n_steps,
                           reinterpret_cast<uint32_t*>(ends), reinterpret_cast<uint32_t*>(ends + b_ends));
        BLH_TRY(hipGetLastError());
        hipLaunchKernelGGL(step_kernel, dim3(blocks_for(n_steps, STPB)), dim3(STPB), 0, s, fp, store ? reinterpret_cast<Step*>(d_steps) : (Step*)nullptr, d_stats);
        BLH_TRY(hipGetLastError());
    }
    ull host[STAT_WORDS] = {};
    BLH_TRY(hipMemcpyAsync(host, d_stats, sizeof(host), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (stats) {
        stats->n_valid = host[STAT_VALID];
        stats->n_found = host[STAT_FOUND];
        stats->n_steps = n_steps;
        stats->n_chains = host[STAT_CHAINS];
        stats->n_linked = host[STAT_LINKED];
        stats->longest_step = host[STAT_LONGEST];
    }
    if (n_steps > capacity && (d_steps || capacity)) return bl_set_error(BL_ERR_CAPACITY, "more steps than the capacity: stats->n_steps is the count");
    return BL_OK;
}

extern "C" int bl_link_support(bl_ctx* ctx, const bl_read_step* d_steps, uint64_t n_steps, const uint64_t* d_link_offsets, const bl_unitig_link* d_links,
                               uint64_t n_links, uint64_t n_unitigs, uint32_t* d_support, bl_support_stats* stats)
{
    using namespace blst;
    if (!ctx) return invalid("ctx is NULL");
    if (n_steps && !d_steps) return invalid("d_steps is NULL with n_steps > 0");
    if (blh::misaligned16(d_steps)) return invalid("d_steps must be 16-byte aligned");
    if (n_unitigs >= (1ull << 31)) return invalid("n_unitigs must be below 2^31");
    if (n_unitigs && !d_link_offsets) return invalid("d_link_offsets is NULL with n_unitigs > 0");
    if (n_links && (!d_links || !d_support)) return invalid("d_links or d_support is NULL with n_links > 0");
    if (stats) *stats = bl_support_stats{};
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    ull* d_counters = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 128));
    if (!d_counters) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    BLH_TRY(hipMemsetAsync(d_counters, 0, 2 * sizeof(ull), s));
    if (n_links) BLH_TRY(hipMemsetAsync(d_support, 0, (size_t)n_links * sizeof(uint32_t), s));
    if (n_steps > 1 && n_unitigs) {
        SupportParams p{};
        p.steps = reinterpret_cast<const Step*>(d_steps);
        p.n_steps = n_steps;
        p.link_offsets = d_link_offsets;
        p.links = reinterpret_cast<const LinkWords*>(d_links);
        p.n_links = n_links;
        p.n_unitigs = n_unitigs;
        p.support = d_support;
        hipLaunchKernelGGL(support_kernel, dim3(blocks_for(n_steps - 1, STPB)), dim3(STPB), 0, s, p, d_counters);
        BLH_TRY(hipGetLastError());
    }
    ull host[2] = {};
    BLH_TRY(hipMemcpyAsync(host, d_counters, sizeof(host), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (stats) {
        stats->n_transitions = host[0];
        stats->n_unmatched = host[1];
    }
    return BL_OK;
}

extern "C" int bl_steps_format_gaf(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const bl_read_step* d_steps, uint64_t n_steps,
                                   const uint64_t* d_unitig_offsets, uint64_t n_unitigs, const bl_gaf_rule* rule, uint8_t* d_out, uint64_t capacity,
                                   uint64_t* n_bytes)
{
    using namespace blst;
    if (n_bytes) *n_bytes = 0;
    if (!ctx || !batch || !rule) return invalid("ctx, batch or rule is NULL");
    const int read_len_prefix = terminated_length(rule->read_prefix), seg_len_prefix = terminated_length(rule->segment_prefix);
    switch (refuse_rule(rule->flags, rule->k, read_len_prefix, seg_len_prefix, rule->reserved)) {
    case 1: return invalid("bl_gaf_rule: unknown flag bits (no flag is defined)");
    case 2: return invalid("bl_gaf_rule: k must be odd and 3 .. 63");
    case 3: return invalid("bl_gaf_rule: read_prefix and segment_prefix are NUL-terminated inside their 16 bytes");
    case 4: return invalid("bl_gaf_rule: reserved must be 0");
    default: break;
    }
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    BLH_OK(blh::offsets_needed(d_offsets, view.n_seqs, view.read_len));
    if (blh::misaligned16(d_out)) return invalid("d_out must be 16-byte aligned");
    if (blh::misaligned16(d_steps)) return invalid("d_steps must be 16-byte aligned");
    if (n_steps && !d_steps) return invalid("d_steps is NULL with n_steps > 0");
    if (n_unitigs && !d_unitig_offsets) return invalid("d_unitig_offsets is NULL with n_unitigs > 0");
    if (n_steps == 0) return BL_OK;
    GafParams p{};
    p.n_bases = view.n_bases;
    p.n_seqs = view.n_seqs;
    p.read_len = view.read_len;
    p.steps = reinterpret_cast<const Step*>(d_steps);
    p.n_steps = n_steps;
    p.unitig_offsets = d_unitig_offsets;
    p.n_unitigs = n_unitigs;
    p.seq_offsets = d_offsets;
    if (d_offsets) p.read_len = 0;
    p.k = rule->k;
    pack_prefix(rule->read_prefix, read_len_prefix, p.read_prefix);
    pack_prefix(rule->segment_prefix, seg_len_prefix, p.seg_prefix);
    p.read_prefix_len = (uint32_t)read_len_prefix;
    p.seg_prefix_len = (uint32_t)seg_len_prefix;
    p.read_first = rule->read_first_number;
    p.seg_first = rule->segment_first_number;

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    // slot 4: four measures and their four sums over the steps, then the chains' first steps, line lengths and line offsets
    const uint64_t n1 = n_steps + 1;
    uint64_t* arena = static_cast<uint64_t*>(bl_ctx_scratch(ctx, 4, (size_t)(11 * n1) * sizeof(uint64_t)));
    ull* d_counters = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 128));
    if (!arena || !d_counters) return bl_set_error(BL_ERR_OOM, "scratch allocation failed (88 bytes per step)");
    p.kmers = arena;
    p.keys = arena + n1;
    p.path = arena + 2 * n1;
    p.head = arena + 3 * n1;
    uint64_t* sums = arena + 4 * n1;
    p.kmers_sum = sums;
    p.keys_sum = sums + n1;
    p.path_sum = sums + 2 * n1;
    p.head_sum = sums + 3 * n1;
    p.chain_begin = arena + 8 * n1;  // n_chains <= n_steps
    p.line_len = arena + 9 * n1;
    uint64_t* line_off = arena + 10 * n1;
    p.line_off = line_off;
    BLH_TRY(hipMemsetAsync(d_counters, 0, sizeof(ull), s));
    hipLaunchKernelGGL(gaf_measure_kernel, dim3(blocks_for(n1, STPB)), dim3(STPB), 0, s, p, d_counters);
    BLH_TRY(hipGetLastError());
    for (int j = 0; j < 4; ++j) BLH_OK(blh::exclusive_sum(ctx, arena + j * n1, sums + j * n1, (size_t)n1, s));
    ull continued = 0, n_chains = 0;
    BLH_TRY(hipMemcpyAsync(&continued, d_counters, sizeof(ull), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipMemcpyAsync(&n_chains, p.head_sum + n_steps, sizeof(ull), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (continued) return invalid("a step carries BL_STEP_CONTINUED: fold the records of consecutive ranges first");
    p.n_chains = n_chains;
    hipLaunchKernelGGL(gaf_chain_kernel, dim3(blocks_for(n1, STPB)), dim3(STPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    hipLaunchKernelGGL(gaf_length_kernel, dim3(blocks_for(n_chains + 1, STPB)), dim3(STPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    uint64_t total = 0;
    BLH_OK(blh::exclusive_sum_total(ctx, p.line_len, line_off, (size_t)(n_chains + 1), s, &total));
    if (n_bytes) *n_bytes = total;
    if (!d_out) return BL_OK;  // sizing only
    if (capacity < total) return bl_set_error(BL_ERR_CAPACITY, "bl_steps_format_gaf: d_out is smaller than the text (*n_bytes says how large it is)");
    p.total = total;
    p.out = d_out;
    hipLaunchKernelGGL(gaf_write_kernel, dim3(blocks_for(n_steps, STPB)), dim3(STPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}
