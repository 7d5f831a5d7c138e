// bl_correct.hip — bl_scan_read_edits: single-substitution repair of reads from a count table, and bl_batch_apply_edits: the edits applied
// to a copy of the batch.  The per-thread bodies are in bl_correct_core.hpp.  Kernels:
//   state_kernel        the tile of bl_scan_kmer_counts (bl_tile128.hpp): a state byte per position instead of five bytes of count and validity
//   run_kernel<false>   one lane per position of the range: the candidates of a workgroup counted, the rejected runs into the statistics
//   run_kernel<true>    after rocPRIM's exclusive sum of the workgroups' counts: the candidates written in position order
//   test_kernel         the hot one: a wave per candidate, a lane per k-mer of the run, three alternatives through one search_group call,
//                       the verdict by ballots; lane 0 writes the edit or the class
//   compact_kernel      after the exclusive sum of the edit flags: the edits in candidate order, nothing at or beyond the capacity;
//                       the verdict classes into the statistics
//   copy_kernel         bl_batch_apply_edits: 16-byte stores
//   apply_kernel        one lane per edit
// No atomic decides where anything is stored; the only atomics add to the statistics words.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/biolib_amd.h"
#include "bl_correct_core.hpp"
#include "bl_host.hpp"
#include "bl_lookup_launch.hpp"
#include "bl_tile128.hpp"

static_assert(sizeof(blcr::Edit) == sizeof(bl_edit) && alignof(blcr::Edit) == 16, "Edit is bl_edit");
static_assert(sizeof(bl_edit_stats) == blcr::STAT_WORDS * sizeof(uint64_t), "the statistics words are bl_edit_stats");

namespace blcr {

typedef unsigned long long ull;

struct StateShared {
    uint32_t codes[bl::NCHUNK_POS];
    uint32_t flags[bl::NCHUNK_POS];
};

__global__ __launch_bounds__(bl::TPB) void state_kernel(const StateParams p)
{
    __shared__ StateShared sh;
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.km.origin + (int64_t)tile * bl::H;
        __syncthreads();  // the previous tile's codes and flags have been read
        bl::stage_tile128<bl::NCHUNK_POS>(p.km, sh.codes, sh.flags, tid, q0);
        __syncthreads();
        state_thread(p, sh.codes, sh.flags, tid, q0);
    }
}

// EMIT = false: block_counts[workgroup] = its candidates, stats += its runs by class.  EMIT = true: block_base = the exclusive sum of the
// counts; the candidates stored from there on in position order.
template <bool EMIT>
__global__ __launch_bounds__(CTPB) void run_kernel(const RunParams p, ull* block_counts, const ull* block_base, Candidate* cand, ull n_cand, ull* stats)
{
    __shared__ uint32_t wave_tot[CTPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t a = p.first + (int64_t)blockIdx.x * CTPB + tid;
    Candidate c{0, 0, 0};
    const int cls = a < p.end ? run_at(p, a, c) : RUN_NOT_A_START;
    const ull is_cand = __ballot(cls == RUN_CANDIDATE);
    if (lane == 0) wave_tot[wv] = (uint32_t)__popcll(is_cand);
    if (!EMIT) {
        const ull runs = __ballot(cls != RUN_NOT_A_START), misfit = __ballot(cls == RUN_MISFIT), low = __ballot(cls == RUN_LOW_SUPPORT);
        if (lane == 0) {
            if (runs) atomicAdd(&stats[STAT_RUNS], (ull)__popcll(runs));
            if (misfit) atomicAdd(&stats[STAT_MISFIT], (ull)__popcll(misfit));
            if (low) atomicAdd(&stats[STAT_LOW_SUPPORT], (ull)__popcll(low));
        }
    }
    __syncthreads();
    if (!EMIT) {
        if (tid == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int i = 0; i < CTPB / 64; ++i) all += wave_tot[i];
            block_counts[blockIdx.x] = all;
        }
    } else if (cls == RUN_CANDIDATE) {
        ull at = block_base[blockIdx.x] + (ull)__popcll(is_cand & ((1ull << lane) - 1));
#pragma unroll
        for (int i = 0; i < CTPB / 64; ++i)
            if (i < wv) at += wave_tot[i];
        if (at < n_cand) cand[at] = c;  // (always)
    }
}

__global__ __launch_bounds__(CTPB) void test_kernel(const TestParams p)
{
    __shared__ uint32_t words[TEST_WAVES][CODE_WORDS_PADDED];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const ull idx = (ull)blockIdx.x * TEST_WAVES + wv;
    const bool active = idx < p.n_cand;  // (wave-uniform)
    Candidate c{0, 1, 0};
    if (active) {
        c = p.cand[idx];
        if (lane < 4 * CODE_WORDS) reinterpret_cast<uint8_t*>(words[wv])[code_byte_index(lane)] = (uint8_t)code_byte(p.bases, p.n_bases, (int64_t)c.a + 4 * lane);
        else if (lane < 4 * CODE_WORDS + (CODE_WORDS_PADDED - CODE_WORDS)) words[wv][CODE_WORDS + lane - 4 * CODE_WORDS] = 0;
    }
    __syncthreads();
    if (!active) return;
    const bool mine = lane < (int)c.len;
    uint32_t orig = 0, fail = 0;
    if (mine) fail = test_lane(p, words[wv], c, lane, orig);
    uint32_t qualifying = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t)
        if (__ballot(mine && ((fail >> t) & 1u)) == 0) qualifying |= 1u << t;
    if (lane == 0) {
        Edit e{};
        const uint64_t pos = edit_position(c, p.k);
        const uint8_t from = pos < (uint64_t)p.n_bases ? p.bases[pos] : (uint8_t)0;  // (always inside: p lies in a valid k-mer)
        const uint32_t v = verdict(qualifying, orig, from, c, p.k, e);
        p.verdicts[idx] = (uint8_t)v;
        p.edit_flag[idx] = v == V_EDIT ? 1 : 0;
        if (v == V_EDIT) p.edits[idx] = e;
    }
}

__global__ __launch_bounds__(CTPB) void compact_kernel(const Edit* edits, const uint8_t* verdicts, const ull* edit_sum, ull n_cand, Edit* out, ull capacity, ull* stats)
{
    const ull i = (ull)blockIdx.x * CTPB + threadIdx.x;
    const uint32_t v = i < n_cand ? verdicts[i] : V_NONE;
    if (i < n_cand && out) compact_edit(edits, verdicts, reinterpret_cast<const uint64_t*>(edit_sum), i, out, capacity);
    const ull ed = __ballot(v == V_EDIT), amb = __ballot(v == V_AMBIGUOUS), nb = __ballot(v == V_NO_BASE);
    if ((threadIdx.x & 63) == 0) {
        if (ed) atomicAdd(&stats[STAT_EDITS], (ull)__popcll(ed));
        if (amb) atomicAdd(&stats[STAT_AMBIGUOUS], (ull)__popcll(amb));
        if (nb) atomicAdd(&stats[STAT_NO_BASE], (ull)__popcll(nb));
    }
}

// n16 16-byte chunks, then the tail's bytes; pad more zero bytes behind them
__global__ __launch_bounds__(CTPB) void copy_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, ull n_bytes, ull pad)
{
    const ull i = (ull)blockIdx.x * CTPB + threadIdx.x, n16 = n_bytes / 16;
    if (i < n16) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    if (i < (n_bytes & 15) + pad) {
        const ull at = 16 * n16 + i;
        dst[at] = at < n_bytes ? src[at] : (uint8_t)0;
    }
}

__global__ __launch_bounds__(CTPB) void apply_kernel(const Edit* edits, ull n_edits, uint8_t* bases, ull n_bases)
{
    edit_at(edits, n_edits, (ull)blockIdx.x * CTPB + threadIdx.x, bases, n_bases);
}

namespace {

using blh::blocks_for;
using blh::invalid;
using blh::round16;
static_assert(sizeof(ull) == sizeof(uint64_t), "blh::exclusive_sum sums the unit's counters as the 8-byte words they are");

}  // namespace

}  // namespace blcr

extern "C" int bl_scan_read_edits(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, const bl_table* table,
                                  uint32_t min_count, uint32_t min_support, bl_edit* d_edits, uint64_t capacity, bl_edit_stats* stats)
{
    using namespace blcr;
    if (!ctx || !batch || !table) return invalid("ctx, batch or table is NULL");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    const uint64_t n_bases = view.n_bases;
    BLH_OK(blh::table_owner(table->ctx, ctx));
    if (!d_edits && capacity != 0) return invalid("d_edits is NULL with a capacity: the counting call passes capacity 0");
    if (blh::misaligned16(d_edits)) return invalid("d_edits must be 16-byte aligned");
    if (k < 1 || k > (uint32_t)bl::MAX_UNIT128) return invalid("k must be in [1, 64]");
    BLH_OK(blh::table_takes_k(table->view.key_words, table->view.key_bits, k));
    if (min_count == 0) return invalid("min_count must be at least 1");
    if (min_support < 1 || min_support > k) return invalid("min_support must be in [1, k]");
    if (flags & ~(uint32_t)(BL_FLAG_CANONICAL | BL_FLAG_SYNC)) return invalid("flags: BL_FLAG_CANONICAL only (BL_FLAG_SYNC is accepted)");
    uint64_t end = 0;
    BLH_OK(blh::range_end(n_bases, first, n, "a scan range", end));
    if (stats) *stats = bl_edit_stats{};
    BLH_OK(bl_ctx_sync(ctx));  // the context's scans in flight
    if (end <= first) return BL_OK;

    const uint32_t* start_bits = nullptr;
    BLH_OK(bl_batch_scan_view(ctx, batch, 1, &start_bits));
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);

    // the states of the range, one position in front and k + 1 behind
    const int64_t s0 = first ? (int64_t)first - 1 : 0;
    const int64_t s1 = end + k + 1 < n_bases ? (int64_t)(end + k + 1) : (int64_t)n_bases;
    const ull n_blocks = (end - first + CTPB - 1) / CTPB;
    const size_t state_bytes = round16((size_t)(s1 - s0));
    unsigned char* arena = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 4, state_bytes + 2 * (size_t)(n_blocks + 1) * sizeof(ull)));
    ull* d_stats = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 128));
    if (!arena || !d_stats) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    ull* block_counts = reinterpret_cast<ull*>(arena + state_bytes);
    ull* block_base = block_counts + (n_blocks + 1);

    StateParams sp{};
    sp.km.bases = view.bases;
    sp.km.n_bases = (int64_t)n_bases;
    sp.km.start_bits = start_bits;
    bl::plan_kmers128(s0, s1, sp.km);
    sp.km.unit = (int32_t)k;
    sp.km.canonical = (flags & BL_FLAG_CANONICAL) ? 1 : 0;
    sp.table = table->view;
    sp.min_count = min_count;
    sp.states = arena;
    BLH_TRY(hipMemsetAsync(d_stats, 0, STAT_WORDS * sizeof(ull), s));
    BLH_TRY(hipMemsetAsync(block_counts + n_blocks, 0, sizeof(ull), s));
    BLH_TRY(bl::launch_tiles128(state_kernel, sp, sp.km.n_tiles, s));

    RunParams rp{};
    rp.states = arena;
    rp.s0 = s0;
    rp.s1 = s1;
    rp.first = (int64_t)first;
    rp.end = (int64_t)end;
    rp.k = k;
    rp.min_support = min_support;
    hipLaunchKernelGGL(run_kernel<false>, dim3((unsigned)n_blocks), dim3(CTPB), 0, s, rp, block_counts, (const ull*)nullptr, (Candidate*)nullptr, (ull)0, d_stats);
    BLH_TRY(hipGetLastError());
    uint64_t n_cand = 0;
    BLH_OK(blh::exclusive_sum_total(ctx, reinterpret_cast<const uint64_t*>(block_counts), reinterpret_cast<uint64_t*>(block_base), (size_t)(n_blocks + 1), s, &n_cand));

    if (n_cand) {
        // slot 0: candidates | their edits | edit flags | the flags' exclusive sum | verdicts
        const size_t rec = (size_t)n_cand * sizeof(Candidate), words = (size_t)(n_cand + 1) * sizeof(ull);
        unsigned char* ca = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 0, 2 * rec + 2 * words + round16((size_t)n_cand)));
        if (!ca) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        Candidate* cand = reinterpret_cast<Candidate*>(ca);
        Edit* edits = reinterpret_cast<Edit*>(ca + rec);
        ull* edit_flag = reinterpret_cast<ull*>(ca + 2 * rec);
        ull* edit_sum = edit_flag + (n_cand + 1);
        uint8_t* verdicts = ca + 2 * rec + 2 * words;
        hipLaunchKernelGGL(run_kernel<true>, dim3((unsigned)n_blocks), dim3(CTPB), 0, s, rp, (ull*)nullptr, (const ull*)block_base, cand, n_cand, (ull*)nullptr);
        BLH_TRY(hipGetLastError());
        TestParams tp{};
        tp.bases = sp.km.bases;
        tp.n_bases = (int64_t)n_bases;
        tp.table = table->view;
        tp.k = k;
        tp.min_count = min_count;
        tp.canonical = (uint32_t)sp.km.canonical;
        tp.cand = cand;
        tp.n_cand = n_cand;
        tp.edits = edits;
        tp.verdicts = verdicts;
        tp.edit_flag = reinterpret_cast<uint64_t*>(edit_flag);
        BLH_TRY(hipMemsetAsync(edit_flag + n_cand, 0, sizeof(ull), s));
        hipLaunchKernelGGL(test_kernel, dim3((unsigned)((n_cand + TEST_WAVES - 1) / TEST_WAVES)), dim3(CTPB), 0, s, tp);
        BLH_TRY(hipGetLastError());
        BLH_OK(blh::exclusive_sum(ctx, reinterpret_cast<const uint64_t*>(edit_flag), reinterpret_cast<uint64_t*>(edit_sum), (size_t)(n_cand + 1), s));
        hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(n_cand, CTPB)), dim3(CTPB), 0, s, edits, verdicts, (const ull*)edit_sum, n_cand, reinterpret_cast<Edit*>(d_edits), (ull)capacity, d_stats);
        BLH_TRY(hipGetLastError());
    }
    ull host[STAT_WORDS] = {};
    BLH_TRY(hipMemcpyAsync(host, d_stats, sizeof(host), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (stats) {
        stats->n_runs = host[STAT_RUNS];
        stats->n_edits = host[STAT_EDITS];
        stats->n_ambiguous = host[STAT_AMBIGUOUS];
        stats->n_no_base = host[STAT_NO_BASE];
        stats->n_misfit = host[STAT_MISFIT];
        stats->n_low_support = host[STAT_LOW_SUPPORT];
    }
    if (host[STAT_EDITS] > capacity) return bl_set_error(BL_ERR_CAPACITY, "more edits than the capacity: stats->n_edits is the count");
    return BL_OK;
}

extern "C" int bl_batch_apply_edits(bl_ctx* ctx, const bl_batch* batch, const bl_edit* d_edits, uint64_t n_edits, bl_batch** out)
{
    using namespace blcr;
    if (!ctx || !batch || !out) return invalid("ctx, batch or out is NULL");
    *out = nullptr;
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    const uint64_t n_bases = view.n_bases;
    if (n_edits && !d_edits) return invalid("d_edits is NULL");
    if (blh::misaligned16(d_edits)) return invalid("d_edits must be 16-byte aligned");
    BLH_OK(bl_ctx_sync(ctx));
    const uint32_t* start_bits = nullptr;  // (NULL on a fixed-length batch that has not needed them: the copy builds its own on demand)
    BLH_OK(bl_batch_scan_view(ctx, batch, 0, &start_bits));
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);

    const size_t bit_words = (size_t)((n_bases + 31) / 32 + 4);  // the length every maker of start bits gives them
    blh::Pooled<uint8_t> d_bases(ctx, (size_t)n_bases + 64);
    blh::Pooled<uint32_t> d_bits;
    if (start_bits) d_bits = blh::Pooled<uint32_t>(ctx, bit_words * sizeof(uint32_t));
    if (!d_bases || (start_bits && !d_bits)) return bl_set_error(BL_ERR_OOM, "device allocation failed (batch)");
    hipLaunchKernelGGL(copy_kernel, dim3(blocks_for(n_bases / 16 + 80, CTPB)), dim3(CTPB), 0, s, view.bases, d_bases.get(), (ull)n_bases, (ull)64);  // 64 bytes of zeros behind the bases
    BLH_TRY(hipGetLastError());
    if (d_bits) {
        hipLaunchKernelGGL(copy_kernel, dim3(blocks_for(bit_words * 4 / 16 + 16, CTPB)), dim3(CTPB), 0, s, reinterpret_cast<const uint8_t*>(start_bits),
                           reinterpret_cast<uint8_t*>(d_bits.get()), (ull)(bit_words * 4), (ull)0);
        BLH_TRY(hipGetLastError());
    }
    if (n_edits) {
        hipLaunchKernelGGL(apply_kernel, dim3(blocks_for(n_edits, CTPB)), dim3(CTPB), 0, s, reinterpret_cast<const Edit*>(d_edits), (ull)n_edits, d_bases.get(), (ull)n_bases);
        BLH_TRY(hipGetLastError());
    }
    BLH_TRY(hipStreamSynchronize(s));
    return bl_batch_adopt_like(ctx, batch, d_bases.release(), d_bits.release(), out);  // takes ownership of both
}
