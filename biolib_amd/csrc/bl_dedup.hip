// bl_dedup.hip — bl_scan_read_duplicates: exact duplicate reads and pairs of a batch, one record per unit and spans for the kept ones
// (what fastp --dedup, clumpify dedupe and Picard MarkDuplicates without coordinates do).  The per-lane bodies are in bl_dedup_core.hpp.
//   hash     sixteen lanes to a unit (four units to a wave) add up the mixed 32-base words of its keys, from the batch's packed copy;
//            under BL_DEDUP_CANONICAL both orientations, the smaller hash kept.  One 16-byte key per unit: hash bits above the index
//   sort     rocPRIM radix sort over the used bits: groups of equal hash lie together, by ascending index inside
//   resolve  rounds of mark (a thread per place: singletons and empties are done), a segmented minimum scan that finds every group's
//            first unresolved place, and compare (sixteen lanes to a place, word by word against that head); until none is left
//   finish   the members ordered by class (a second sort only where a group held several classes or a unit was empty), the
//            segmented maximum of (score, lowest index) and the class sizes (reduce by key), then records, spans and statistics
// No atomic decides a value or a place: the only atomics are the integer sums and the maximum of the statistics on striped counters.
// The one word many threads store without an atomic is flag word 0 / 1, and they all store 1.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <string>

#include "../../include/biolib_amd.h"
#include "bl_dedup_core.hpp"
#include "bl_host.hpp"
#include "bl_keylist.hpp"

static_assert(sizeof(bld::Rule) == sizeof(bl_dedup_rule) && sizeof(bld::Record) == sizeof(bl_read_duplicate) && sizeof(bl_read_duplicate) == 16,
              "the header's structs");
static_assert(offsetof(bld::Rule, prefix_len) == offsetof(bl_dedup_rule, prefix_len) && offsetof(bld::Rule, seed) == offsetof(bl_dedup_rule, seed) &&
                  offsetof(bld::Record, copies) == offsetof(bl_read_duplicate, copies),
              "the header's layouts");
static_assert((uint32_t)BL_DEDUP_PAIRED == bld::FLAG_PAIRED && (uint32_t)BL_DEDUP_CANONICAL == bld::FLAG_CANONICAL && BL_DUP_DUPLICATE == bld::DUP_DUPLICATE &&
                  BL_DUP_EMPTY == bld::DUP_EMPTY && BL_DUP_REVERSED == bld::DUP_REVERSED,
              "the header's constants");
static_assert(sizeof(bl_dedup_stats) == 32 * sizeof(uint64_t), "bl_dedup_stats is 32 words");

namespace bld {

namespace {

// the sum of a value over the SUB lanes of a unit (a wave holds four units; every lane of the wave takes part)
__device__ __forceinline__ Hash sub_sum(Hash h)
{
#pragma unroll
    for (int d = SUB / 2; d >= 1; d >>= 1) {
        h.lo += __shfl_xor((unsigned long long)h.lo, d, 64);
        h.hi += __shfl_xor((unsigned long long)h.hi, d, 64);
    }
    return h;
}

__device__ __forceinline__ UnitSpan blank_span(const DedupParams& p)
{
    UnitSpan s;
    s.reads = (p.flags & FLAG_PAIRED) ? 2 : 1;
    s.empty = true;
    for (int t = 0; t < 2; ++t) s.start[t] = s.n[t] = s.b[t] = s.e[t] = 0;
    return s;
}

}  // namespace

__global__ __launch_bounds__(TPB) void dedup_hash_kernel(const DedupParams p)
{
    const uint64_t u = ((uint64_t)blockIdx.x * TPB + threadIdx.x) / SUB;
    const int sub = threadIdx.x % SUB;
    const bool active = u < p.n_units;
    const UnitSpan s = active ? unit_span(p, u) : blank_span(p);
    const bool reversed_too = (p.flags & (FLAG_CANONICAL | FLAG_PAIRED)) == FLAG_CANONICAL;
    Hash fwd[2], rev0;
    fwd[1].lo = fwd[1].hi = rev0.lo = rev0.hi = 0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (t >= s.reads) break;
        const uint64_t n = s.empty ? 0 : s.n[t];
        fwd[t] = hash_length(p, sub_sum(hash_part(p, s.start[t], n, false, sub)), n);
    }
    if (reversed_too) {
        const uint64_t n = s.empty ? 0 : s.n[0];
        rev0 = hash_length(p, sub_sum(hash_part(p, s.start[0], n, true, sub)), n);
    }
    if (!active || sub != 0) return;
    p.keys[u] = make_key(unit_hash(p, fwd, rev0), p.hash_bits, u, s.empty);
    p.notes[u] = s.empty ? U_EMPTY : 0;
    if (s.empty) p.flag_words[1] = 1u;
}

__global__ __launch_bounds__(TPB) void dedup_mark_kernel(const DedupParams p)
{
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (j < p.n_units) mark_place(p, j);
}

__global__ __launch_bounds__(TPB) void dedup_resolve_kernel(const DedupParams p)
{
    const uint64_t j = ((uint64_t)blockIdx.x * TPB + threadIdx.x) / SUB;
    const int sub = threadIdx.x % SUB;
    const uint32_t head = j < p.n_units ? place_head(p, j) : NONE32;
    uint32_t ok = 0;
    if (head != NONE32 && head != (uint32_t)j) {
        const UnitSpan a = unit_span(p, key_unit(p.keys[j])), h = unit_span(p, key_unit(p.keys[head]));
        ok = compare_unit(p, a, h, sub);
    }
#pragma unroll
    for (int d = SUB / 2; d >= 1; d >>= 1) ok &= __shfl_xor(ok, d, 64);
    if (head == NONE32 || sub != 0) return;
    const bool mixed = resolve_place(p, j, head, ok);
    if (mixed && p.counters) atomicAdd(&p.counters[(blockIdx.x % STRIPES) * STRIPE_WORDS + C_MIXED], 1ull);  // an integer sum
}

__global__ __launch_bounds__(TPB) void dedup_order_kernel(const DedupParams p, uint64_t* out)
{
    const uint64_t j = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (j < p.n_units) out[j] = order_key(p, j);
}

__global__ __launch_bounds__(TPB) void dedup_member_kernel(const DedupParams p)
{
    const uint64_t t = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (t < p.n_units) member_entry(p, t);
}

// the classes' results to the places of their heads
__global__ __launch_bounds__(TPB) void dedup_scatter_kernel(const uint32_t* heads, const Best* results, const uint32_t* n_classes, uint64_t n_units, Best* classes)
{
    const uint64_t c = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    if (c < *n_classes && heads[c] < n_units) classes[heads[c]] = results[c];
}

__global__ __launch_bounds__(TPB) void dedup_finish_kernel(const DedupParams p)
{
    const int lane = threadIdx.x & 63;
    const uint64_t n_threads = (uint64_t)gridDim.x * TPB;
    unsigned long long mine = 0;  // lane k's: counter k of this wave
    for (uint64_t j0 = (uint64_t)blockIdx.x * TPB + (threadIdx.x & ~63u); j0 < p.n_units; j0 += n_threads) {
        const uint64_t j = j0 + (uint64_t)lane;
        Tally t{};
        if (j < p.n_units) t = finish_place(p, j);
        if (!p.counters) continue;
        const uint32_t bin = t.copies ? (t.copies < 16 ? t.copies : 16) - 1 : NONE32;
        unsigned long long bases = t.bases_kept;
        uint32_t largest = t.copies;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            bases += __shfl_xor(bases, d, 64);
            const uint32_t other = __shfl_xor(largest, d, 64);
            largest = other > largest ? other : largest;
        }
        const unsigned long long add[C_HIST0] = {
            (unsigned long long)__builtin_popcountll(__ballot(t.empty)), (unsigned long long)__builtin_popcountll(__ballot(t.head)),
            (unsigned long long)__builtin_popcountll(__ballot(t.dup)),   (unsigned long long)__builtin_popcountll(__ballot(t.rev)),
            (unsigned long long)(__builtin_popcountll(__ballot(t.reads_kept >= 1)) + __builtin_popcountll(__ballot(t.reads_kept >= 2))), bases, 0ull};
#pragma unroll
        for (int k = 0; k < C_HIST0; ++k) mine += lane == k ? add[k] : 0ull;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned long long n = (unsigned long long)__builtin_popcountll(__ballot(bin == (uint32_t)k));
            mine += lane == C_HIST0 + k ? n : 0ull;
        }
        if (lane == C_LARGEST && largest > mine) mine = largest;
    }
    if (!p.counters || lane >= N_COUNTERS || !mine) return;
    unsigned long long* at = &p.counters[(blockIdx.x % STRIPES) * STRIPE_WORDS + lane];
    if (lane == C_LARGEST) atomicMax(at, mine);  // a maximum and integer sums: the order does not matter
    else atomicAdd(at, mine);
}

namespace {

using blh::invalid;

struct ScanJoin {
    __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return scan_join(a, b); }
};
struct BestJoin {
    __host__ __device__ Best operator()(const Best& a, const Best& b) const { return best_join(a, b); }
};

int launch_failed(const char* kernel)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BL_OK : bl_set_error(BL_ERR_HIP, (std::string(kernel) + ": " + hipGetErrorString(e)).c_str());
}

uint32_t bits_for(uint64_t n)  // the bits that hold every value below n
{
    uint32_t b = 1;
    while (b < 64 && (n - 1) >> b) ++b;
    return b;
}

}  // namespace

}  // namespace bld

extern "C" int bl_scan_read_duplicates(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const uint64_t* d_spans_in, const uint64_t* d_scores,
                                       const bl_dedup_rule* rule, bl_read_duplicate* d_records, uint64_t* d_spans, bl_dedup_stats* stats)
{
    using namespace bld;
    if (!ctx || !batch || !rule) return invalid("ctx, batch or rule is NULL");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    BLH_OK(blh::offsets_needed(d_offsets, view.n_seqs, view.read_len));
    Rule r;
    static_assert(sizeof(r) == sizeof(*rule), "one layout");
    std::memcpy(&r, rule, sizeof(r));
    if (const char* what = rule_error(r, view.n_seqs)) return invalid(what);
    if (blh::misaligned16(d_records) || blh::misaligned16(d_spans) || blh::misaligned16(d_spans_in))
        return invalid("d_records, d_spans and d_spans_in must be 16-byte aligned");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const uint64_t n = (r.flags & FLAG_PAIRED) ? view.n_seqs / 2 : view.n_seqs;
    if (n == 0) return BL_OK;

    DedupParams p{};
    p.src.bases = view.bases;
    p.src.n_bases = view.n_bases;
    p.src.offsets = d_offsets;
    p.src.read_len = d_offsets ? 0 : (view.read_len ? view.read_len : (view.n_bases ? view.n_bases : 1));
    p.src.n_seqs = view.n_seqs;
    BLH_OK(bl_batch_packed_view(ctx, batch, &p.src.codes_packed, &p.src.chunk_bad));
    p.src.spans_in = d_spans_in;
    p.scores = d_scores;
    p.flags = r.flags;
    p.hash_bits = r.hash_bits ? r.hash_bits : HASH_BITS;
    p.prefix_len = r.prefix_len;
    p.seed_lo = fmix64(r.seed + 0x2545f4914f6cdd1dull);
    p.seed_hi = fmix64(r.seed ^ 0x9fb21c651e98df25ull);
    p.n_units = n;
    p.out_records = reinterpret_cast<Record*>(d_records);
    p.out_spans = d_spans;

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the context's scans in flight and the calls that write the input spans and scores

    // slot 4, in units of n: two key arrays (the first is the members' once the keys are sorted), the class results twice, two pairs of
    // 8-byte words (the scan's, then the class order's), rep, the members' classes, the heads, the notes: 93 bytes per unit
    const size_t n16 = blh::round16(n * 16), n8 = blh::round16(n * 8), n4 = blh::round16(n * 4), n1 = blh::round16(n);
    char* block = static_cast<char*>(bl_ctx_scratch(ctx, 4, 4 * n16 + 2 * n8 + 3 * n4 + n1));
    constexpr size_t STRIPE_BYTES = STRIPES * STRIPE_WORDS * sizeof(unsigned long long);
    char* small = static_cast<char*>(bl_ctx_scratch(ctx, 6, STRIPE_BYTES + 64));
    if (!block || !small) return blkeys::scratch_failed();
    Key* unsorted = reinterpret_cast<Key*>(block);
    p.members = reinterpret_cast<Best*>(block);
    Key* sorted = reinterpret_cast<Key*>(block + n16);
    Best* results = reinterpret_cast<Best*>(block + 2 * n16);
    Best* classes = reinterpret_cast<Best*>(block + 3 * n16);
    uint64_t* words_a = reinterpret_cast<uint64_t*>(block + 4 * n16);
    uint64_t* words_b = reinterpret_cast<uint64_t*>(block + 4 * n16 + n8);
    p.rep = reinterpret_cast<uint32_t*>(block + 4 * n16 + 2 * n8);
    p.member_class = p.rep + n4 / 4;
    uint32_t* heads = p.member_class + n4 / 4;
    p.notes = reinterpret_cast<uint8_t*>(heads + n4 / 4);
    p.classes = classes;
    p.counters = stats ? reinterpret_cast<unsigned long long*>(small) : nullptr;
    p.flag_words = reinterpret_cast<uint32_t*>(small + STRIPE_BYTES);  // [0] left, [1] empty, [2] the number of classes
    BLH_TRY(hipMemsetAsync(small, 0, STRIPE_BYTES + 64, s));

    const unsigned per_place = blh::blocks_for(n, TPB), per_unit = blh::blocks_for(n * SUB, TPB);
    // with bl_ctx_kernel_timing on: five markers (bl_ctx_mark) around the four phases, for a benchmark to read with bl_ctx_mark_times
    const bool marks = bl_ctx_kernel_timing_on(ctx) != 0;
    if (marks) BLH_OK(bl_ctx_mark(ctx));
    // 1: hash
    p.keys = unsorted;
    hipLaunchKernelGGL(dedup_hash_kernel, dim3(per_unit), dim3(TPB), 0, s, p);
    BLH_OK(launch_failed("dedup_hash_kernel"));
    if (marks) BLH_OK(bl_ctx_mark(ctx));
    // 2: sort
    BLH_TRY(blkeys::sort_to(ctx, reinterpret_cast<__uint128_t*>(unsorted), reinterpret_cast<__uint128_t*>(sorted), n, 32 + p.hash_bits, s));
    p.keys = sorted;
    if (marks) BLH_OK(bl_ctx_mark(ctx));
    // 3: rounds.  Each reads back one word: whether a member is left
    uint32_t flags[2] = {0, 0};
    uint64_t rounds = 0;
    for (;;) {
        p.round = (uint32_t)(rounds < 0xffffffffull ? rounds + 1 : 0xffffffffull);
        ++rounds;
        if (rounds > 1) BLH_TRY(hipMemsetAsync(p.flag_words, 0, sizeof(uint32_t), s));
        p.scan = words_a;
        hipLaunchKernelGGL(dedup_mark_kernel, dim3(per_place), dim3(TPB), 0, s, p);
        BLH_OK(launch_failed("dedup_mark_kernel"));
        BLH_TRY(blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) { return rocprim::inclusive_scan(ws, bytes, words_a, words_b, (size_t)n, ScanJoin(), s); }));
        p.scan = words_b;
        hipLaunchKernelGGL(dedup_resolve_kernel, dim3(per_unit), dim3(TPB), 0, s, p);
        BLH_OK(launch_failed("dedup_resolve_kernel"));
        BLH_TRY(hipMemcpyAsync(flags, p.flag_words, sizeof(flags), hipMemcpyDeviceToHost, s));
        BLH_TRY(hipStreamSynchronize(s));
        if (!flags[0]) break;
    }
    if (marks) BLH_OK(bl_ctx_mark(ctx));
    // 4: finish
    if (rounds > 1 || flags[1]) {  // a group held several classes, or empty units lie among the others: order the places by class
        hipLaunchKernelGGL(dedup_order_kernel, dim3(per_place), dim3(TPB), 0, s, p, words_a);
        BLH_OK(launch_failed("dedup_order_kernel"));
        BLH_TRY(blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) { return rocprim::radix_sort_keys(ws, bytes, words_a, words_b, (size_t)n, 0u, 32 + bits_for(n), s); }));
        p.order = words_b;
    }
    hipLaunchKernelGGL(dedup_member_kernel, dim3(per_place), dim3(TPB), 0, s, p);
    BLH_OK(launch_failed("dedup_member_kernel"));
    uint32_t* d_n_classes = p.flag_words + 2;
    BLH_TRY(blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) {
        return rocprim::reduce_by_key(ws, bytes, p.member_class, p.members, (size_t)n, heads, results, d_n_classes, BestJoin(), rocprim::equal_to<uint32_t>(), s);
    }));
    hipLaunchKernelGGL(dedup_scatter_kernel, dim3(per_place), dim3(TPB), 0, s, heads, results, d_n_classes, n, classes);
    BLH_OK(launch_failed("dedup_scatter_kernel"));
    hipLaunchKernelGGL(dedup_finish_kernel, dim3(per_place < 2048u ? per_place : 2048u), dim3(TPB), 0, s, p);
    BLH_OK(launch_failed("dedup_finish_kernel"));
    if (marks) BLH_OK(bl_ctx_mark(ctx));
    if (!stats) return BL_OK;

    unsigned long long stripes[STRIPES * STRIPE_WORDS];
    BLH_TRY(hipMemcpyAsync(stripes, p.counters, sizeof(stripes), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    uint64_t host[N_COUNTERS] = {};
    for (int i = 0; i < STRIPES; ++i)
        for (int k = 0; k < N_COUNTERS; ++k) {
            const uint64_t x = stripes[i * STRIPE_WORDS + k];
            host[k] = k == C_LARGEST ? (x > host[k] ? x : host[k]) : host[k] + x;
        }
    stats->n_units = n;
    stats->n_empty = host[C_EMPTY];
    stats->n_classes = host[C_CLASSES];
    stats->n_duplicates = host[C_DUP];
    stats->n_reversed = host[C_REV];
    stats->largest_class = host[C_LARGEST];
    stats->n_reads_kept = host[C_READS_KEPT];
    stats->n_bases_kept = host[C_BASES_KEPT];
    for (int k = 0; k < 16; ++k) stats->class_hist[k] = host[C_HIST0 + k];
    stats->n_mixed_groups = host[C_MIXED];
    stats->rounds = rounds;
    return BL_OK;
}
