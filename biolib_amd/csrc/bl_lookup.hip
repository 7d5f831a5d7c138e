// bl_lookup.hip — the count table: what consumes the (k-mer, multiplicity) arrays the counting calls return.  bl_table_build_* sorts
// and merges any list of keys with counts into sorted distinct keys, saturating 32-bit counts and a prefix index; bl_table_lookup_*
// answers key arrays; bl_scan_kmer_counts (entry in bl_capi.hip) looks up every k-mer of a batch range inside the scan, so that the
// k-mers never reach memory; bl_table_histogram is the count-of-counts spectrum.  As in bl_setops128.hip the pair sort and the
// reduce-by-key of the build are rocPRIM device primitives (library plumbing).  Hand-written: the OR check of the key_bits promise, the
// index fill, the lookup kernel, the scan kernel (the tile of kmer128_kernel, bl_tile128.hpp) and the histogram.  The per-thread bodies
// are in bl_lookup_core.hpp.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/iterator/constant_iterator.hpp>

#include <new>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"
#include "bl_lookup_launch.hpp"
#include "bl_tile128.hpp"

namespace bllk {

namespace {

typedef unsigned long long ull;

// OR of all low words into out[0], of all high words into out[1] (one-word keys: every word is a low word)
__global__ __launch_bounds__(LTPB) void or_reduce_kernel(const uint64_t* __restrict__ keys, ull n, uint32_t key_words, ull* out)
{
    ull lo = 0, hi = 0;
    for (ull i = (ull)blockIdx.x * LTPB + threadIdx.x; i < n; i += (ull)gridDim.x * LTPB) {
        if (key_words == 2) {
            const Key2 k = reinterpret_cast<const Key2*>(keys)[i];
            lo |= k.lo;
            hi |= k.hi;
        } else {
            lo |= keys[i];
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        lo |= __shfl_xor(lo, d, 64);
        hi |= __shfl_xor(hi, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (lo) atomicOr(&out[0], lo);
        if (hi) atomicOr(&out[1], hi);
    }
}

__global__ __launch_bounds__(LTPB) void index_fill_kernel(const TableView t, uint32_t* __restrict__ index)
{
    const ull j = (ull)blockIdx.x * LTPB + threadIdx.x;
    if (j <= (1ull << t.prefix_bits)) index[j] = index_entry(t, (uint32_t)j);
}

// a workgroup takes LTPB * G queries at a time, query g of a lane LTPB behind query g - 1: the loads and the stores of a wave are contiguous
__global__ __launch_bounds__(LTPB) void lookup_kernel(const TableView t, const uint64_t* __restrict__ q, ull nq, uint32_t* __restrict__ out)
{
    for (ull base = (ull)blockIdx.x * (LTPB * G); base < nq; base += (ull)gridDim.x * (LTPB * G)) lookup_thread(t, q, nq, base + threadIdx.x, LTPB, out);
}

// n_bins <= HIST_LDS_BINS: per-workgroup bins in LDS, then one atomic per non-empty bin and workgroup
__global__ __launch_bounds__(LTPB) void histogram_lds_kernel(const uint32_t* __restrict__ counts, uint32_t n, uint32_t n_bins, ull* __restrict__ hist)
{
    __shared__ uint32_t bins[HIST_LDS_BINS];
    for (uint32_t b = threadIdx.x; b < n_bins; b += LTPB) bins[b] = 0;
    __syncthreads();
    for (ull i = (ull)blockIdx.x * LTPB + threadIdx.x; i < n; i += (ull)gridDim.x * LTPB) atomicAdd(&bins[histogram_bin(counts[i], n_bins)], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n_bins; b += LTPB)
        if (bins[b]) atomicAdd(&hist[b], (ull)bins[b]);
}

// more bins than LDS holds: one atomic per key on the device array
__global__ __launch_bounds__(LTPB) void histogram_global_kernel(const uint32_t* __restrict__ counts, uint32_t n, uint32_t n_bins, ull* __restrict__ hist)
{
    for (ull i = (ull)blockIdx.x * LTPB + threadIdx.x; i < n; i += (ull)gridDim.x * LTPB) atomicAdd(&hist[histogram_bin(counts[i], n_bins)], 1ull);
}

struct ScanCountShared {
    uint32_t codes[bl::NCHUNK_POS];
    uint32_t flags[bl::NCHUNK_POS];
    unsigned long long dig[5];
};

constexpr unsigned SCAN_SLOTS = bl::DIG_COUNT | bl::DIG_LO | bl::DIG_HASH | bl::DIG_POS | bl::DIG_HI;

}  // namespace

// The fused scan: kmer128_kernel's loop over the tiles.  Slot 2 (xor_hash) carries the number of k-mers found and slot 3 (xor_pos) the
// sum of the counts: both are wrapping sums here, with the count.
__global__ __launch_bounds__(bl::TPB) void scan_counts_kernel(const ScanCountParams p)
{
    __shared__ ScanCountShared sh;
    const int tid = threadIdx.x;
    bl::Kmer128Acc acc{0, 0, 0, 0, 0};
    bl::zero_digest128<SCAN_SLOTS>(sh.dig, tid);
    for (int tile = blockIdx.x; tile < p.km.n_tiles; tile += gridDim.x) {
        const int64_t q0 = p.km.origin + (int64_t)tile * bl::H;
        __syncthreads();  // the previous tile's codes and flags have been read
        bl::stage_tile128<bl::NCHUNK_POS>(p.km, sh.codes, sh.flags, tid, q0);
        __syncthreads();
        scan_counts_thread(p, sh.codes, sh.flags, tid, q0, acc);
    }
    bl::fold_digest128<SCAN_SLOTS, bl::DIG_COUNT | bl::DIG_HASH | bl::DIG_POS>(p.km.shards, sh.dig, tid, acc);
}

hipError_t launch_scan_counts(const ScanCountParams& p, hipStream_t stream) { return bl::launch_tiles128(scan_counts_kernel, p, p.km.n_tiles, stream); }

void free_table(bl_table* t)
{
    if (t->view.keys) (void)hipFree(const_cast<uint64_t*>(t->view.keys));
    if (t->view.counts) (void)hipFree(const_cast<uint32_t*>(t->view.counts));
    if (t->view.index) (void)hipFree(const_cast<uint32_t*>(t->view.index));
    delete t;
}

int new_table(bl_ctx* ctx, uint32_t key_words, uint32_t key_bits, uint64_t n, bl_table** out)
{
    *out = nullptr;
    bl_table* t = new (std::nothrow) bl_table{};
    if (!t) return bl_set_error(BL_ERR_OOM, "out of host memory");
    t->ctx = ctx;
    t->device = bl_ctx_device(ctx);
    t->view.key_words = key_words;
    t->view.key_bits = key_bits;
    t->view.n = (uint32_t)n;
    if (n) {
        void* keys = nullptr;
        void* counts = nullptr;
        hipError_t e = hipMalloc(&keys, (size_t)n * key_words * sizeof(uint64_t));
        t->view.keys = static_cast<uint64_t*>(keys);
        if (e == hipSuccess) e = hipMalloc(&counts, (size_t)n * sizeof(uint32_t));
        t->view.counts = static_cast<uint32_t*>(counts);
        if (e != hipSuccess) {
            free_table(t);
            return blh::hip_rc(e);
        }
    }
    *out = t;
    return BL_OK;
}

hipError_t finish_table(bl_ctx* ctx, bl_table* t, hipStream_t s)
{
    t->view.prefix_bits = choose_prefix_bits(bl_ctx_table_prefix_bits(ctx), t->view.n, t->view.key_bits);
    const ull words = (1ull << t->view.prefix_bits) + 1;
    void* index = nullptr;
    hipError_t e = hipMalloc(&index, words * sizeof(uint32_t));
    if (e == hipSuccess) {
        t->view.index = static_cast<uint32_t*>(index);
        hipLaunchKernelGGL(index_fill_kernel, dim3((unsigned)((words + LTPB - 1) / LTPB)), dim3(LTPB), 0, s, t->view, static_cast<uint32_t*>(index));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

namespace {

struct SatAdd {
    __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const
    {
        const uint32_t s = a + b;
        return s < a ? 0xffffffffu : s;
    }
};

using blh::hip_rc;
using blh::invalid;
using blh::misaligned16;
using blh::round16;
// the grid of the one-thread-per-key kernels, which stride: at most TABLE_GRID_MAX workgroups
unsigned capped_blocks_for(ull n) { return n > (ull)TABLE_GRID_MAX * LTPB ? (unsigned)TABLE_GRID_MAX : blh::blocks_for(n, LTPB); }

// KeyT: unsigned long long or __uint128_t — what rocPRIM sorts; the bytes are the table's
template <typename KeyT>
int build(bl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_counts, uint64_t n, uint32_t key_bits, bl_table** out)
{
    constexpr uint32_t W = sizeof(KeyT) / 8;
    if (!ctx || !out || (n && !d_keys) || key_bits < 1 || key_bits > 64 * W) return invalid(W == 2 ? "bad argument (1 <= key_bits <= 128)" : "bad argument (1 <= key_bits <= 64)");
    *out = nullptr;
    if (W == 2 && n && misaligned16(d_keys)) return invalid("arrays of 16-byte keys must be 16-byte aligned");
    if (n >= (1ull << 32)) return invalid("a count table takes fewer than 2^32 entries");
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);

    ull distinct = 0;
    KeyT* merged = nullptr;  // slot 4: the distinct keys and their counts
    uint32_t* merged_c = nullptr;
    if (n) {
        ull* d_words = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 64));  // [0] OR of low words, [1] OR of high words, [2] distinct keys
        if (!d_words) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        // the key_bits promise, before the sort that relies on it
        ull host[3] = {0, 0, 0};
        BLH_TRY(hipMemsetAsync(d_words, 0, 3 * sizeof(ull), s));
        hipLaunchKernelGGL(or_reduce_kernel, dim3(capped_blocks_for(n)), dim3(LTPB), 0, s, d_keys, (ull)n, W, d_words);
        BLH_TRY(hipGetLastError());
        BLH_TRY(hipMemcpyAsync(host, d_words, 2 * sizeof(ull), hipMemcpyDeviceToHost, s));
        BLH_TRY(hipStreamSynchronize(s));
        if (above_key_bits(host[0], host[1], key_bits)) return invalid("a key has a bit set at or above key_bits");

        // slot 4: sorted keys | merged keys | sorted counts | merged counts
        const size_t kb = round16((size_t)n * sizeof(KeyT)), cb = round16((size_t)n * sizeof(uint32_t));
        unsigned char* data = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 4, 2 * kb + 2 * cb));
        if (!data) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        KeyT* sorted = reinterpret_cast<KeyT*>(data);
        merged = reinterpret_cast<KeyT*>(data + kb);
        uint32_t* sorted_c = reinterpret_cast<uint32_t*>(data + 2 * kb);
        merged_c = reinterpret_cast<uint32_t*>(data + 2 * kb + cb);
        const KeyT* in = reinterpret_cast<const KeyT*>(d_keys);
        const rocprim::constant_iterator<uint32_t> ones(1u);
        // slot 5 for both, one after the other: the stream orders them
        BLH_TRY(blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) {
            if (d_counts) return rocprim::radix_sort_pairs(ws, bytes, in, sorted, d_counts, sorted_c, (size_t)n, 0u, key_bits, s);
            return rocprim::radix_sort_pairs(ws, bytes, in, sorted, ones, sorted_c, (size_t)n, 0u, key_bits, s);
        }));
        BLH_TRY(blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) {
            return rocprim::reduce_by_key(ws, bytes, sorted, sorted_c, (size_t)n, merged, merged_c, d_words + 2, SatAdd(), rocprim::equal_to<KeyT>(), s);
        }));
        BLH_TRY(hipMemcpyAsync(&distinct, d_words + 2, sizeof(ull), hipMemcpyDeviceToHost, s));
        BLH_TRY(hipStreamSynchronize(s));
        if (distinct == 0 || distinct > n) return bl_set_error(BL_ERR_INTERNAL, "reduce_by_key returned an impossible number of keys");
    }
    bl_table* t = nullptr;
    const int rc = new_table(ctx, W, key_bits, distinct, &t);
    if (rc != BL_OK) return rc;
    hipError_t e = hipSuccess;
    if (distinct) {
        e = hipMemcpyAsync(const_cast<uint64_t*>(t->view.keys), merged, (size_t)distinct * sizeof(KeyT), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(const_cast<uint32_t*>(t->view.counts), merged_c, (size_t)distinct * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { free_table(t); return hip_rc(e); }
    }
    e = finish_table(ctx, t, s);
    if (e != hipSuccess) { free_table(t); return hip_rc(e); }
    *out = t;
    return BL_OK;
}

int lookup(bl_ctx* ctx, const bl_table* t, const uint64_t* d_queries, uint64_t n, uint32_t* d_out, uint32_t key_words)
{
    if (!ctx || !t || (n && (!d_queries || !d_out))) return invalid("NULL argument");
    BLH_OK(blh::table_owner(t->ctx, ctx));
    if (t->view.key_words != key_words) return invalid(key_words == 2 ? "bl_table_lookup_u128 takes a table of two-word keys" : "bl_table_lookup_u64 takes a table of one-word keys");
    if (n == 0) return BL_OK;
    if (key_words == 2 && misaligned16(d_queries)) return invalid("arrays of 16-byte keys must be 16-byte aligned");
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    const ull groups = (n + (ull)LTPB * G - 1) / ((ull)LTPB * G);
    hipLaunchKernelGGL(lookup_kernel, dim3((unsigned)(groups < LOOKUP_GRID_MAX ? groups : LOOKUP_GRID_MAX)), dim3(LTPB), 0, s, t->view, d_queries, (ull)n, d_out);
    BLH_TRY(hipGetLastError());
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}

}  // namespace

}  // namespace bllk

extern "C" {

int bl_table_build_u64(bl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_counts, uint64_t n, uint32_t key_bits, bl_table** out)
{
    return bllk::build<unsigned long long>(ctx, d_keys, d_counts, n, key_bits, out);
}

int bl_table_build_u128(bl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_counts, uint64_t n, uint32_t key_bits, bl_table** out)
{
    return bllk::build<__uint128_t>(ctx, d_keys, d_counts, n, key_bits, out);
}

int bl_table_destroy(bl_table* t)
{
    if (!t) return BL_OK;
    (void)hipSetDevice(t->device);
    bllk::free_table(t);  // (hipFree waits for the device: a scan still reading the table has finished)
    return BL_OK;
}

int bl_table_info(const bl_table* t, uint64_t* n_distinct, uint32_t* key_words, uint32_t* key_bits, uint32_t* prefix_bits)
{
    if (!t) return blh::invalid("table is NULL");
    if (n_distinct) *n_distinct = t->view.n;
    if (key_words) *key_words = t->view.key_words;
    if (key_bits) *key_bits = t->view.key_bits;
    if (prefix_bits) *prefix_bits = t->view.prefix_bits;
    return BL_OK;
}

int bl_table_arrays(const bl_table* t, const uint64_t** d_keys, const uint32_t** d_counts)
{
    if (!t) return blh::invalid("table is NULL");
    if (d_keys) *d_keys = t->view.keys;
    if (d_counts) *d_counts = t->view.counts;
    return BL_OK;
}

int bl_table_lookup_u64(bl_ctx* ctx, const bl_table* t, const uint64_t* d_queries, uint64_t n, uint32_t* d_counts_out)
{
    return bllk::lookup(ctx, t, d_queries, n, d_counts_out, 1);
}

int bl_table_lookup_u128(bl_ctx* ctx, const bl_table* t, const uint64_t* d_queries, uint64_t n, uint32_t* d_counts_out)
{
    return bllk::lookup(ctx, t, d_queries, n, d_counts_out, 2);
}

int bl_table_histogram(bl_ctx* ctx, const bl_table* t, uint64_t* hist, uint32_t n_bins)
{
    using namespace bllk;
    if (!ctx || !t || !hist || n_bins < 1 || n_bins > 65536) return invalid("bad argument (1 <= n_bins <= 65536)");
    BLH_OK(blh::table_owner(t->ctx, ctx));
    for (uint32_t b = 0; b < n_bins; ++b) hist[b] = 0;
    const uint32_t n = t->view.n;
    if (n == 0) return BL_OK;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    ull* d_hist = static_cast<ull*>(bl_ctx_scratch(ctx, 6, (size_t)n_bins * sizeof(ull)));
    if (!d_hist) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    BLH_TRY(hipMemsetAsync(d_hist, 0, (size_t)n_bins * sizeof(ull), s));
    if (n_bins <= (uint32_t)HIST_LDS_BINS) {
        // a workgroup clears and flushes n_bins words: give it at least that many keys
        const ull per = n_bins > HIST_LDS_KEYS_MIN ? n_bins : HIST_LDS_KEYS_MIN;
        const ull wg = (n + per - 1) / per;
        hipLaunchKernelGGL(histogram_lds_kernel, dim3((unsigned)(wg < HIST_LDS_GRID_MAX ? wg : HIST_LDS_GRID_MAX)), dim3(LTPB), 0, s, t->view.counts, n, n_bins, d_hist);
    } else {
        hipLaunchKernelGGL(histogram_global_kernel, dim3(capped_blocks_for(n)), dim3(LTPB), 0, s, t->view.counts, n, n_bins, d_hist);
    }
    BLH_TRY(hipGetLastError());
    static_assert(sizeof(ull) == sizeof(uint64_t), "the device bins are the caller's words");
    BLH_TRY(hipMemcpyAsync(hist, d_hist, (size_t)n_bins * sizeof(ull), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}

}  // extern "C"
