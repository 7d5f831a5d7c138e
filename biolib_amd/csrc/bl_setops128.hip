// bl_setops128.hip — the consumer side of the pipeline for 16-byte keys (k-mers of 33 <= k <= 64, kmer_view<__uint128_t>): sort,
// unique, run-length count, owner split, the device half of the run-file calls, and the sizes of intersection / union of two sorted
// unique sets.  As in bl_setops.hip the host bodies are bl_keylist.hpp's, instantiated here for __uint128_t (rocPRIM device
// primitives: library plumbing); the owner split is blpart::partition with a 16-byte element.  Hand-written: the two intersection
// kernels, whose per-thread bodies live in bl_setops128_core.hpp —
//   merge kernel    merge path: one thread per tile boundary finds the tile's split in global memory (merge_partition_kernel); one
//                   workgroup per tile of 2048 merged elements stages its A range and its B range plus ONE more B element in LDS with
//                   16-byte accesses, every thread merges 8 elements from its own diagonal and counts the equal pairs
//                   (merge_tile_kernel).  Every key is read from HBM once.
//   search kernel   every key of the smaller set binary-searches the larger one: log2(n_large) dependent 16-byte loads per key, the
//                   better form when the sets differ much in size.
// The context option "jaccard128_path" forces one of them (1 merge, 2 search); 0 chooses by the size ratio (bl128s::choose_merge).
#include <hip/hip_runtime.h>

#include "../../include/biolib_amd.h"
#include "bl_keylist.hpp"
#include "bl_kmers128_core.hpp"
#include "bl_setops128_core.hpp"

namespace {

using bl128s::Key;
using bl128s::TILE;
using bl128s::TPB;
typedef unsigned long long ull;

static_assert(sizeof(Key) == 16 && sizeof(__uint128_t) == 16, "a key is the object representation of __uint128_t");

// splits[t] = A elements in front of diagonal min(t * TILE, na + nb), t = 0 .. n_tiles
__global__ __launch_bounds__(TPB) void merge_partition_kernel(const Key* __restrict__ a, ull na, const Key* __restrict__ b, ull nb, ull n_tiles, ull* __restrict__ splits)
{
    const ull t = (ull)blockIdx.x * TPB + threadIdx.x;
    if (t > n_tiles) return;
    const ull total = na + nb;
    const ull d = t * (ull)TILE < total ? t * (ull)TILE : total;
    splits[t] = bl128s::diag_split<ull>(a, na, b, nb, d);
}

// per wave, then one atomic per workgroup (integer sums: the order does not matter)
__device__ __forceinline__ void block_add(uint32_t found, ull* out)
{
    __shared__ uint32_t wave_sum[TPB / 64];
    for (int d = 32; d >= 1; d >>= 1) found += __shfl_xor(found, d, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = found;
    __syncthreads();
    if (threadIdx.x == 0) {
        ull sum = 0;
        for (int w = 0; w < TPB / 64; ++w) sum += wave_sum[w];
        if (sum) atomicAdd(out, sum);
    }
}

__global__ __launch_bounds__(TPB) void merge_tile_kernel(const Key* __restrict__ a, ull na, const Key* __restrict__ b, ull nb, const ull* __restrict__ splits, ull* out)
{
    __shared__ Key keys[bl128s::LDS_KEYS];
    const bl128s::TileRange r = bl128s::tile_range(splits, blockIdx.x, na, nb);
    for (uint32_t x = threadIdx.x; x < r.la; x += TPB) keys[x] = a[r.a0 + x];
    for (uint32_t x = threadIdx.x; x < r.lbx; x += TPB) keys[r.la + x] = b[r.b0 + x];
    __syncthreads();
    const uint32_t found = bl128s::tile_thread_count(keys, r.la, keys + r.la, r.lb, r.lbx, threadIdx.x);
    block_add(found, out);
}

__global__ __launch_bounds__(TPB) void search_count_kernel(const Key* __restrict__ a, ull na, const Key* __restrict__ b, ull nb, ull* out)
{
    uint32_t found = 0;
    for (ull i = (ull)blockIdx.x * TPB + threadIdx.x; i < na; i += (ull)gridDim.x * TPB) found += bl128s::search_count(a[i], b, nb);
    block_add(found, out);
}

struct Key128HashOwner {
    const Key* keys;
    uint32_t seed;
    __device__ uint32_t operator()(ull i, uint32_t parts) const
    {
        const Key k = keys[i];
        return blpart::bucket_of(bl::murmur64_u128(k.lo, k.hi, seed), parts);
    }
};

using blh::hip_rc;
using blkeys::bad_alignment;
using blh::misaligned16;

int bad_key_bits() { return bl_set_error(BL_ERR_INVALID, "bad argument (1 <= key_bits <= 128)"); }
__uint128_t* as_keys(uint64_t* p) { return reinterpret_cast<__uint128_t*>(p); }
const __uint128_t* as_keys(const uint64_t* p) { return reinterpret_cast<const __uint128_t*>(p); }

}  // namespace

extern "C" {

int bl_sort_u128(bl_ctx* ctx, uint64_t* d_keys, uint64_t n, uint32_t key_bits)
{
    if (!ctx || (n && !d_keys) || key_bits < 1 || key_bits > 128) return bad_key_bits();
    if (n == 0) return BL_OK;
    if (misaligned16(d_keys)) return bad_alignment();
    return blkeys::sort_keys(ctx, as_keys(d_keys), n, key_bits);
}

int bl_sort_unique_u128(bl_ctx* ctx, uint64_t* d_keys, uint64_t n, uint32_t key_bits, uint64_t* n_unique)
{
    if (!ctx || !n_unique || (n && !d_keys) || key_bits < 1 || key_bits > 128) return bad_key_bits();
    *n_unique = 0;
    if (n == 0) return BL_OK;
    if (misaligned16(d_keys)) return bad_alignment();
    return blkeys::sort_unique(ctx, as_keys(d_keys), n, key_bits, n_unique);
}

int bl_count_sorted_u128(bl_ctx* ctx, const uint64_t* d_sorted, uint64_t n, uint64_t* d_unique, uint32_t* d_counts, uint64_t* n_unique)
{
    if (!ctx || !n_unique || (n && (!d_sorted || !d_unique || !d_counts))) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    *n_unique = 0;
    if (n == 0) return BL_OK;
    if (misaligned16(d_sorted) || misaligned16(d_unique)) return bad_alignment();
    return blkeys::count_sorted(ctx, as_keys(d_sorted), n, as_keys(d_unique), d_counts, n_unique);
}

int bl_jaccard_sorted_u128(bl_ctx* ctx, const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* intersection, uint64_t* union_size)
{
    if (!ctx || !intersection || !union_size || (na && !d_a) || (nb && !d_b)) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    if ((na && misaligned16(d_a)) || (nb && misaligned16(d_b))) return bad_alignment();
    if (na >= (1ull << 40) || nb >= (1ull << 40)) return bl_set_error(BL_ERR_INVALID, "bl_jaccard_sorted_u128 takes fewer than 2^40 keys per set");
    if (na == 0 || nb == 0) {
        *intersection = 0;
        *union_size = na + nb;
        return BL_OK;
    }
    hipError_t e = hipSetDevice(bl_ctx_device(ctx));
    if (e != hipSuccess) return hip_rc(e);
    hipStream_t s = bl_ctx_stream(ctx);
    const Key* a = reinterpret_cast<const Key*>(d_a);
    const Key* b = reinterpret_cast<const Key*>(d_b);
    ull* d_out = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 64));
    if (!d_out) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    e = hipMemsetAsync(d_out, 0, sizeof(ull), s);
    const int path = bl_ctx_jaccard128_path(ctx);
    const bool merge = path == 1 || (path == 0 && bl128s::choose_merge(na, nb));
    if (e == hipSuccess && merge) {
        const ull n_tiles = (na + nb + TILE - 1) / TILE;  // < 2^30
        ull* splits = static_cast<ull*>(bl_ctx_scratch(ctx, 5, (n_tiles + 1) * sizeof(ull)));
        if (!splits) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        hipLaunchKernelGGL(merge_partition_kernel, dim3((unsigned)((n_tiles + 1 + TPB - 1) / TPB)), dim3(TPB), 0, s, a, (ull)na, b, (ull)nb, n_tiles, splits);
        hipLaunchKernelGGL(merge_tile_kernel, dim3((unsigned)n_tiles), dim3(TPB), 0, s, a, (ull)na, b, (ull)nb, splits, d_out);
        e = hipGetLastError();
    } else if (e == hipSuccess) {
        // search the larger set with the elements of the smaller one
        const bool a_small = na <= nb;
        const Key* x = a_small ? a : b;
        const Key* y = a_small ? b : a;
        const ull nx = a_small ? na : nb, ny = a_small ? nb : na;
        const unsigned blocks = (unsigned)((nx + TPB - 1) / TPB < 256 * 16 ? (nx + TPB - 1) / TPB : 256 * 16);
        hipLaunchKernelGGL(search_count_kernel, dim3(blocks), dim3(TPB), 0, s, x, nx, y, ny, d_out);
        e = hipGetLastError();
    }
    ull inter = 0;
    if (e == hipSuccess) e = blkeys::read_counter(d_out, s, &inter);
    if (e != hipSuccess) return hip_rc(e);
    *intersection = inter;
    *union_size = na + nb - inter;
    return BL_OK;
}

int bl_partition_u128(bl_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t parts, uint64_t seed, uint64_t* d_out, uint64_t* counts)
{
    if (!ctx || !counts || parts == 0 || parts > blpart::MAX_PARTS || (n && (!d_keys || !d_out))) return bl_set_error(BL_ERR_INVALID, "bad argument (1 <= parts <= 64)");
    if (n && (misaligned16(d_keys) || misaligned16(d_out))) return bad_alignment();
    const Key* keys = reinterpret_cast<const Key*>(d_keys);
    return blkeys::partition_keys(ctx, keys, n, parts, Key128HashOwner{keys, (uint32_t)seed}, reinterpret_cast<Key*>(d_out), counts);
}

int bl_read_file_u128(bl_ctx* ctx, const char* path, int with_count, uint64_t* d_out, uint64_t capacity, uint64_t* n)
{
    if (!ctx || !path) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    return blkeys::read_file(ctx, path, with_count, as_keys(d_out), capacity, n);
}

int bl_merge_runs_u128(bl_ctx* ctx, const char* const* paths, uint32_t n_paths, uint64_t* d_out, uint64_t capacity, uint64_t* n_total)
{
    if (!ctx || (n_paths && !paths) || !n_total) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    return blkeys::merge_runs(ctx, paths, n_paths, as_keys(d_out), capacity, n_total);
}

}  // extern "C"
