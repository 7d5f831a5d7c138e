// bl_setops.hip — what happens to k-mers right after the scan in biolib's own consumer
// (tests/test_jaccard.cpp:55-130 in the reference tree), for 8-byte keys: sort, unique, run-length count, owner
// split, the device half of the run-file calls, and the sizes of intersection / union of two sorted unique sets
// (include/ordered_unique_sampler.hpp:115-130, include/jaccard.hpp:8-37).  The host bodies are bl_keylist.hpp's, instantiated here
// for unsigned long long (rocPRIM device primitives: plain library plumbing, like a BLAS GEMM would be); the set intersection is a
// hand-written merge-path-free kernel: every element of the smaller... of A binary-searches B (both unique and sorted).
#include <hip/hip_runtime.h>

#include "../../include/biolib_amd.h"
#include "bl_keylist.hpp"
#include "bl_scan_core.hpp"

namespace {

typedef unsigned long long ull;

__global__ void intersect_count_kernel(const unsigned long long* a, unsigned long long na, const unsigned long long* b, unsigned long long nb,
                                       unsigned long long* out)
{
    unsigned long long local = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < na; i += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long key = a[i];
        unsigned long long lo = 0, hi = nb;  // first element of b that is >= key
        while (lo < hi) {
            const unsigned long long mid = (lo + hi) >> 1;
            if (b[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        local += (lo < nb && b[lo] == key) ? 1 : 0;
    }
    for (int d = 32; d >= 1; d >>= 1) local += __shfl_xor(local, d, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(out, local);
}

// the owner GPU of a k-mer in the multi-GPU bucket exchange: hash64(key, seed) % parts
struct KeyHashOwner {
    const unsigned long long* keys;
    uint32_t seed;
    __device__ uint32_t operator()(unsigned long long i, uint32_t parts) const { return blpart::bucket_of(bl::murmur64(keys[i], seed), parts); }
};

ull* as_keys(uint64_t* p) { return reinterpret_cast<ull*>(p); }
const ull* as_keys(const uint64_t* p) { return reinterpret_cast<const ull*>(p); }

}  // namespace

extern "C" {

int bl_sort_u64(bl_ctx* ctx, uint64_t* d_keys, uint64_t n)
{
    if (!ctx || (n && !d_keys)) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    return n ? blkeys::sort_keys(ctx, as_keys(d_keys), n, 64) : BL_OK;
}

int bl_sort_unique_u64(bl_ctx* ctx, uint64_t* d_keys, uint64_t n, uint64_t* n_unique)
{
    if (!ctx || !n_unique || (n && !d_keys)) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    *n_unique = 0;
    return n ? blkeys::sort_unique(ctx, as_keys(d_keys), n, 64, n_unique) : BL_OK;
}

int bl_count_sorted_u64(bl_ctx* ctx, const uint64_t* d_sorted, uint64_t n, uint64_t* d_unique, uint32_t* d_counts, uint64_t* n_unique)
{
    if (!ctx || !n_unique || (n && (!d_sorted || !d_unique || !d_counts))) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    *n_unique = 0;
    return n ? blkeys::count_sorted(ctx, as_keys(d_sorted), n, as_keys(d_unique), d_counts, n_unique) : BL_OK;
}

int bl_jaccard_sorted_u64(bl_ctx* ctx, const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* intersection,
                          uint64_t* union_size)
{
    if (!ctx || !intersection || !union_size || (na && !d_a) || (nb && !d_b)) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    unsigned long long* d_out = static_cast<unsigned long long*>(bl_ctx_scratch(ctx, 6, 64));
    if (!d_out) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    hipError_t e = hipMemsetAsync(d_out, 0, sizeof(unsigned long long), s);
    // search the larger set with the elements of the smaller one
    const bool a_small = na <= nb;
    const unsigned long long* x = as_keys(a_small ? d_a : d_b);
    const unsigned long long* y = as_keys(a_small ? d_b : d_a);
    const unsigned long long nx = a_small ? na : nb, ny = a_small ? nb : na;
    if (e == hipSuccess && nx && ny) {
        const unsigned blocks = (unsigned)((nx + 255) / 256 < 256 * 16 ? (nx + 255) / 256 : 256 * 16);
        hipLaunchKernelGGL(intersect_count_kernel, dim3(blocks), dim3(256), 0, s, x, nx, y, ny, d_out);
        e = hipGetLastError();
    }
    unsigned long long inter = 0;
    if (e == hipSuccess) e = blkeys::read_counter(d_out, s, &inter);
    if (e != hipSuccess) return bl_set_error(BL_ERR_HIP, hipGetErrorString(e));
    *intersection = inter;
    *union_size = na + nb - inter;
    return BL_OK;
}

int bl_partition_u64(bl_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t parts, uint64_t seed, uint64_t* d_out, uint64_t* counts)
{
    if (!ctx || !counts || parts == 0 || parts > blpart::MAX_PARTS || (n && (!d_keys || !d_out))) return bl_set_error(BL_ERR_INVALID, "bad argument (1 <= parts <= 64)");
    return blkeys::partition_keys(ctx, as_keys(d_keys), n, parts, KeyHashOwner{as_keys(d_keys), (uint32_t)seed}, as_keys(d_out), counts);
}

int bl_read_file_u64(bl_ctx* ctx, const char* path, int with_count, uint64_t* d_out, uint64_t capacity, uint64_t* n)
{
    if (!ctx || !path) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    return blkeys::read_file(ctx, path, with_count, as_keys(d_out), capacity, n);
}

int bl_merge_runs_u64(bl_ctx* ctx, const char* const* paths, uint32_t n_paths, uint64_t* d_out, uint64_t capacity, uint64_t* n_total)
{
    if (!ctx || (n_paths && !paths) || !n_total) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    return blkeys::merge_runs(ctx, paths, n_paths, as_keys(d_out), capacity, n_total);
}

}  // extern "C"
