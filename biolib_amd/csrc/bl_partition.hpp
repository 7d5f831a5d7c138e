// bl_partition.hpp — bucket split of a device array by an owner function (the routing step of the multi-GPU counter).
// Two passes, no global atomics: (1) every block of 4096 items builds its histogram in LDS and writes it to
// hist[bucket][block]; an exclusive scan over that bucket-major table gives every (bucket, block) pair its output
// offset; (2) every block scatters its items behind LDS cursors that start at those offsets.  Buckets come out
// contiguous and in bucket order; the order inside a bucket is by block, arbitrary inside a block.
// (The first version used one global atomic cursor per bucket: 142 M atomics on 8 addresses, 560 ms per 1.5 Gbp.)
#pragma once
#include <hip/hip_runtime.h>

#include "bl_host.hpp"

namespace blpart {

constexpr int MAX_PARTS = 64;
constexpr int PT = 256;         // threads per block
constexpr int ITEMS = 16;       // items per thread
constexpr int CHUNK = PT * ITEMS;

__device__ __forceinline__ uint32_t bucket_of(unsigned long long h, uint32_t parts) { return (parts & (parts - 1)) == 0 ? (uint32_t)h & (parts - 1) : (uint32_t)(h % parts); }

template <typename Owner>
__global__ __launch_bounds__(PT) void hist_kernel(Owner owner, unsigned long long n, uint32_t parts, unsigned long long n_blocks, unsigned long long* hist)
{
    __shared__ unsigned int h[MAX_PARTS];
    if (threadIdx.x < MAX_PARTS) h[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long base = (unsigned long long)blockIdx.x * CHUNK;
#pragma unroll 4
    for (int j = 0; j < ITEMS; ++j) {
        const unsigned long long i = base + (unsigned long long)j * PT + threadIdx.x;
        if (i < n) atomicAdd(&h[owner(i, parts)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < parts) hist[(unsigned long long)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

template <typename T, typename Owner>
__global__ __launch_bounds__(PT) void scatter_kernel(const T* __restrict__ src, Owner owner, unsigned long long n, uint32_t parts, unsigned long long n_blocks,
                                                     const unsigned long long* __restrict__ offset, T* __restrict__ dst)
{
    __shared__ unsigned long long start[MAX_PARTS];
    __shared__ unsigned int cursor[MAX_PARTS];
    if (threadIdx.x < parts) {
        start[threadIdx.x] = offset[(unsigned long long)threadIdx.x * n_blocks + blockIdx.x];
        cursor[threadIdx.x] = 0;
    }
    __syncthreads();
    const unsigned long long base = (unsigned long long)blockIdx.x * CHUNK;
#pragma unroll 4
    for (int j = 0; j < ITEMS; ++j) {
        const unsigned long long i = base + (unsigned long long)j * PT + threadIdx.x;
        if (i < n) {
            const uint32_t b = owner(i, parts);
            const unsigned int r = atomicAdd(&cursor[b], 1u);
            dst[start[b] + r] = src[i];
        }
    }
}

// starts[b] = offset of bucket b (= offset[b][0]); starts[parts] = n
static __global__ void starts_kernel(const unsigned long long* offset, unsigned long long n_blocks, uint32_t parts, unsigned long long n, unsigned long long* starts)
{
    const uint32_t b = threadIdx.x;
    if (b < parts) starts[b] = offset[(unsigned long long)b * n_blocks];
    if (b == parts) starts[b] = n;
}

// counts: host array of `parts` entries.  Scratch slot 4 holds the histogram, the offsets and the bucket starts, slot 5 the workspace of
// the scan (blh::exclusive_sum): the caller holds neither.  Returns a BL_* code.
template <typename T, typename Owner>
int partition(bl_ctx* ctx, const T* d_src, unsigned long long n, uint32_t parts, Owner owner, T* d_dst, uint64_t* counts, hipStream_t s)
{
    for (uint32_t b = 0; b < parts; ++b) counts[b] = 0;
    if (n == 0) return BL_OK;
    const unsigned long long n_blocks = (n + CHUNK - 1) / CHUNK;
    const size_t cells = (size_t)parts * n_blocks;
    unsigned long long* d_hist = static_cast<unsigned long long*>(bl_ctx_scratch(ctx, 4, (2 * cells + MAX_PARTS + 1) * sizeof(unsigned long long)));
    if (!d_hist) return blh::hip_rc(hipErrorOutOfMemory);
    unsigned long long *d_off = d_hist + cells, *d_starts = d_off + cells;
    hipLaunchKernelGGL((hist_kernel<Owner>), dim3((unsigned)n_blocks), dim3(PT), 0, s, owner, n, parts, n_blocks, d_hist);
    const int rc = blh::exclusive_sum(ctx, reinterpret_cast<const uint64_t*>(d_hist), reinterpret_cast<uint64_t*>(d_off), cells, s);
    if (rc != BL_OK) return rc;
    hipLaunchKernelGGL((scatter_kernel<T, Owner>), dim3((unsigned)n_blocks), dim3(PT), 0, s, d_src, owner, n, parts, n_blocks, d_off, d_dst);
    hipLaunchKernelGGL(starts_kernel, dim3(1), dim3(MAX_PARTS + 1), 0, s, d_off, n_blocks, parts, n, d_starts);
    BLH_TRY(hipGetLastError());
    unsigned long long starts[MAX_PARTS + 1] = {0};
    BLH_TRY(hipMemcpyAsync(starts, d_starts, (parts + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    for (uint32_t b = 0; b < parts; ++b) counts[b] = starts[b + 1] - starts[b];
    return BL_OK;
}

}  // namespace blpart
