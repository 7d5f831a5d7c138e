// Super-k-mer records and the exact bucketed k-mer counter for k up to 64 (bl_pack_super_kmers128, bl_partition_records128,
// bl_expand_super_kmers128, bl_count_super_kmers128).  The 64-bit calls and their 16-byte record live in bl_superkmer.hip and are
// untouched; this file is the same pipeline over a 32-byte record (bl_superkmer128_core.hpp) and 128-bit k-mers:
//
//   1. bucket_id128_kernel   per record: the minimizer m-mer found again through mm_pos, hashed as the scan hashed it (8-byte key);
//                            bucket = 32 mixed bits of that hash scaled to the number of buckets (~BUCKET_RECS records each)
//   2. rocprim::radix_sort_pairs (bucket id -> record INDEX): the 32-byte records stay where they are and are read through the
//                            sorted index (a stable sort: a bucket's records keep their input order)
//   3. bucket_starts128_kernel
//   4. count128_kernel<false>  one WAVE per bucket: the bucket's k-mers go into the wave's LDS table (owner word + two key words +
//                            16-bit count per slot, protocol in bl_superkmer128_core.hpp) in rounds of up to 64 records / CT128_CAP
//                            k-mers; the number of distinct k-mers is kept.  A bucket that may come to hold more than CT128_FULL
//                            distinct k-mers, or holds more than CT128_MAXREC records, is listed for the fallback
//   5. exclusive scan of those numbers = where every bucket writes
//   6. count128_kernel<true>   the tables are built again and written out at the buckets' offsets — only once the caller's capacity
//                            is known to hold everything (nothing is written otherwise)
//   7. fallback              records of the listed buckets: gather -> expand -> 128-bit radix sort -> run-length encode -> appended.
//                            The fallback has no table and no reserved key value; with the context option "count128_tables" = 0 it
//                            counts the whole input.
// The table has no empty KEY either (the owner word marks empty slots), so k = 64 without the canonical flag — where the all-T 64-mer
// is all ones in both words — takes the tables like any other call.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <vector>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"
#include "bl_partition.hpp"
#include "bl_superkmer128_core.hpp"

namespace {

using bl::CT128_CAP;
using bl::CT128_FULL;
using bl::CT128_MAXREC;
using bl::CT128_SLOTS;
using bl::CT128_WAVES;
using bl::U64x2;
using bl::WaveTable128;

constexpr int MAX_PARTS = 64;
constexpr const char* LIMITS = "need 1 <= m <= 32, m <= k <= 64, k - m + 1 <= 64 and 2k - m <= 122 (bases per 32-byte record)";

bool shape_ok(uint32_t k, uint32_t m) { return m >= 1 && m <= 32 && k >= m && k <= 64 && k - m + 1 <= 64 && 2 * k - m <= (uint32_t)bl::SK128_MAX_BASES; }

struct alignas(32) Rec32 {
    unsigned long long w[4];
};

__global__ __launch_bounds__(256) void pack128_kernel(const unsigned char* __restrict__ bases, unsigned long long n_bases,
                                                      const unsigned long long* __restrict__ first_pos, const unsigned char* __restrict__ sizes,
                                                      const unsigned char* __restrict__ mm_pos, unsigned long long n, int k, Rec32* __restrict__ out,
                                                      unsigned long long origin)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    uint64_t w[4];
    bl::sk128_pack(bases, n_bases, first_pos[g] - origin, (int)sizes[g], (int)mm_pos[g], k, w);
    Rec32 r;
    r.w[0] = w[0]; r.w[1] = w[1]; r.w[2] = w[2]; r.w[3] = w[3];
    out[g] = r;
}

struct HashArrayOwner {
    const unsigned long long* hashes;
    __device__ uint32_t operator()(unsigned long long i, uint32_t parts) const { return blpart::bucket_of(hashes[i], parts); }
};

__global__ void sizes128_kernel(const Rec32* recs, unsigned long long n, unsigned long long* sizes)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) sizes[g] = (unsigned long long)bl::sk128_size(recs[g].w[3]);
}

__global__ __launch_bounds__(256) void expand128_kernel(const Rec32* __restrict__ recs, const unsigned long long* __restrict__ offsets, unsigned long long n, int k,
                                                        int canonical, unsigned long long* __restrict__ out)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const Rec32 r = recs[g];
    bl::sk128_expand(r.w[0], r.w[1], r.w[2], r.w[3], k, canonical != 0, reinterpret_cast<uint64_t*>(out + 2 * offsets[g]));
}

__global__ __launch_bounds__(256) void bucket_id128_kernel(const Rec32* __restrict__ recs, uint32_t n, int m, int canonical, uint32_t seed, uint32_t n_buckets,
                                                           uint32_t* __restrict__ ids, uint32_t* __restrict__ index)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const Rec32 r = recs[g];
    const unsigned long long h = bl::sk128_minimizer_hash(r.w[0], r.w[1], r.w[2], r.w[3], m, canonical != 0, seed);
    // 32 well-mixed bits of the hash, scaled to [0, n_buckets): independent of the low bits that pick the owner rank
    ids[g] = (uint32_t)((((h * 0x9E3779B97F4A7C15ULL) >> 32) * (unsigned long long)n_buckets) >> 32);
    index[g] = g;
}

// starts[b] = first position of the sorted ids holding a value >= b, for b = 0 .. n_buckets
__global__ __launch_bounds__(256) void bucket_starts128_kernel(const uint32_t* __restrict__ ids, uint32_t n, uint32_t n_buckets, uint32_t* __restrict__ starts)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_buckets) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    starts[b] = lo;
}

// lanes of a wave see each other's LDS writes once the compiler keeps the program order (LDS traffic of one wave is served in issue
// order): a wavefront-scope fence, no s_barrier, no other wave involved
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned int wave_incl_scan(unsigned int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ void list_overflow(int lane, uint32_t lo, uint32_t hi, unsigned long long* cursor, uint2* overflow, uint32_t max_overflow)
{
    if (lane == 0) {
        const unsigned long long slot = atomicAdd(&cursor[0], 1ULL);
        if (slot < max_overflow) overflow[slot] = make_uint2(lo, hi);
    }
}

// One bucket, one wave: sorted positions [lo, hi).  Everything that steers control flow here is wave-uniform (ballots and shuffles of
// the lanes' values), so every wave_lds_sync is reached by the whole wave.  Returns false when the bucket is the fallback's.
// WRITE: the second pass — same records, same order, same decisions; it lists nothing and writes the table out at `off`.
template <bool WRITE>
__device__ __forceinline__ bool count_one_bucket128(WaveTable128& t, int lane, uint32_t lo, uint32_t hi, const Rec32* __restrict__ recs,
                                                    const uint32_t* __restrict__ perm, int k, bool canonical, unsigned int& d_out, unsigned long long off,
                                                    U64x2* __restrict__ out_keys, unsigned int* __restrict__ out_counts)
{
    d_out = 0;
    const uint32_t n_rec = hi - lo;
    if (n_rec == 0) return true;
    if (n_rec > (uint32_t)CT128_MAXREC) return false;  // more occurrences than a 16-bit count holds
    wave_lds_sync();  // the previous bucket's table has been read out
#pragma unroll
    for (int i = 0; i < CT128_SLOTS / 64; ++i) {
        t.owner[i * 64 + lane] = 0;
        if (i < CT128_SLOTS / 128) t.cnt[i * 64 + lane] = 0;
    }
    unsigned int held = 0;  // distinct k-mers in the table (wave-uniform)
    for (uint32_t at = lo; at < hi;) {
        const bool mine = at + (uint32_t)lane < hi;
        Rec32 rec = {};
        if (mine) rec = recs[perm[at + lane]];
        const unsigned int size = mine ? (unsigned int)bl::sk128_size(rec.w[3]) : 0u;
        const unsigned int incl = wave_incl_scan(size, lane);
        // the records of this round: the longest prefix whose k-mers fit the work list (sizes are <= 64: at least 10 records)
        const unsigned long long fits = __ballot(size != 0 && incl <= (unsigned int)CT128_CAP);
        const int n_take = (int)__popcll(fits);  // >= 1; a prefix of the lanes, since incl only grows
        const unsigned int total = __shfl(incl, n_take - 1, 64);
        if (held + total > (unsigned int)CT128_FULL) return false;  // the table might fill up (every k-mer of the round may be new)
        wave_lds_sync();  // the round before has read its records and its work list
        if (lane < n_take) {
            bl::table128_stage(t, lane, rec.w[0], rec.w[1], rec.w[2], rec.w[3]);
            const unsigned int first = incl - size;
            for (unsigned int q = 0; q < size; ++q) t.work[first + q] = (unsigned short)((lane << 6) | q);
        }
        wave_lds_sync();
        unsigned int fresh = 0;
        for (unsigned int base = 0; base < total; base += 64) {  // uniform trip count
            bool pending = base + lane < total;
            uint64_t klo = 0, khi = 0;
            if (pending) bl::table128_work_key(t, t.work[base + lane], k, canonical, klo, khi);
            uint32_t h = bl::table128_slot(klo, khi);
            // at most CT128_SLOTS steps by construction; the table holds < CT128_SLOTS keys, so every lane settles before that
            for (int step = 0; step < CT128_SLOTS; ++step) {
                const bool won = pending && bl::table128_claim(t, h, klo, khi);
                wave_lds_sync();
                if (pending && bl::table128_settle(t, h, klo, khi)) {
                    pending = false;
                    fresh += won ? 1u : 0u;
                }
                if (__ballot(pending) == 0ULL) break;
            }
        }
        at += (uint32_t)n_take;
        if (at < hi) held += __shfl(wave_incl_scan(fresh, lane), 63, 64);
    }
    wave_lds_sync();
    // occupied slots, 64 consecutive ones per step, ranked by ballot: the bucket's k-mers leave in slot order
    unsigned int before = 0;
    for (int i = 0; i < CT128_SLOTS / 64; ++i) {
        const uint32_t h = (uint32_t)(i * 64 + lane);
        const bool occ = t.owner[h] != 0;
        const unsigned long long occupied = __ballot(occ);
        if (WRITE && occ) {
            const unsigned int idx = before + __builtin_amdgcn_mbcnt_hi((uint32_t)(occupied >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)occupied, 0u));
            out_keys[off + idx] = U64x2{t.klo[h], t.khi[h]};
            out_counts[off + idx] = bl::table128_count(t, h);
        }
        before += (unsigned int)__popcll(occupied);
    }
    d_out = before;
    return true;
}

// Every WAVE walks its own buckets with its own table: no workgroup barrier anywhere.
template <bool WRITE>
__global__ __launch_bounds__(64 * CT128_WAVES) void count128_kernel(const Rec32* __restrict__ recs, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ starts,
                                                                     uint32_t n_buckets, int k, int canonical, unsigned int* __restrict__ distinct,
                                                                     const unsigned long long* __restrict__ offsets, U64x2* __restrict__ out_keys,
                                                                     unsigned int* __restrict__ out_counts, unsigned long long* cursor, uint2* __restrict__ overflow,
                                                                     uint32_t max_overflow)
{
    __shared__ WaveTable128 tables[CT128_WAVES];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WaveTable128& t = tables[wv];
    const uint32_t stride = gridDim.x * CT128_WAVES;
    for (uint32_t b = blockIdx.x * CT128_WAVES + wv; b < n_buckets; b += stride) {
        const uint32_t lo = __builtin_amdgcn_readfirstlane(starts[b]), hi = __builtin_amdgcn_readfirstlane(starts[b + 1]);
        unsigned int d = 0;
        const unsigned long long off = WRITE ? offsets[b] : 0ULL;
        const bool kept = count_one_bucket128<WRITE>(t, lane, lo, hi, recs, perm, k, canonical != 0, d, off, out_keys, out_counts);
        if (!WRITE) {
            if (!kept) list_overflow(lane, lo, hi, cursor, overflow, max_overflow);
            if (lane == 0) distinct[b] = kept ? d : 0u;
        }
    }
}

// records of the listed ranges of the sorted order, one range after the other: the fallback's input (one workgroup per range)
__global__ __launch_bounds__(256) void gather_ranges128_kernel(const Rec32* __restrict__ recs, const uint32_t* __restrict__ perm, const uint2* __restrict__ ranges,
                                                               const unsigned long long* __restrict__ dst_off, Rec32* __restrict__ dst)
{
    const uint2 r = ranges[blockIdx.x];
    Rec32* out = dst + dst_off[blockIdx.x];
    for (uint32_t i = r.x + threadIdx.x; i < r.y; i += blockDim.x) out[i - r.x] = recs[perm[i]];
}

__global__ void append_counted128_kernel(const __uint128_t* keys, const unsigned int* counts, unsigned long long n_runs, U64x2* out_keys, unsigned int* out_counts,
                                         unsigned long long base)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_runs) {
        out_keys[base + i] = U64x2{(uint64_t)keys[i], (uint64_t)(keys[i] >> 64)};
        out_counts[base + i] = counts[i];
    }
}

hipError_t excl_scan(bl_ctx* ctx, int tmp_slot, const unsigned long long* in, unsigned long long* out, size_t n, hipStream_t s)
{
    return blh::with_workspace(ctx, tmp_slot, [&](void* ws, size_t& bytes) { return rocprim::exclusive_scan(ws, bytes, in, out, 0ull, n, rocprim::plus<unsigned long long>(), s); });
}

// the k-mers of recs[0 .. n), group after group, to d_kmers when they fit `capacity` (nothing is written otherwise); *need = their number.
// Scratch slots 4 and 5.
hipError_t expand128(bl_ctx* ctx, const Rec32* recs, unsigned long long n, int k, int canonical, unsigned long long* d_kmers, unsigned long long capacity,
                     unsigned long long* need, hipStream_t s)
{
    *need = 0;
    if (n == 0) return hipSuccess;
    unsigned long long* sizes = static_cast<unsigned long long*>(bl_ctx_scratch(ctx, 4, 2 * n * sizeof(unsigned long long)));
    if (!sizes) return hipErrorOutOfMemory;
    unsigned long long* offsets = sizes + n;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(sizes128_kernel, dim3(blocks), dim3(256), 0, s, recs, n, sizes);
    hipError_t e = excl_scan(ctx, 5, sizes, offsets, (size_t)n, s);
    unsigned long long last[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&last[0], offsets + n - 1, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&last[1], sizes + n - 1, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    *need = last[0] + last[1];
    if (!d_kmers || *need > capacity) return hipSuccess;
    hipLaunchKernelGGL(expand128_kernel, dim3(blocks), dim3(256), 0, s, recs, offsets, n, k, canonical, d_kmers);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

// The fallback: expand -> sort (128-bit keys, the 2k bits that can differ) -> run-length encode.  *uniq / *cnts (scratch slots 2 and 3)
// hold *runs distinct k-mers ascending and their multiplicities.  Library plumbing, as in bl_setops.hip.  Scratch slots 2-7.
hipError_t count_by_sort128(bl_ctx* ctx, const Rec32* recs, unsigned long long n, int k, int canonical, __uint128_t** uniq, unsigned int** cnts, unsigned long long* runs,
                            hipStream_t s)
{
    *runs = 0;
    unsigned long long n_kmers = 0;
    hipError_t e = expand128(ctx, recs, n, k, canonical, nullptr, 0, &n_kmers, s);
    if (e != hipSuccess || n_kmers == 0) return e;
    __uint128_t* keys = static_cast<__uint128_t*>(bl_ctx_scratch(ctx, 2, 3 * n_kmers * sizeof(__uint128_t)));
    unsigned int* counts = static_cast<unsigned int*>(bl_ctx_scratch(ctx, 3, n_kmers * sizeof(unsigned int) + 16));
    unsigned long long* d_runs = static_cast<unsigned long long*>(bl_ctx_scratch(ctx, 7, 16));
    if (!keys || !counts || !d_runs) return hipErrorOutOfMemory;
    __uint128_t *sorted = keys + n_kmers, *distinct = keys + 2 * n_kmers;
    e = expand128(ctx, recs, n, k, canonical, reinterpret_cast<unsigned long long*>(keys), n_kmers, &n_kmers, s);
    if (e != hipSuccess) return e;
    e = blh::with_workspace(ctx, 6, [&](void* ws, size_t& bytes) { return rocprim::radix_sort_keys(ws, bytes, keys, sorted, (size_t)n_kmers, 0u, (unsigned)(2 * k), s); });
    if (e != hipSuccess) return e;
    if (n_kmers >= (1ull << 32)) return hipErrorInvalidValue;  // (run_length_encode takes a 32-bit size; 2^32 k-mers are 64 GiB of keys)
    e = blh::with_workspace(ctx, 6, [&](void* ws, size_t& bytes) { return rocprim::run_length_encode(ws, bytes, sorted, (unsigned int)n_kmers, distinct, counts, d_runs, s); });
    if (e == hipSuccess) e = hipMemcpyAsync(runs, d_runs, sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    *uniq = distinct;
    *cnts = counts;
    return e;
}

using blh::hip_rc;

}  // namespace

extern "C" {

int bl_pack_super_kmers128(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_first_pos, const uint8_t* d_sizes, const uint8_t* d_mm_pos, uint64_t n_groups,
                           uint32_t k, uint32_t m, uint64_t* d_records)
{
    if (!ctx || !batch || (n_groups && (!d_first_pos || !d_sizes || !d_records))) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    if (n_groups && !d_mm_pos) return bl_set_error(BL_ERR_INVALID, "d_mm_pos is required: the record's owner finds the minimizer through it");
    if (!shape_ok(k, m)) return bl_set_error(BL_ERR_INVALID, LIMITS);
    if ((uintptr_t)d_records & 31u) return bl_set_error(BL_ERR_INVALID, "d_records must be 32-byte aligned");
    if (n_groups == 0) return BL_OK;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    hipLaunchKernelGGL(pack128_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, s, static_cast<const unsigned char*>(bl_batch_device_bases(batch)),
                       (unsigned long long)bl_batch_n_bases(batch), reinterpret_cast<const unsigned long long*>(d_first_pos), d_sizes, d_mm_pos,
                       (unsigned long long)n_groups, (int)k, reinterpret_cast<Rec32*>(d_records), (unsigned long long)bl_batch_origin(batch));
    BLH_TRY(hipGetLastError());
    return BL_OK;
}

int bl_partition_records128(bl_ctx* ctx, const uint64_t* d_hashes, const uint64_t* d_records, uint64_t n, uint32_t parts, uint64_t* d_out, uint64_t* counts)
{
    if (!ctx || !counts || parts == 0 || parts > MAX_PARTS || (n && (!d_hashes || !d_records || !d_out)))
        return bl_set_error(BL_ERR_INVALID, "bad argument (1 <= parts <= 64)");
    if (((uintptr_t)d_records | (uintptr_t)d_out) & 31u) return bl_set_error(BL_ERR_INVALID, "d_records and d_out must be 32-byte aligned");
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    return blpart::partition(ctx, reinterpret_cast<const Rec32*>(d_records), (unsigned long long)n, parts, HashArrayOwner{reinterpret_cast<const unsigned long long*>(d_hashes)},
                             reinterpret_cast<Rec32*>(d_out), counts, bl_ctx_stream(ctx));
}

int bl_expand_super_kmers128(bl_ctx* ctx, const uint64_t* d_records, uint64_t n_groups, uint32_t k, uint32_t flags, uint64_t* d_kmers, uint64_t capacity,
                             uint64_t* n_kmers)
{
    if (!ctx || !n_kmers || (n_groups && !d_records)) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    if (k < 1 || k > 64) return bl_set_error(BL_ERR_INVALID, "need 1 <= k <= 64");
    if ((uintptr_t)d_records & 31u) return bl_set_error(BL_ERR_INVALID, "d_records must be 32-byte aligned");
    if ((uintptr_t)d_kmers & 15u) return bl_set_error(BL_ERR_INVALID, "d_kmers must be 16-byte aligned");
    *n_kmers = 0;
    if (n_groups == 0) return BL_OK;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    unsigned long long need = 0;
    const hipError_t e = expand128(ctx, reinterpret_cast<const Rec32*>(d_records), n_groups, (int)k, (flags & BL_FLAG_CANONICAL) ? 1 : 0,
                                   reinterpret_cast<unsigned long long*>(d_kmers), capacity, &need, bl_ctx_stream(ctx));
    if (e != hipSuccess) return hip_rc(e);
    *n_kmers = need;
    if (need > capacity || (!d_kmers && need)) return bl_set_error(BL_ERR_CAPACITY, "expanded k-mers exceed the capacity of d_kmers (n_kmers holds the need)");
    return BL_OK;
}

int bl_count_super_kmers128(bl_ctx* ctx, const uint64_t* d_records, uint64_t n_groups, uint32_t k, uint32_t m, uint64_t seed, uint32_t flags, uint64_t* d_kmers,
                            uint32_t* d_counts, uint64_t capacity, uint64_t* n_distinct)
{
    if (!ctx || !n_distinct || (n_groups && !d_records)) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    if (!shape_ok(k, m)) return bl_set_error(BL_ERR_INVALID, LIMITS);
    if (n_groups >= (1ull << 32)) return bl_set_error(BL_ERR_INVALID, "at most 2^32 - 1 records per call");
    if ((uintptr_t)d_records & 31u) return bl_set_error(BL_ERR_INVALID, "d_records must be 32-byte aligned");
    if ((uintptr_t)d_kmers & 15u) return bl_set_error(BL_ERR_INVALID, "d_kmers must be 16-byte aligned");
    const int canonical = (flags & BL_FLAG_CANONICAL) ? 1 : 0;
    *n_distinct = 0;
    if (n_groups == 0) return BL_OK;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    const uint32_t n = (uint32_t)n_groups;
    const Rec32* recs = reinterpret_cast<const Rec32*>(d_records);
    const bool write = d_kmers && d_counts;
    U64x2* out_keys = reinterpret_cast<U64x2*>(d_kmers);
    const char* short_msg = "distinct k-mers exceed the capacity of the output arrays (n_distinct holds the need)";
    __uint128_t* uniq = nullptr;
    unsigned int* cnts = nullptr;
    unsigned long long runs = 0, table_total = 0;
    hipError_t e = hipSuccess;

    if (!bl_ctx_count128_tables(ctx)) {  // every bucket takes the fallback: the whole input is one
        e = count_by_sort128(ctx, recs, n, (int)k, canonical, &uniq, &cnts, &runs, s);
        if (e != hipSuccess) return hip_rc(e);
        *n_distinct = runs;
        if (runs > capacity || (!write && runs)) return bl_set_error(BL_ERR_CAPACITY, short_msg);
        if (runs) {
            hipLaunchKernelGGL(append_counted128_kernel, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, s, uniq, cnts, runs, out_keys, d_counts, 0ull);
            BLH_TRY(hipGetLastError());
            BLH_TRY(hipStreamSynchronize(s));
        }
        return BL_OK;
    }

    // buckets of ~24 records (about 400 k-mers at k = 51, m = 21), one wave each; at most 2^26 of them
    unsigned long long want_buckets = (n_groups + 23) / 24;
    if (want_buckets > (1ull << 26)) want_buckets = 1ull << 26;
    const uint32_t n_buckets = (uint32_t)(want_buckets ? want_buckets : 1);
    int bits = 0;  // of a bucket number (what the radix sort looks at)
    while ((1ull << bits) < n_buckets) ++bits;
    const uint32_t max_overflow = n_buckets;
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t ids_bytes = up16(4ull * n * sizeof(uint32_t)), starts_bytes = up16(((size_t)n_buckets + 2) * sizeof(uint32_t));
    const size_t over_bytes = up16((size_t)max_overflow * sizeof(uint2)), offs_bytes = up16(((size_t)n_buckets + 1) * sizeof(unsigned long long));
    const size_t dist_bytes = up16(((size_t)n_buckets + 1) * sizeof(unsigned long long));
    unsigned char* arena = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 0, ids_bytes + starts_bytes + over_bytes + offs_bytes + dist_bytes + 64));
    if (!arena) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    uint32_t* ids = reinterpret_cast<uint32_t*>(arena);
    uint32_t *ids_sorted = ids + n, *index = ids + 2ull * n, *perm = ids + 3ull * n;
    uint32_t* starts = reinterpret_cast<uint32_t*>(arena + ids_bytes);
    uint2* overflow = reinterpret_cast<uint2*>(arena + ids_bytes + starts_bytes);
    unsigned long long* offsets = reinterpret_cast<unsigned long long*>(arena + ids_bytes + starts_bytes + over_bytes);
    unsigned int* distinct = reinterpret_cast<unsigned int*>(arena + ids_bytes + starts_bytes + over_bytes + offs_bytes);
    unsigned long long* cursor = reinterpret_cast<unsigned long long*>(arena + ids_bytes + starts_bytes + over_bytes + offs_bytes + dist_bytes);
    e = hipMemsetAsync(cursor, 0, 2 * sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bucket_id128_kernel, dim3((n + 255) / 256), dim3(256), 0, s, recs, n, (int)m, canonical, (uint32_t)seed, n_buckets, ids, index);
        e = hipGetLastError();
    }
    if (e == hipSuccess && bits > 0) {
        e = blh::with_workspace(ctx, 1, [&](void* ws, size_t& bytes) { return rocprim::radix_sort_pairs(ws, bytes, ids, ids_sorted, index, perm, (size_t)n, 0, (unsigned)bits, s); });
    } else if (e == hipSuccess) {  // one bucket: the input order
        ids_sorted = ids;
        perm = index;
    }
    const uint32_t want = (n_buckets + CT128_WAVES - 1) / CT128_WAVES;
    const uint32_t grid = want < 256u * 3u ? want : 256u * 3u;  // 3 workgroups of 2 waves per CU by LDS (25.4 KB per wave): all resident, grid-stride
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bucket_starts128_kernel, dim3(n_buckets / 256 + 1), dim3(256), 0, s, ids_sorted, n, n_buckets, starts);
        hipLaunchKernelGGL((count128_kernel<false>), dim3(grid), dim3(64 * CT128_WAVES), 0, s, recs, perm, starts, n_buckets, (int)k, canonical, distinct, offsets,
                           out_keys, d_counts, cursor, overflow, max_overflow);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemsetAsync(distinct + n_buckets, 0, sizeof(unsigned int), s);
    if (e == hipSuccess)  // (the sort is done with slot 1: same stream)
        e = blh::with_workspace(ctx, 1, [&](void* ws, size_t& bytes) { return rocprim::exclusive_scan(ws, bytes, distinct, offsets, 0ull, (size_t)n_buckets + 1, rocprim::plus<unsigned long long>(), s); });
    unsigned long long n_over = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&table_total, offsets + n_buckets, sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&n_over, cursor, sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_rc(e);
    if (n_over > max_overflow) return bl_set_error(BL_ERR_INTERNAL, "more oversized buckets than the fallback list holds");
    if (n_over) {
        std::vector<uint2> ranges(n_over);
        e = hipMemcpy(ranges.data(), overflow, n_over * sizeof(uint2), hipMemcpyDeviceToHost);
        std::vector<unsigned long long> off(n_over + 1, 0);
        for (unsigned long long i = 0; i < n_over; ++i) off[i + 1] = off[i] + (ranges[i].y - ranges[i].x);
        const unsigned long long n_over_recs = off[n_over];
        const size_t gathered_bytes = n_over_recs * sizeof(Rec32);
        unsigned char* a1 = nullptr;
        if (e == hipSuccess) {
            a1 = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 1, gathered_bytes + (n_over + 1) * sizeof(unsigned long long) + 32));
            if (!a1) e = hipErrorOutOfMemory;
        }
        if (e == hipSuccess) {
            Rec32* gathered = reinterpret_cast<Rec32*>(a1);
            unsigned long long* d_off = reinterpret_cast<unsigned long long*>(a1 + gathered_bytes);
            e = hipMemcpy(d_off, off.data(), (n_over + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(gather_ranges128_kernel, dim3((unsigned)n_over), dim3(256), 0, s, recs, perm, overflow, d_off, gathered);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = count_by_sort128(ctx, gathered, n_over_recs, (int)k, canonical, &uniq, &cnts, &runs, s);
        }
        if (e != hipSuccess) return hip_rc(e);
    }
    const unsigned long long total = table_total + runs;
    *n_distinct = total;
    if (total > capacity || (!write && total)) return bl_set_error(BL_ERR_CAPACITY, short_msg);
    if (total == 0) return BL_OK;
    // the second pass: everything fits, so bucket b writes [offsets[b], offsets[b + 1]) and the fallback's k-mers follow
    hipLaunchKernelGGL((count128_kernel<true>), dim3(grid), dim3(64 * CT128_WAVES), 0, s, recs, perm, starts, n_buckets, (int)k, canonical, distinct, offsets, out_keys,
                       d_counts, cursor, overflow, max_overflow);
    e = hipGetLastError();
    if (e == hipSuccess && runs) {
        hipLaunchKernelGGL(append_counted128_kernel, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, s, uniq, cnts, runs, out_keys, d_counts, table_total);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_rc(e);
    return BL_OK;
}

}  // extern "C"
