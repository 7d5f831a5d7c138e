// bl_keylist.hpp — the host bodies of the calls that take a k-mer list right after the scan, once for a key type K (unsigned long long
// in bl_setops.hip, __uint128_t in bl_setops128.hip): sort, sort + unique, run-length count, owner split, run file -> device array and
// the k-way merge of run files.  All of it is plumbing around rocPRIM device primitives; the extern "C" entry points check their
// arguments and make one call.  Scratch: slot 4 the second array, slot 5 rocPRIM's workspace, slot 6 the counter word.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_select.hpp>

#include <vector>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"
#include "bl_partition.hpp"

namespace blkeys {

typedef unsigned long long ull;

// what differs by width and is not a type: the host half of the file calls (bl_spill.cpp) and one text
template <typename K>
struct Width;
template <>
struct Width<ull> {
    static const char* count_limit() { return "bl_count_sorted_u64 takes fewer than 2^32 keys"; }
    static int file_count(const char* path, int with_count, uint64_t* n) { return bl_file_count_u64(path, with_count, n); }
    static int read_host(const char* path, int with_count, void* out, uint64_t capacity) { return bl_read_file_u64_host(path, with_count, static_cast<uint64_t*>(out), capacity, nullptr); }
};
template <>
struct Width<__uint128_t> {
    static const char* count_limit() { return "bl_count_sorted_u128 takes fewer than 2^32 keys"; }
    static int file_count(const char* path, int with_count, uint64_t* n) { return bl_file_count_u128(path, with_count, n); }
    static int read_host(const char* path, int with_count, void* out, uint64_t capacity) { return bl_read_file_u128_host(path, with_count, static_cast<uint64_t*>(out), capacity, nullptr); }
};

inline int scratch_failed() { return bl_set_error(BL_ERR_OOM, "scratch allocation failed"); }
inline int bad_alignment() { return bl_set_error(BL_ERR_INVALID, "arrays of 16-byte keys must be 16-byte aligned"); }

// the word a kernel or a primitive left at d_word, once the stream has drained
inline hipError_t read_counter(const ull* d_word, hipStream_t s, ull* host)
{
    const hipError_t e = hipMemcpyAsync(host, d_word, sizeof(ull), hipMemcpyDeviceToHost, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

// keys[0 .. n) -> sorted[0 .. n) over the bits [0, key_bits)
template <typename K>
hipError_t sort_to(bl_ctx* ctx, K* keys, K* sorted, ull n, uint32_t key_bits, hipStream_t s)
{
    return blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) { return rocprim::radix_sort_keys(ws, bytes, keys, sorted, (size_t)n, 0u, key_bits, s); });
}

// Every body below: n != 0, the pointers checked by the caller.
template <typename K>
int sort_keys(bl_ctx* ctx, K* keys, ull n, uint32_t key_bits)
{
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    // temporaries from the context's scratch (no hipMalloc / hipFree per call: they cost more than the kernels on small inputs and a
    // device-wide synchronisation each on large ones)
    K* tmp = static_cast<K*>(bl_ctx_scratch(ctx, 4, n * sizeof(K)));
    if (!tmp) return scratch_failed();
    BLH_TRY(sort_to(ctx, keys, tmp, n, key_bits, s));
    BLH_TRY(hipMemcpyAsync(keys, tmp, n * sizeof(K), hipMemcpyDeviceToDevice, s));
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}

template <typename K>
int sort_unique(bl_ctx* ctx, K* keys, ull n, uint32_t key_bits, uint64_t* n_unique)
{
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    K* tmp = static_cast<K*>(bl_ctx_scratch(ctx, 4, n * sizeof(K)));
    ull* d_count = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 64));
    if (!tmp || !d_count) return scratch_failed();
    BLH_TRY(sort_to(ctx, keys, tmp, n, key_bits, s));  // keys -> tmp (sorted)
    BLH_TRY(blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) { return rocprim::unique(ws, bytes, tmp, keys, d_count, (size_t)n, rocprim::equal_to<K>(), s); }));  // tmp -> keys
    ull cnt = 0;
    BLH_TRY(read_counter(d_count, s, &cnt));
    *n_unique = cnt;
    return BL_OK;
}

// sorted keys (duplicates kept) -> distinct keys + their multiplicities; *n_unique = the number of distinct keys
template <typename K>
int count_sorted(bl_ctx* ctx, const K* sorted, ull n, K* uniq, uint32_t* d_counts, uint64_t* n_unique)
{
    if (n >= (1ull << 32)) return bl_set_error(BL_ERR_INVALID, Width<K>::count_limit());  // (run_length_encode's size is 32 bits)
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    ull* d_runs = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 64));
    if (!d_runs) return scratch_failed();
    BLH_TRY(blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) { return rocprim::run_length_encode(ws, bytes, sorted, (unsigned int)n, uniq, d_counts, d_runs, s); }));
    ull runs = 0;
    BLH_TRY(read_counter(d_runs, s, &runs));
    *n_unique = runs;
    return BL_OK;
}

// keys[0 .. n) -> out, bucket after bucket by owner(i, parts); counts[parts] on the host (blpart::partition: scratch slots 4 and 5)
template <typename K, typename Owner>
int partition_keys(bl_ctx* ctx, const K* keys, ull n, uint32_t parts, Owner owner, K* out, uint64_t* counts)
{
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    return blpart::partition(ctx, keys, n, parts, owner, out, counts, bl_ctx_stream(ctx));
}

// Read side of the spill format: a run file / stored vector biolib wrote -> device array.  d_out may be NULL
// where the file holds nothing or more than `capacity` elements.
template <typename K>
int read_file(bl_ctx* ctx, const char* path, int with_count, K* d_out, uint64_t capacity, uint64_t* n)
{
    uint64_t cnt = 0;
    int rc = Width<K>::file_count(path, with_count, &cnt);
    if (rc != BL_OK) return rc;
    if (n) *n = cnt;
    if (cnt > capacity) return bl_set_error(BL_ERR_CAPACITY, "device array too small for the file");
    if (cnt == 0) return BL_OK;
    if (!d_out) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    if (sizeof(K) == 16 && blh::misaligned16(d_out)) return bad_alignment();
    std::vector<K> host(cnt);
    rc = Width<K>::read_host(path, with_count, host.data(), cnt);
    if (rc != BL_OK) return rc;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    BLH_TRY(hipMemcpyAsync(d_out, host.data(), cnt * sizeof(K), hipMemcpyHostToDevice, s));
    BLH_TRY(hipStreamSynchronize(s));  // `host` goes away
    return BL_OK;
}

// The k-way merge the reference's external_memory_vector iterator performs (external_memory_vector.hpp:265-347) as a tree of pairwise
// device merges (rocprim::merge) over the runs loaded back to back.  Slot 4: the ping-pong array, slot 5: the merge's workspace.
template <typename K>
int merge_runs(bl_ctx* ctx, const char* const* paths, uint32_t n_paths, K* d_out, uint64_t capacity, uint64_t* n_total)
{
    std::vector<uint64_t> len(n_paths), off(n_paths + 1, 0);
    for (uint32_t i = 0; i < n_paths; ++i) {
        const int rc = Width<K>::file_count(paths[i], 0, &len[i]);
        if (rc != BL_OK) return rc;
        off[i + 1] = off[i] + len[i];
    }
    const uint64_t total = off[n_paths];
    *n_total = total;
    if (total > capacity) return bl_set_error(BL_ERR_CAPACITY, "device array too small for the merged runs");
    if (total == 0) return BL_OK;
    if (!d_out) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    if (sizeof(K) == 16 && blh::misaligned16(d_out)) return bad_alignment();
    for (uint32_t i = 0; i < n_paths; ++i) {
        const int rc = read_file<K>(ctx, paths[i], 0, d_out + off[i], len[i], nullptr);
        if (rc != BL_OK) return rc;
    }
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    // runs = [cur[i], cur[i+1]); merge neighbours pairwise, ping-ponging between d_out and the scratch array
    K* a = d_out;
    K* b = nullptr;
    hipError_t e = hipSuccess;
    std::vector<uint64_t> cur(off);
    bool in_a = true;
    while (cur.size() > 2 && e == hipSuccess) {
        if (!b) {
            b = static_cast<K*>(bl_ctx_scratch(ctx, 4, total * sizeof(K)));
            if (!b) return scratch_failed();
        }
        K* src = in_a ? a : b;
        K* dst = in_a ? b : a;
        std::vector<uint64_t> next(1, 0);
        for (size_t i = 0; i + 1 < cur.size() && e == hipSuccess; i += 2) {
            const uint64_t lo = cur[i], mid = cur[i + 1], hi = i + 2 < cur.size() ? cur[i + 2] : cur[i + 1];
            if (hi == mid) {  // odd run out: copied through
                if (mid > lo) e = hipMemcpyAsync(dst + lo, src + lo, (mid - lo) * sizeof(K), hipMemcpyDeviceToDevice, s);
            } else {  // (where slot 5 has to grow, the merges in flight are done with the old block first: blh::with_workspace)
                e = blh::with_workspace(ctx, 5, [&](void* ws, size_t& bytes) { return rocprim::merge(ws, bytes, src + lo, src + mid, dst + lo, mid - lo, hi - mid, rocprim::less<K>(), s); });
            }
            next.push_back(hi);
        }
        cur.swap(next);
        in_a = !in_a;
    }
    if (e == hipSuccess && !in_a) e = hipMemcpyAsync(a, b, total * sizeof(K), hipMemcpyDeviceToDevice, s);
    const hipError_t se = hipStreamSynchronize(s);
    return e != hipSuccess ? blh::hip_rc(e) : se != hipSuccess ? blh::hip_rc(se) : BL_OK;
}

}  // namespace blkeys
