// bl_table_ops.hip — count-table algebra: bl_table_combine (union, intersection, key subtraction and count subtraction of two tables
// with a count rule and count bounds, and the comparison statistics) and bl_table_filter.  One linear merge of two sorted (key, count)
// sequences with ordered output, in the two-pass form of DESIGN.md §5.5 —
//   partition   one thread per tile boundary finds the tile's merge-path split in global memory (table_partition_kernel)
//   count       one workgroup per tile stages its A and B ranges (one A key more in front, one B element more behind) in LDS; every
//               thread walks its merged elements, decides which are in the result and adds to the statistics; the workgroup writes its
//               tile total and adds the statistics with a handful of integer atomics (table_count_kernel)
//   scan        exclusive scan of the tile totals (rocPRIM, library plumbing as in the build)
//   write       the same walk, a workgroup prefix of the per-thread emit counts, keys and counts written at tile_base + rank
//               (table_write_kernel).  No atomic places anything: the result is bit-reproducible.
// The per-thread bodies and the rule that decides correctness are in bl_table_ops_core.hpp.  The result becomes an ordinary table through
// bllk::finish_table (bl_lookup.hip): the prefix index is the build's.
#include <hip/hip_runtime.h>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"
#include "bl_lookup_launch.hpp"
#include "bl_table_ops_core.hpp"

namespace {

using namespace bltop;
typedef unsigned long long ull;

static_assert(BL_TABLE_UNION == OP_UNION && BL_TABLE_INTERSECT == OP_INTERSECT && BL_TABLE_SUBTRACT == OP_SUBTRACT && BL_TABLE_COUNT_SUBTRACT == OP_COUNT_SUBTRACT,
              "the ops of the header are the core's");
static_assert(BL_COUNT_SUM == MODE_SUM && BL_COUNT_MIN == MODE_MIN && BL_COUNT_MAX == MODE_MAX && BL_COUNT_LEFT == MODE_LEFT && BL_COUNT_RIGHT == MODE_RIGHT,
              "the count modes of the header are the core's");
static_assert(sizeof(bl_table_stats) == 8 * sizeof(ull), "the device words are the caller's");
static_assert(sizeof(Key1) == 8 && sizeof(Key2) == 16, "a key is one or two words");

constexpr int N_STATS = 7;  // n_a_only, n_b_only, n_both, n_out, sum_min, sum_max, sum_out: the order of bl_table_stats
constexpr int WRITTEN = 8;  // word of the counter block that takes the write pass's total

struct Tables {
    const void* a;
    const uint32_t* ca;
    ull na;
    const void* b;
    const uint32_t* cb;
    ull nb;
};

template <typename K>
struct TileShared {
    K keys[lds_keys<K>()];            // [front A key] A range, B range [B element behind]
    uint32_t counts[lds_counts<K>()];  // A range, B range [B element behind]
    ull red[TPB / 64][N_STATS];
    uint32_t wave[TPB / 64];
};

// splits[t] = A elements in front of diagonal min(t * TILE, na + nb), t = 0 .. n_tiles
template <typename K>
__global__ __launch_bounds__(TPB) void table_partition_kernel(const Tables in, ull n_tiles, ull* __restrict__ splits)
{
    const ull t = (ull)blockIdx.x * TPB + threadIdx.x;
    if (t > n_tiles) return;
    const ull total = in.na + in.nb;
    const ull d = t * (ull)Geo<K>::TILE < total ? t * (ull)Geo<K>::TILE : total;
    splits[t] = diag_split<K, ull>(static_cast<const K*>(in.a), in.na, static_cast<const K*>(in.b), in.nb, d);
}

template <typename K>
__device__ __forceinline__ void stage_tile(TileShared<K>& sh, const TileRange& r, const Tables& in)
{
    tile_stage_thread<K>(r, static_cast<const K*>(in.a), in.ca, static_cast<const K*>(in.b), in.cb, sh.keys, sh.counts, threadIdx.x);
}

template <typename K>
__global__ __launch_bounds__(TPB) void table_count_kernel(const Tables in, const Rule rule, const ull* __restrict__ splits, ull* __restrict__ tile_totals, ull* stats)
{
    __shared__ TileShared<K> sh;
    const TileRange r = tile_range<K>(splits, blockIdx.x, in.na, in.nb);
    stage_tile(sh, r, in);
    __syncthreads();
    ThreadStats st{0, 0, 0, 0, 0, 0, 0};
    Walk<K> w;
    tile_thread_walk<K>(rule, sh.keys + r.laf, sh.counts, r.la, r.laf, sh.keys + r.laf + r.la, sh.counts + r.la, r.lb, r.lbx, threadIdx.x, st, w);
    ull v[N_STATS] = {st.n_a_only, st.n_b_only, st.n_both, st.n_out, st.sum_min, st.sum_max, st.sum_out};
#pragma unroll
    for (int k = 0; k < N_STATS; ++k)
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N_STATS; ++k) sh.red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < N_STATS) {  // integer sums: the order does not matter
        ull sum = 0;
        for (int wv = 0; wv < TPB / 64; ++wv) sum += sh.red[wv][threadIdx.x];
        if (sum) atomicAdd(&stats[threadIdx.x], sum);
        if (threadIdx.x == 3) tile_totals[blockIdx.x] = sum;
    }
}

template <typename K>
__global__ __launch_bounds__(TPB) void table_write_kernel(const Tables in, const Rule rule, const ull* __restrict__ splits, const ull* __restrict__ tile_bases, ull n_out,
                                                          K* __restrict__ out_keys, uint32_t* __restrict__ out_counts, ull* counters)
{
    __shared__ TileShared<K> sh;
    const TileRange r = tile_range<K>(splits, blockIdx.x, in.na, in.nb);
    stage_tile(sh, r, in);
    __syncthreads();
    ThreadStats st{0, 0, 0, 0, 0, 0, 0};
    Walk<K> w;
    const K* sa = sh.keys + r.laf;
    const K* sb = sh.keys + r.laf + r.la;
    tile_thread_walk<K>(rule, sa, sh.counts, r.la, r.laf, sb, sh.counts + r.la, r.lb, r.lbx, threadIdx.x, st, w);
    // the thread's rank in the tile: inclusive scan in the wave, then the totals of the waves in front
    const uint32_t mine = (uint32_t)__builtin_popcount(w.emit);
    const uint32_t lane = threadIdx.x & 63;
    uint32_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) sh.wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t rank = incl - mine;
    for (uint32_t wv = 0; wv < (threadIdx.x >> 6); ++wv) rank += sh.wave[wv];
    const ull first = tile_bases[blockIdx.x] + rank;
    // (the count pass made the same walk over the same data: first + mine <= n_out.  Checked all the same; the host sees the shortfall)
    uint32_t wrote = 0;
    if (first + mine <= n_out) wrote = tile_thread_write<K>(w, sa, sb, out_keys + first, out_counts + first);
    for (int d = 32; d >= 1; d >>= 1) wrote += __shfl_xor(wrote, d, 64);
    if (lane == 0 && wrote) atomicAdd(&counters[WRITTEN], (ull)wrote);
}

using blh::hip_rc;

template <typename K>
int combine(bl_ctx* ctx, const bl_table* ta, const bl_table* tb, const Rule& rule, bl_table** out, bl_table_stats* stats)
{
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    Tables in{};
    in.a = ta->view.keys;
    in.ca = ta->view.counts;
    in.na = ta->view.n;
    if (tb) {
        in.b = tb->view.keys;
        in.cb = tb->view.counts;
        in.nb = tb->view.n;
    }
    const ull n_tiles = (in.na + in.nb + Geo<K>::TILE - 1) / Geo<K>::TILE;  // < 2^23

    // slot 6: the statistics and the write pass's total; slot 4: splits | tile totals | tile bases
    ull host[WRITTEN + 1] = {};
    ull* d_counters = nullptr;
    ull* splits = nullptr;
    ull* totals = nullptr;
    ull* bases = nullptr;
    if (n_tiles) {
        d_counters = static_cast<ull*>(bl_ctx_scratch(ctx, 6, 128));
        splits = static_cast<ull*>(bl_ctx_scratch(ctx, 4, (3 * n_tiles + 1) * sizeof(ull)));
        if (!d_counters || !splits) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        totals = splits + n_tiles + 1;
        bases = totals + n_tiles;
        BLH_TRY(hipMemsetAsync(d_counters, 0, (WRITTEN + 1) * sizeof(ull), s));
        hipLaunchKernelGGL(table_partition_kernel<K>, dim3((unsigned)((n_tiles + 1 + TPB - 1) / TPB)), dim3(TPB), 0, s, in, n_tiles, splits);
        hipLaunchKernelGGL(table_count_kernel<K>, dim3((unsigned)n_tiles), dim3(TPB), 0, s, in, rule, splits, totals, d_counters);
        BLH_TRY(hipGetLastError());
        BLH_TRY(hipMemcpyAsync(host, d_counters, N_STATS * sizeof(ull), hipMemcpyDeviceToHost, s));
        BLH_TRY(hipStreamSynchronize(s));
    }
    const ull n_out = host[3];
    if (stats) {
        stats->n_a_only = host[0];
        stats->n_b_only = host[1];
        stats->n_both = host[2];
        stats->n_out = host[3];
        stats->sum_min = host[4];
        stats->sum_max = host[5];
        stats->sum_out = host[6];
        stats->reserved = 0;
    }
    if (!out) return BL_OK;
    if (!fits_table(n_out, MAX_OUT)) return bl_set_error(BL_ERR_CAPACITY, "the result has 2^32 entries or more: a count table takes fewer");

    bl_table* t = nullptr;
    int rc = bllk::new_table(ctx, ta->view.key_words, ta->view.key_bits, n_out, &t);
    if (rc != BL_OK) return rc;
    if (n_out) {
        static_assert(sizeof(ull) == sizeof(uint64_t), "the tile totals are 8-byte words");
        rc = blh::exclusive_sum(ctx, reinterpret_cast<const uint64_t*>(totals), reinterpret_cast<uint64_t*>(bases), (size_t)n_tiles, s);
        if (rc != BL_OK) { bllk::free_table(t); return rc; }
        hipLaunchKernelGGL(table_write_kernel<K>, dim3((unsigned)n_tiles), dim3(TPB), 0, s, in, rule, splits, bases, n_out,
                           reinterpret_cast<K*>(const_cast<uint64_t*>(t->view.keys)), const_cast<uint32_t*>(t->view.counts), d_counters);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&host[WRITTEN], d_counters + WRITTEN, sizeof(ull), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { bllk::free_table(t); return hip_rc(e); }
        if (host[WRITTEN] != n_out) { bllk::free_table(t); return bl_set_error(BL_ERR_INTERNAL, "the write pass emitted another number of keys than the count pass"); }
    }
    const hipError_t e = bllk::finish_table(ctx, t, s);
    if (e != hipSuccess) { bllk::free_table(t); return hip_rc(e); }
    *out = t;
    return BL_OK;
}

}  // namespace

extern "C" {

int bl_table_combine(bl_ctx* ctx, const bl_table* a, const bl_table* b, uint32_t op, uint32_t count_mode, uint32_t count_lo, uint32_t count_hi, bl_table** out,
                     bl_table_stats* stats)
{
    if (out) *out = nullptr;
    if (!ctx || !a) return blh::invalid("ctx or table a is NULL");
    BLH_OK(blh::table_owner(a->ctx, ctx));
    if (b) BLH_OK(blh::table_owner(b->ctx, ctx));
    if (b && (b->view.key_words != a->view.key_words || b->view.key_bits != a->view.key_bits))
        return blh::invalid("the two tables differ in key_words or key_bits");
    if (op >= N_OPS) return blh::invalid("unknown op (BL_TABLE_UNION .. BL_TABLE_COUNT_SUBTRACT)");
    if (count_mode >= N_MODES) return blh::invalid("unknown count mode (BL_COUNT_SUM .. BL_COUNT_RIGHT)");
    if (!rule_ok(op, count_mode)) return blh::invalid("BL_TABLE_SUBTRACT and BL_TABLE_COUNT_SUBTRACT take BL_COUNT_LEFT only");
    if (count_lo > count_hi) return blh::invalid("count_lo exceeds count_hi");
    const Rule rule{op, count_mode, count_lo, count_hi};
    return a->view.key_words == 2 ? combine<Key2>(ctx, a, b, rule, out, stats) : combine<Key1>(ctx, a, b, rule, out, stats);
}

int bl_table_filter(bl_ctx* ctx, const bl_table* a, uint32_t count_lo, uint32_t count_hi, bl_table** out)
{
    if (!out) return blh::invalid("out is NULL");
    return bl_table_combine(ctx, a, nullptr, BL_TABLE_UNION, BL_COUNT_LEFT, count_lo, count_hi, out, nullptr);
}

}  // extern "C"
