// bl_select.hip — bl_batch_select: a new device-resident batch from per-read spans of another one (whole-read filtering, trimming), and
// bl_read_spans: the spans from whole-read bl_read_counts records.  The per-thread bodies are in bl_select_core.hpp.  Kernels:
//   span_lengths_kernel    per source read: the clamped span's length, absolute start and keep flag
//   place_kernel           per kept read, after rocPRIM's exclusive sums: the result's offsets, source starts and source index
//   gather_kernel          the hot path: a lane produces CHUNKS_PER_LANE 16-byte output chunks, each with one 16-byte store; the 64 lanes
//                          of a wave store 1 KiB contiguously per step and 4 KiB per wave.  The wave finds its first sequence with a
//                          64-ary search and keeps the next 64 offsets in registers: ballots and shuffles, no LDS, no barrier, no atomic.
//   uniform_kernel         is the result a fixed-length batch (bl_parse.hip's rule)
//   read_spans_kernel      bl_read_spans, elementwise
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"
#include "bl_select_core.hpp"

static_assert(sizeof(blsel::Record) == sizeof(bl_read_counts), "Record is bl_read_counts");
static_assert(sizeof(blsel::SpanRule) == sizeof(bl_span_rule), "SpanRule is bl_span_rule");
static_assert((uint32_t)BL_SELECT_KEEP_EMPTY == blsel::KEEP_EMPTY && BL_TRIM_LONGER == blsel::TRIM_LONGER, "the header's constants");

namespace blsel {

__global__ __launch_bounds__(TPB) void span_lengths_kernel(const SelectParams p) { span_lengths(p, (uint64_t)blockIdx.x * TPB + threadIdx.x); }

__global__ __launch_bounds__(TPB) void place_kernel(const SelectParams p) { place_sequence(p, (uint64_t)blockIdx.x * TPB + threadIdx.x); }

__global__ __launch_bounds__(TPB) void uniform_kernel(const uint64_t* out_offsets, uint64_t n_out, uint64_t len, unsigned int* flag)
{
    if (breaks_uniform(out_offsets, n_out, len, (uint64_t)blockIdx.x * TPB + threadIdx.x)) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(TPB) void read_spans_kernel(const SpanParams p) { read_span(p, (uint64_t)blockIdx.x * TPB + threadIdx.x); }

__global__ __launch_bounds__(TPB) void gather_kernel(const SelectParams p)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    const uint64_t x_first = wave_first_byte(wave);
    if (x_first >= p.total) return;  // (wave-uniform, as everything up to the chunks)
    // the wave's first sequence: 64-ary search with all lanes
    uint64_t lo = 0, e = p.n_out;
    while (e - lo > 1) kary_narrow(lo, e, (uint64_t)__popcll(__ballot(kary_probe(p.out_offsets, lo, e, lane, x_first))));
    // the next 64 offsets and source starts in registers; do they reach the wave's last byte?
    const uint64_t x_last = wave_last_byte(p, wave);
    const uint64_t o = lane_offset(p, lo, lane), src = lane_source(p, lo, lane), o_lo = p.out_offsets[lo];
    const int inside = __popcll(__ballot(o <= x_last));
    const bool in_registers = inside < 64;
    const uint64_t hi = in_registers ? lo + (uint64_t)inside : seq_of(p.out_offsets, x_last, lo + 64, p.n_out - 1);

    // the sequence that holds output byte x (wave-uniform control flow: every lane takes part in the shuffles)
    auto locate = [&](uint64_t x) {
        SeqAt s;
        if (in_registers) {
            uint32_t cnt = 0;
#pragma unroll
            for (uint32_t step = 32; step >= 1; step >>= 1) count_step(cnt, step, __shfl(o, (int)(cnt + step - 1), 64), x);
            const uint64_t before = __shfl(o, (int)cnt - 1, 64);  // (cnt = 0: any lane's, not used)
            s.j = lo + cnt;
            s.begin = cnt ? before : o_lo;
            s.end = __shfl(o, (int)cnt, 64);
            s.src = __shfl(src, (int)cnt, 64);
        } else {
            s = seq_from_memory(p, x, lo, hi);
        }
        return s;
    };

    // Where every chunk lies, and the loads of those that are one window: all issued before the first is used.  Only the loaded dwords,
    // the shift and a flag per chunk stay in registers; the few chunks that go piece by piece look their sequence up again below.
    uint32_t v[CHUNKS_PER_LANE][5];
    uint32_t one_window = 0, shifts = 0;
#pragma unroll
    for (int u = 0; u < CHUNKS_PER_LANE; ++u) {
        const uint64_t x0 = chunk_first_byte(wave, u, lane);
        const SeqAt s = locate(x0 < p.total ? x0 : p.total - 1);
        if (x0 < p.total && chunk_is_one_window(p, s, x0)) {
            const uint64_t vsrc = (uint64_t)chunk_vsrc(s, x0);
            window_load(p.bases, vsrc, v[u]);
            one_window |= 1u << u;
            shifts |= (uint32_t)(vsrc & 3u) << (2 * u);
        }
    }
#pragma unroll
    for (int u = 0; u < CHUNKS_PER_LANE; ++u) {
        const uint64_t x0 = chunk_first_byte(wave, u, lane);
        const bool live = x0 < p.total, whole = (one_window >> u) & 1u;
        uint32_t w[4];
        if (__ballot(live && !whole)) {  // (wave-uniform)
            const SeqAt s = locate(live ? x0 : p.total - 1);
            if (live && !whole) gather_pieces(p, x0, s, w);
        }
        if (whole) window_shift(v[u], (shifts >> (2 * u)) & 3u, w);
        if (live) *reinterpret_cast<uint4*>(p.out + x0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

namespace {

using blh::blocks_for;
using blh::exclusive_sum;
using blh::invalid;

// what both calls check of (ctx, batch, d_offsets); fills the source's description
int describe_source(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, uint64_t& n_bases, uint64_t& n_seqs, uint64_t& read_len)
{
    blh::BatchView v;
    BLH_OK(blh::batch_view(ctx, batch, v));
    BLH_OK(blh::offsets_needed(d_offsets, v.n_seqs, v.read_len));
    n_bases = v.n_bases;
    n_seqs = v.n_seqs;
    read_len = d_offsets ? 0 : (v.read_len ? v.read_len : (n_bases ? n_bases : 1));
    return BL_OK;
}

}  // namespace

}  // namespace blsel

extern "C" int bl_batch_select(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const uint64_t* d_spans, uint32_t flags, bl_batch** out,
                               uint64_t* d_out_offsets, uint64_t* d_source_index, uint64_t* n_seqs_out, uint64_t* n_bases_out)
{
    using namespace blsel;
    if (!ctx || !batch || !out) return invalid("ctx, batch or out is NULL");
    *out = nullptr;
    if (!d_spans) return invalid("d_spans is NULL");
    if (blh::misaligned16(d_spans)) return invalid("d_spans must be 16-byte aligned");
    if (flags & ~(uint32_t)BL_SELECT_KEEP_EMPTY) return invalid("unknown flag bits");
    SelectParams p{};
    BLH_OK(describe_source(ctx, batch, d_offsets, p.n_bases, p.n_seqs, p.read_len));
    p.bases = static_cast<const uint8_t*>(bl_batch_device_bases(batch));
    p.offsets = d_offsets;
    p.spans = d_spans;
    p.flags = flags;
    p.user_offsets = d_out_offsets;
    p.source_index = d_source_index;

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the context's scans in flight
    const uint64_t n1 = p.n_seqs + 1;
    // slot 4: len, keep, start, their two sums and the result's source starts; slot 6: the fixed-length flag
    uint64_t* arena = static_cast<uint64_t*>(bl_ctx_scratch(ctx, 4, (size_t)(6 * n1) * sizeof(uint64_t)));
    unsigned int* d_flag = static_cast<unsigned int*>(bl_ctx_scratch(ctx, 6, 128));
    if (!arena || !d_flag) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    p.len = arena;
    p.keep = arena + n1;
    p.start = arena + 2 * n1;
    uint64_t* len_sum = arena + 3 * n1;
    uint64_t* keep_sum = arena + 4 * n1;
    p.len_sum = len_sum;
    p.keep_sum = keep_sum;
    p.src_start = arena + 5 * n1;

    hipLaunchKernelGGL(span_lengths_kernel, dim3(blocks_for(n1, TPB)), dim3(TPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    BLH_OK(exclusive_sum(ctx, p.len, len_sum, (size_t)n1, s));
    BLH_OK(exclusive_sum(ctx, p.keep, keep_sum, (size_t)n1, s));  // (the first sum is done with slot 5: same stream)
    unsigned long long total = 0, n_out = 0;
    BLH_TRY(hipMemcpyAsync(&total, len_sum + p.n_seqs, sizeof(total), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipMemcpyAsync(&n_out, keep_sum + p.n_seqs, sizeof(n_out), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    p.total = total;
    p.n_out = n_out;

    blh::Pooled<uint8_t> d_bases(ctx, (size_t)total + 64);
    blh::Pooled<uint64_t> d_offs(ctx, (size_t)(n_out + 1) * sizeof(uint64_t));
    if (!d_bases || !d_offs) return bl_set_error(BL_ERR_OOM, "device allocation failed (batch)");
    p.out = d_bases.get();
    p.out_offsets = d_offs.get();
    BLH_TRY(hipMemsetAsync(d_bases.get() + (total & ~15ull), 0, 64 + (total & 15ull), s));  // (the last chunk's store comes after it and repeats its zeros)
    hipLaunchKernelGGL(place_kernel, dim3(blocks_for(n1, TPB)), dim3(TPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    if (total) {
        const uint64_t waves = (total + WAVE_BYTES - 1) / WAVE_BYTES;
        hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(waves * 64, TPB)), dim3(TPB), 0, s, p);
        BLH_TRY(hipGetLastError());
    }
    // sequences of one length make a fixed-length batch (the parser's rule): the read-tiled scan kernels, no start-bit vector
    uint64_t fixed_len = n_out > 1 && total != 0 && total % n_out == 0 ? total / n_out : 0;
    unsigned int ragged = 0;
    if (fixed_len) {
        BLH_TRY(hipMemsetAsync(d_flag, 0, sizeof(unsigned int), s));
        hipLaunchKernelGGL(uniform_kernel, dim3(blocks_for(n_out + 1, TPB)), dim3(TPB), 0, s, d_offs.get(), (uint64_t)n_out, fixed_len, d_flag);
        BLH_TRY(hipGetLastError());
        BLH_TRY(hipMemcpyAsync(&ragged, d_flag, sizeof(ragged), hipMemcpyDeviceToHost, s));
    }
    BLH_TRY(hipStreamSynchronize(s));
    if (ragged) fixed_len = 0;
    BLH_OK(bl_batch_adopt_device(ctx, d_bases.release(), total, d_offs.release(), n_out, fixed_len, out));  // takes ownership of both
    if (n_seqs_out) *n_seqs_out = n_out;
    if (n_bases_out) *n_bases_out = total;
    return BL_OK;
}

extern "C" int bl_read_spans(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const bl_read_counts* d_records, const uint32_t* d_stat,
                             const bl_span_rule* rule, uint64_t* d_spans)
{
    using namespace blsel;
    if (!ctx || !batch) return invalid("ctx or batch is NULL");
    if (!d_records || !rule || !d_spans) return invalid("d_records, rule or d_spans is NULL");
    if (blh::misaligned16(d_records) || blh::misaligned16(d_spans)) return invalid("d_records and d_spans must be 16-byte aligned");
    SpanParams p{};
    static_assert(sizeof(p.rule) == sizeof(*rule), "one layout");
    std::memcpy(&p.rule, rule, sizeof(p.rule));
    if (!rule_valid(p.rule)) return invalid("bl_span_rule: trim is 0 .. 3, k 1 .. 64, every fraction has den >= 1 and num <= den, reserved is 0");
    BLH_OK(describe_source(ctx, batch, d_offsets, p.n_bases, p.n_seqs, p.read_len));
    p.offsets = d_offsets;
    p.records = reinterpret_cast<const Record*>(d_records);
    p.stat = d_stat;
    p.spans = d_spans;
    if (p.n_seqs == 0) return BL_OK;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the scan that writes the records
    hipLaunchKernelGGL(read_spans_kernel, dim3(blocks_for(p.n_seqs, TPB)), dim3(TPB), 0, s, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? BL_OK : bl_set_error(BL_ERR_HIP, (std::string("read_spans_kernel: ") + hipGetErrorString(e)).c_str());
}
