// bl_format.hip — the chain's exit: bl_text_index_build (a parsed text keeps its names and qualities on the device), bl_batch_format (a
// batch written as FASTA / FASTQ text on the device) and bl_text_write (device text to a file through two pinned buffers).  The
// per-thread bodies are in bl_format_core.hpp.  Kernels:
//   index_kernel           per line of the parsed text: a header line writes its record's row (name place, quality place, offset)
//   record_length_kernel   per sequence: the byte count of its record
//   format_kernel          the hot path, output-centric like bl_select.hip's gather_kernel: a lane produces CHUNKS_PER_LANE 16-byte chunks
//                          with one 16-byte store each, a wave 4 KiB contiguously.  The wave finds its first record with the 64-ary search
//                          and keeps the next 64 record offsets in registers: ballots and shuffles, no LDS, no barrier, no atomic.
// No grid cap: the grids are sized by the work (2^31 - 1 workgroups of 16 KiB are 32 TiB of text).
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/biolib_amd.h"
#include "bl_format_core.hpp"
#include "bl_host.hpp"
#include "bl_parse_core.hpp"

int bl_parse_device_text_lines(bl_ctx* ctx, const uint8_t* d_text_in, uint64_t n_bytes, char first_byte, const char* ends, uint64_t ends_n, bl_batch** out,
                               uint64_t* n_seqs, uint64_t* n_bases, bl_parse::LineIndex* lines);  // bl_parse.hip

static_assert(sizeof(blfmt::TextRecord) == 16 && sizeof(blfmt::Desc) == 64, "the index's record is 16 bytes, a description 64");
static_assert(BL_FORMAT_FASTA == blfmt::FORMAT_FASTA && BL_FORMAT_FASTQ == blfmt::FORMAT_FASTQ && (uint32_t)BL_FORMAT_SKIP_EMPTY == blfmt::SKIP_EMPTY &&
                  (uint32_t)BL_FORMAT_TAG_LENGTH == blfmt::TAG_LENGTH,
              "the header's constants");

struct bl_text_index {
    bl_ctx* ctx = nullptr;
    uint8_t* d_text = nullptr;  // pool: n_bytes + 64
    uint64_t n_bytes = 0;
    blfmt::TextRecord* d_records = nullptr;  // pool: max(n_records, 1)
    uint64_t* d_offsets = nullptr;           // pool: n_records + 1
    uint64_t n_records = 0;
    uint64_t n_bases = 0;  // of the batch it was built with: d_offsets[n_records]
    int fastq = 0;
};

namespace blfmt {

__global__ __launch_bounds__(TPB) void index_kernel(const uint8_t* text, const bl_parse::LineIndex li, TextRecord* records, uint64_t* offsets, unsigned int* err)
{
    const uint32_t e = index_line(text, li.line_end, li.hdr, li.rec_incl, li.dst, li.n_lines, li.fastq, li.n_records, li.total, records, offsets,
                                  (uint64_t)blockIdx.x * TPB + threadIdx.x);
    if (e) atomicOr(err, e);
}

__global__ __launch_bounds__(TPB) void record_length_kernel(const FormatParams p) { record_length(p, (uint64_t)blockIdx.x * TPB + threadIdx.x); }

__global__ __launch_bounds__(TPB) void format_kernel(const FormatParams p)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    const uint64_t x_first = blsel::wave_first_byte(wave);
    if (x_first >= p.total) return;  // (wave-uniform, as everything up to the chunks)
    // the wave's first record: 64-ary search with all lanes
    uint64_t lo = 0, e = p.n_seqs;
    while (e - lo > 1) blsel::kary_narrow(lo, e, (uint64_t)__popcll(__ballot(blsel::kary_probe(p.rec_off, lo, e, lane, x_first))));
    // the next 64 offsets in registers; do they reach the wave's last byte?
    const uint64_t x_last = wave_last_byte(p, wave);
    const uint64_t o = lane_offset(p, lo, lane), o_lo = p.rec_off[lo];
    const int inside = __popcll(__ballot(o <= x_last));
    const bool in_registers = inside < 64;
    const uint64_t hi = in_registers ? lo + (uint64_t)inside : blsel::seq_of(p.rec_off, x_last, lo + 64, p.n_seqs - 1);

    // the record that holds output byte x (wave-uniform control flow: every lane takes part in the shuffles)
    auto locate = [&](uint64_t x) {
        RecAt s;
        if (in_registers) {
            uint32_t cnt = 0;
#pragma unroll
            for (uint32_t step = 32; step >= 1; step >>= 1) blsel::count_step(cnt, step, __shfl(o, (int)(cnt + step - 1), 64), x);
            const uint64_t before = __shfl(o, (int)cnt - 1, 64);  // (cnt = 0: any lane's, not used)
            s.j = lo + cnt;
            s.begin = cnt ? before : o_lo;
            s.end = __shfl(o, (int)cnt, 64);
        } else {
            s = rec_from_memory(p, x, lo, hi);
        }
        return s;
    };

    // Where every chunk lies, and the loads of those that are one window: all issued before the first is used.
    uint32_t v[CHUNKS_PER_LANE][5];
    uint32_t one_window = 0, shifts = 0;
#pragma unroll
    for (int u = 0; u < CHUNKS_PER_LANE; ++u) {
        const uint64_t x0 = blsel::chunk_first_byte(wave, u, lane);
        const bool live = x0 < p.total;
        const RecAt s = locate(live ? x0 : p.total - 1);
        if (live) {
            const Rec d = load_rec(p, s.j);
            const uint8_t* src;
            uint64_t vsrc;
            if (x0 + CHUNK <= s.end && chunk_window(p, d, x0 - s.begin, src, vsrc)) {
                blsel::window_load(src, vsrc, v[u]);
                one_window |= 1u << u;
                shifts |= (uint32_t)(vsrc & 3u) << (2 * u);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CHUNKS_PER_LANE; ++u) {
        const uint64_t x0 = blsel::chunk_first_byte(wave, u, lane);
        const bool live = x0 < p.total, whole = (one_window >> u) & 1u;
        uint32_t w[4];
        if (__ballot(live && !whole)) {  // (wave-uniform)
            const RecAt s = locate(live ? x0 : p.total - 1);
            if (live && !whole) format_pieces(p, x0, s, w);
        }
        if (whole) blsel::window_shift(v[u], (shifts >> (2 * u)) & 3u, w);
        if (live) store_chunk(p.out, p.total, x0, w);
    }
}

namespace {

using blh::blocks_for;
using blh::exclusive_sum;
using blh::hip_rc;
using blh::invalid;
using blh::pack_prefix;
using blh::terminated_length;

void free_index(bl_text_index* ix)
{
    if (!ix) return;
    bl_ctx_pool_free(ix->ctx, ix->d_text);
    bl_ctx_pool_free(ix->ctx, ix->d_records);
    bl_ctx_pool_free(ix->ctx, ix->d_offsets);
    delete ix;
}

// ix->d_text holds the text already (copy enqueued on the context's stream): parse it and build the rows
int index_device_text(bl_ctx* ctx, bl_text_index* ix, char first_byte, const char* ends, uint64_t ends_n, bl_batch** out_batch, uint64_t* n_seqs, uint64_t* n_bases)
{
    bl_parse::LineIndex li{};
    int rc = bl_parse_device_text_lines(ctx, ix->d_text, ix->n_bytes, first_byte, ends, ends_n, out_batch, n_seqs, n_bases, &li);
    if (rc != BL_OK) return rc;
    auto fail = [&](int code) {
        bl_batch_destroy(*out_batch);
        *out_batch = nullptr;
        if (n_seqs) *n_seqs = 0;
        if (n_bases) *n_bases = 0;
        return code;
    };
    ix->n_records = li.n_records;
    ix->n_bases = li.total;
    ix->fastq = first_byte == '@';
    ix->d_records = static_cast<TextRecord*>(bl_ctx_pool_alloc(ctx, (size_t)(li.n_records ? li.n_records : 1) * sizeof(TextRecord)));
    ix->d_offsets = static_cast<uint64_t*>(bl_ctx_pool_alloc(ctx, (size_t)(li.n_records + 1) * sizeof(uint64_t)));
    unsigned int* d_err = static_cast<unsigned int*>(bl_ctx_scratch(ctx, 6, 128));
    if (!ix->d_records || !ix->d_offsets || !d_err) return fail(bl_set_error(BL_ERR_OOM, "device allocation failed (text index)"));
    hipStream_t s = bl_ctx_stream(ctx);
    hipError_t e = hipMemsetAsync(ix->d_offsets, 0, sizeof(uint64_t), s);  // (a text of no record: the one entry)
    if (e != hipSuccess) return fail(hip_rc(e));
    unsigned int err = 0;
    if (li.n_lines) {
        e = hipMemsetAsync(d_err, 0, sizeof(unsigned int), s);
        if (e != hipSuccess) return fail(hip_rc(e));
        hipLaunchKernelGGL(index_kernel, dim3(blocks_for(li.n_lines, TPB)), dim3(TPB), 0, s, ix->d_text, li, ix->d_records, ix->d_offsets, d_err);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return fail(hip_rc(e));
    }
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(hip_rc(e));
    if (err) return fail(invalid("a record's name or the distance from its name to its quality line does not fit 32 bits"));
    return BL_OK;
}

}  // namespace

}  // namespace blfmt

// The reader's path (bl_ingest.cpp): the text is on the device already; the index takes its own copy of text[0, n_bytes).
int bl_text_index_from_device(bl_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, char first_byte, const char* ends, uint64_t ends_n, bl_batch** out_batch,
                              bl_text_index** out_index, uint64_t* n_seqs, uint64_t* n_bases)
{
    using namespace blfmt;
    if (!ctx || !out_batch || !out_index || !d_text || n_bytes == 0) return blh::invalid("NULL argument");
    *out_batch = nullptr;
    *out_index = nullptr;
    if (hipSetDevice(bl_ctx_device(ctx)) != hipSuccess) return bl_set_error(BL_ERR_HIP, "hipSetDevice failed");
    bl_text_index* ix = new bl_text_index();
    ix->ctx = ctx;
    ix->n_bytes = n_bytes;
    ix->d_text = static_cast<uint8_t*>(bl_ctx_pool_alloc(ctx, (size_t)n_bytes + 64));
    if (!ix->d_text) {
        free_index(ix);
        return bl_set_error(BL_ERR_OOM, "device allocation failed (text)");
    }
    const hipError_t e = hipMemcpyAsync(ix->d_text, d_text, n_bytes, hipMemcpyDeviceToDevice, bl_ctx_stream(ctx));
    int rc = e == hipSuccess ? index_device_text(ctx, ix, first_byte, ends, ends_n, out_batch, n_seqs, n_bases) : hip_rc(e);
    if (rc != BL_OK) {
        (void)hipStreamSynchronize(bl_ctx_stream(ctx));
        free_index(ix);
        return rc;
    }
    *out_index = ix;
    return BL_OK;
}

extern "C" int bl_text_index_build(bl_ctx* ctx, const char* text, uint64_t n_bytes, bl_batch** out_batch, bl_text_index** out_index, uint64_t* n_seqs,
                                   uint64_t* n_bases)
{
    using namespace blfmt;
    if (!ctx || !out_batch || !out_index || (n_bytes && !text)) return blh::invalid("NULL argument");
    *out_batch = nullptr;
    *out_index = nullptr;
    if (n_seqs) *n_seqs = 0;
    if (n_bases) *n_bases = 0;
    if (hipSetDevice(bl_ctx_device(ctx)) != hipSuccess) return bl_set_error(BL_ERR_HIP, "hipSetDevice failed");
    bl_text_index* ix = new bl_text_index();
    ix->ctx = ctx;
    ix->n_bytes = n_bytes;
    int rc = BL_OK;
    if (n_bytes == 0) {
        rc = bl_batch_upload(ctx, "", 0, nullptr, 0, out_batch);
        if (rc == BL_OK) {
            ix->d_offsets = static_cast<uint64_t*>(bl_ctx_pool_alloc(ctx, sizeof(uint64_t)));
            if (!ix->d_offsets || hipMemset(ix->d_offsets, 0, sizeof(uint64_t)) != hipSuccess) {
                bl_batch_destroy(*out_batch);
                *out_batch = nullptr;
                rc = bl_set_error(BL_ERR_OOM, "device allocation failed (text index)");
            }
        }
    } else {
        ix->d_text = static_cast<uint8_t*>(bl_ctx_pool_alloc(ctx, (size_t)n_bytes + 64));
        if (!ix->d_text) rc = bl_set_error(BL_ERR_OOM, "device allocation failed (text)");
        if (rc == BL_OK) {
            const hipError_t e = hipMemcpyAsync(ix->d_text, text, n_bytes, hipMemcpyHostToDevice, bl_ctx_stream(ctx));
            if (e != hipSuccess) rc = bl_set_error(BL_ERR_HIP, hipGetErrorString(e));
        }
        if (rc == BL_OK) {
            const uint64_t ends_n = n_bytes < 64 ? n_bytes : 64;
            rc = index_device_text(ctx, ix, text[0], text + (n_bytes - ends_n), ends_n, out_batch, n_seqs, n_bases);
        }
        if (rc != BL_OK) (void)hipStreamSynchronize(bl_ctx_stream(ctx));  // the copy out of the caller's buffer is over when we return
    }
    if (rc != BL_OK) {
        free_index(ix);
        return rc;
    }
    *out_index = ix;
    return BL_OK;
}

extern "C" int bl_text_index_info(const bl_text_index* ix, uint64_t* n_records, int* is_fastq, const uint8_t** d_text, uint64_t* n_bytes, const void** d_records)
{
    if (!ix) return blh::invalid("NULL argument");
    if (n_records) *n_records = ix->n_records;
    if (is_fastq) *is_fastq = ix->fastq;
    if (d_text) *d_text = ix->d_text;
    if (n_bytes) *n_bytes = ix->n_bytes;
    if (d_records) *d_records = ix->d_records;
    return BL_OK;
}

extern "C" const uint64_t* bl_text_index_offsets(const bl_text_index* ix) { return ix ? ix->d_offsets : nullptr; }

int bl_text_index_describe(const bl_text_index* ix, bl_ctx** ctx, uint64_t* n_bases)
{
    if (!ix) return blh::invalid("NULL argument");
    *ctx = ix->ctx;
    *n_bases = ix->n_bases;
    return BL_OK;
}

extern "C" int bl_text_index_destroy(bl_text_index* ix)
{
    if (!ix) return BL_OK;
    if (ix->ctx) {
        (void)hipSetDevice(bl_ctx_device(ix->ctx));
        (void)hipStreamSynchronize(bl_ctx_stream(ix->ctx));  // a format that reads it may be in flight
    }
    blfmt::free_index(ix);
    return BL_OK;
}

extern "C" int bl_batch_format(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const bl_text_index* index, const uint64_t* d_source_index,
                               const uint64_t* d_spans, const uint64_t* d_tags, const bl_format_rule* rule, uint8_t* d_out, uint64_t capacity,
                               uint64_t* n_bytes, uint64_t* n_records)
{
    using namespace blfmt;
    if (!ctx || !batch || !rule) return invalid("ctx, batch or rule is NULL");
    if (n_bytes) *n_bytes = 0;
    if (n_records) *n_records = 0;
    if (rule->format != BL_FORMAT_FASTA && rule->format != BL_FORMAT_FASTQ) return invalid("bl_format_rule: format is BL_FORMAT_FASTA or BL_FORMAT_FASTQ");
    if (rule->flags & ~(uint32_t)(BL_FORMAT_SKIP_EMPTY | BL_FORMAT_TAG_LENGTH)) return invalid("bl_format_rule: unknown flag bits");
    if (rule->format == BL_FORMAT_FASTQ && rule->line_width != 0) return invalid("bl_format_rule: line_width must be 0 for FASTQ");
    if (rule->quality_fill < 33 || rule->quality_fill > 126) return invalid("bl_format_rule: quality_fill is a byte 33 .. 126");
    const int prefix_len = terminated_length(rule->name_prefix), label_len = terminated_length(rule->tag_label);
    if (prefix_len < 0 || label_len < 0) return invalid("bl_format_rule: name_prefix and tag_label are NUL-terminated inside their 16 bytes");
    if (rule->reserved != 0) return invalid("bl_format_rule: reserved must be 0");
    if (blh::misaligned16(d_spans)) return invalid("d_spans must be 16-byte aligned");
    if (blh::misaligned16(d_out)) return invalid("d_out must be 16-byte aligned");
    if (index && index->ctx != ctx) return invalid("the index belongs to another context");
    blh::BatchView view;
    BLH_OK(blh::batch_view(ctx, batch, view));
    BLH_OK(blh::offsets_needed(d_offsets, view.n_seqs, view.read_len));
    FormatParams p{};
    p.n_bases = view.n_bases;
    p.n_seqs = view.n_seqs;
    p.read_len = d_offsets ? 0 : (view.read_len ? view.read_len : (p.n_bases ? p.n_bases : 1));
    p.full_reads = p.read_len ? p.n_bases / p.read_len : 0;
    p.bases = view.bases;
    p.offsets = d_offsets;
    if (index && index->n_records) {
        p.text = index->d_text;
        p.n_text = index->n_bytes;
        p.records = index->d_records;
        p.index_offsets = index->d_offsets;
        p.n_records = index->n_records;
        p.index_fastq = index->fastq ? 1u : 0u;
    }
    p.source_index = d_source_index;
    p.spans = d_spans;
    p.tags = d_tags;
    p.format = rule->format;
    p.flags = rule->flags;
    p.line_width = rule->line_width;
    p.quality_fill = rule->quality_fill;
    pack_prefix(rule->name_prefix, prefix_len, p.prefix);
    pack_prefix(rule->tag_label, label_len, p.label);
    p.prefix_len = (uint32_t)prefix_len;
    p.label_len = (uint32_t)label_len;
    p.first_number = rule->first_number;

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the context's scans in flight
    const uint64_t n1 = p.n_seqs + 1;
    // slot 4: lengths, flags, their two sums and the descriptions (behind 32 * n1 bytes: 16-byte aligned)
    uint64_t* arena = static_cast<uint64_t*>(bl_ctx_scratch(ctx, 4, (size_t)(4 * n1) * sizeof(uint64_t) + (size_t)n1 * sizeof(Desc)));
    if (!arena) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    p.rec_len = arena;
    p.written = arena + n1;
    uint64_t* rec_off = arena + 2 * n1;
    uint64_t* written_sum = arena + 3 * n1;
    p.rec_off = rec_off;
    p.desc = reinterpret_cast<Desc*>(arena + 4 * n1);

    hipLaunchKernelGGL(record_length_kernel, dim3(blocks_for(n1, TPB)), dim3(TPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    BLH_OK(exclusive_sum(ctx, p.rec_len, rec_off, (size_t)n1, s));
    BLH_OK(exclusive_sum(ctx, p.written, written_sum, (size_t)n1, s));  // (the first sum is done with slot 5: same stream)
    unsigned long long total = 0, n_written = 0;
    BLH_TRY(hipMemcpyAsync(&total, rec_off + p.n_seqs, sizeof(total), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipMemcpyAsync(&n_written, written_sum + p.n_seqs, sizeof(n_written), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (n_bytes) *n_bytes = total;
    if (n_records) *n_records = n_written;
    if (!d_out) return BL_OK;  // sizing only
    if (capacity < total) return bl_set_error(BL_ERR_CAPACITY, "bl_batch_format: d_out is smaller than the text (*n_bytes says how large it is)");
    if (total == 0) return BL_OK;
    p.total = total;
    p.out = d_out;
    const uint64_t waves = (total + WAVE_BYTES - 1) / WAVE_BYTES;
    hipLaunchKernelGGL(format_kernel, dim3(blocks_for(waves * 64, TPB)), dim3(TPB), 0, s, p);
    BLH_TRY(hipGetLastError());
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}

// Device text to a file: chunks of WRITE_CHUNK bytes through two pinned buffers, chunk c + 1 copying while chunk c is written.
extern "C" int bl_text_write(bl_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const char* path, int append)
{
    constexpr size_t WRITE_CHUNK = (size_t)8 << 20;
    if (!ctx || !path || (n_bytes && !d_text)) return blh::invalid("NULL argument");
    hipError_t e = hipSetDevice(bl_ctx_device(ctx));
    if (e != hipSuccess) return blh::hip_rc(e);
    FILE* f = std::fopen(path, append ? "ab" : "wb");
    if (!f) return bl_set_error(BL_ERR_IO, (std::string("cannot open ") + path + ": " + std::strerror(errno)).c_str());
    hipStream_t s = bl_ctx_stream(ctx);
    uint8_t* buf[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    const size_t chunk = n_bytes < WRITE_CHUNK ? (size_t)n_bytes : WRITE_CHUNK;
    int rc = BL_OK;
    for (int i = 0; i < 2 && rc == BL_OK && n_bytes; ++i) {
        e = hipHostMalloc(reinterpret_cast<void**>(&buf[i]), chunk ? chunk : 1, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
        if (e != hipSuccess) rc = blh::hip_rc(e);
    }
    const uint64_t n_chunks = n_bytes ? (n_bytes + chunk - 1) / chunk : 0;
    auto enqueue = [&](uint64_t c) {
        const uint64_t at = c * chunk, n = n_bytes - at < chunk ? n_bytes - at : chunk;
        hipError_t err = hipMemcpyAsync(buf[c & 1], d_text + at, n, hipMemcpyDeviceToHost, s);
        if (err == hipSuccess) err = hipEventRecord(done[c & 1], s);
        return err;
    };
    if (rc == BL_OK && n_chunks) {
        e = enqueue(0);
        if (e != hipSuccess) rc = blh::hip_rc(e);
    }
    for (uint64_t c = 0; c < n_chunks && rc == BL_OK; ++c) {
        if (c + 1 < n_chunks) {  // (buffer (c + 1) & 1 was written out in the step before)
            e = enqueue(c + 1);
            if (e != hipSuccess) { rc = blh::hip_rc(e); break; }
        }
        e = hipEventSynchronize(done[c & 1]);
        if (e != hipSuccess) { rc = blh::hip_rc(e); break; }
        const uint64_t at = c * chunk, n = n_bytes - at < chunk ? n_bytes - at : chunk;
        if (std::fwrite(buf[c & 1], 1, n, f) != n) rc = bl_set_error(BL_ERR_IO, (std::string("short write to ") + path + ": " + std::strerror(errno)).c_str());
    }
    (void)hipStreamSynchronize(s);  // nothing copies into the buffers when they go
    if (std::fclose(f) != 0 && rc == BL_OK) rc = bl_set_error(BL_ERR_IO, (std::string("closing ") + path + ": " + std::strerror(errno)).c_str());
    for (int i = 0; i < 2; ++i) {
        if (done[i]) (void)hipEventDestroy(done[i]);
        if (buf[i]) (void)hipHostFree(buf[i]);
    }
    return rc;
}
