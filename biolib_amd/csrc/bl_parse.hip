// bl_parse.hip — device-side FASTA / FASTQ text parser: the raw file bytes are copied to HBM once and turned into
// a batch THERE (newline index -> line classification -> prefix sums -> gather of the sequence lines), so ingest
// runs at PCIe speed instead of at the speed of one host thread (the host reader of
// bl_ingest.cpp stays the general path and the semantic reference, itself pinned against the reference's kseq).
// Accepted on this path: FASTQ with exactly four lines per record (at most three blank lines behind the last one), FASTA with
// any line wrapping; LF or CRLF; the last line may lack its terminator.
// Anything irregular is refused with BL_ERR_INVALID (never silently mis-parsed): use bl_reader_* for those files.  Refused are
//   * a text that starts with neither '>' nor '@'; FASTQ whose lines are not '@' header, sequence, '+' separator, quality of
//     the sequence's length, four by four
//   * a FASTQ sequence line, or a FASTA line that is no header, that opens with a byte which ends the sequence in the
//     reference reader: '>', '@' or '+' in FASTQ, '@' or '+' in FASTA
//   * a line that is a lone '\r' where the reference reader counts it as a base (it drops a trailing '\r' only from more than
//     one gathered byte): a FASTQ sequence or quality line, and a FASTA line with nothing of its record gathered in front of it
//     (after the scans: its dst equals its record's offset).  The same FASTA line behind bases vanishes there as it does here.
// The per-thread bodies of the kernels and the host's decisions on the text's ends are in bl_parse_core.hpp, which also compiles
// for the host: tests/emu/emu_parse.cpp runs them under the sanitizers on the texts of tests/parse_cases.py.
#include <hip/hip_runtime.h>
#include <cstring>
#include <rocprim/device/device_scan.hpp>
#include <string>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"
#include "bl_parse_core.hpp"

namespace {

using namespace bl_parse;

__global__ __launch_bounds__(PB) void count_newlines_kernel(const uint8_t* text, uint64_t n, unsigned long long* block_count)
{
    __shared__ unsigned int wsum[PB / 64];
    unsigned int c = __builtin_popcount(chunk_mask(text, n, chunk_at(blockIdx.x, threadIdx.x)));
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// line_end[i] = byte offset of the i-th '\n'
__global__ __launch_bounds__(PB) void newline_positions_kernel(const uint8_t* text, uint64_t n, const unsigned long long* block_base,
                                                               unsigned long long* line_end)
{
    __shared__ unsigned int wsum[PB / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t at = chunk_at(blockIdx.x, threadIdx.x);
    const uint32_t m = chunk_mask(text, n, at);
    const unsigned int c = __builtin_popcount(m);
    unsigned int incl = c;
    for (int d = 1; d < 64; d <<= 1) incl = scan_step(incl, __shfl_up(incl, d, 64), lane, d);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    unsigned int before = 0;
    for (int i = 0; i < wv; ++i) before += wsum[i];
    write_newline_positions(m, at, block_base[blockIdx.x] + before + incl - c, line_end);
}

// one thread per line: kind, sequence length (0 unless a sequence line), header flag; format checks
__global__ void classify_lines_kernel(const uint8_t* text, const unsigned long long* line_end, uint64_t n_lines, int fastq,
                                      unsigned long long* seq_len, unsigned long long* hdr, unsigned int* err)
{
    const uint64_t li = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n_lines) return;
    unsigned long long len, h;
    const unsigned int e = classify_line(text, line_end, li, fastq, len, h);
    if (e) atomicOr(err, e);
    seq_len[li] = len;
    hdr[li] = h;
}

// FASTA: lines in front of the first header belong to no record
__global__ void mask_leading_lines_kernel(const unsigned long long* rec_incl, unsigned long long* seq_len, uint64_t n_lines)
{
    const uint64_t li = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li < n_lines) mask_leading_line(rec_incl, seq_len, li);
}

// offsets[r] = first base of record r (r = rec_incl - 1 at its header line); offsets[n_records] = total
__global__ void record_offsets_kernel(const unsigned long long* hdr, const unsigned long long* rec_incl, const unsigned long long* dst,
                                      uint64_t n_lines, unsigned long long* offsets, uint64_t n_records, uint64_t total)
{
    record_offset_line(hdr, rec_incl, dst, n_lines, offsets, n_records, total, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// FASTA texts that hold a lone-'\r' line (rare: launched only then, after record_offsets_kernel): refuse where it opens a record
__global__ void lone_cr_lines_kernel(const uint8_t* text, const unsigned long long* line_end, const unsigned long long* hdr,
                                     const unsigned long long* rec_incl, const unsigned long long* dst, const unsigned long long* offsets,
                                     uint64_t n_lines, unsigned int* err)
{
    const uint64_t li = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li < n_lines && lone_cr_opens_record(text, line_end, hdr, rec_incl, dst, offsets, li)) atomicOr(err, (unsigned)ERR_LONE_CR);
}

// do all records hold exactly `len` bases?  (flag |= 1 where one does not)
__global__ void uniform_length_kernel(const unsigned long long* offsets, uint64_t n_records, uint64_t len, unsigned int* flag)
{
    if (breaks_uniform_length(offsets, n_records, len, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x)) atomicOr(flag, 1u);
}

// one thread per 16 output bytes
__global__ void gather_bases_kernel(const uint8_t* text, const unsigned long long* line_end, const unsigned long long* dst,
                                    const unsigned long long* seq_len, uint64_t n_lines, uint8_t* bases, uint64_t total)
{
    const uint64_t x0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (x0 < total) gather16(text, line_end, dst, seq_len, n_lines, bases, total, x0);
}

// Waits for the stream on the way out of the parser, once: nothing may still be running on the scratch, or on the outputs when they go.
struct Drain {
    hipStream_t s;
    bool armed = true;
    void now()
    {
        if (armed) (void)hipStreamSynchronize(s);
        armed = false;
    }
    ~Drain() { now(); }
};

}  // namespace

// The parser proper, over text that is in device memory already.  `ends` is the host's copy of the text's last `ends_n` bytes
// (all of it when the text is shorter than 64): the few decisions taken on the host look at the first byte and at the end only.
int bl_parse_device_text(bl_ctx* ctx, const uint8_t* d_text_in, uint64_t n_bytes, char first_byte, const char* ends, uint64_t ends_n, bl_batch** out,
                         uint64_t* n_seqs, uint64_t* n_bases);
// The same, and (lines != NULL) where the line arrays it leaves in scratch slot 1 are: valid until the context's next parse.  bl_format.hip
// builds the record index of a text from them.  With lines NULL the launches and the results are those of bl_parse_device_text.
int bl_parse_device_text_lines(bl_ctx* ctx, const uint8_t* d_text_in, uint64_t n_bytes, char first_byte, const char* ends, uint64_t ends_n, bl_batch** out,
                               uint64_t* n_seqs, uint64_t* n_bases, bl_parse::LineIndex* lines);

extern "C" int bl_batch_from_text(bl_ctx* ctx, const char* text, uint64_t n_bytes, bl_batch** out, uint64_t* n_seqs, uint64_t* n_bases)
{
    if (!ctx || !out || (n_bytes && !text)) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (n_seqs) *n_seqs = 0;
    if (n_bases) *n_bases = 0;
    if (n_bytes == 0) return bl_batch_upload(ctx, "", 0, nullptr, 0, out);
    if (hipSetDevice(bl_ctx_device(ctx)) != hipSuccess) return bl_set_error(BL_ERR_HIP, "hipSetDevice failed");
    uint8_t* d_text = static_cast<uint8_t*>(bl_ctx_scratch(ctx, 3, n_bytes + 64));
    if (!d_text) return bl_set_error(BL_ERR_OOM, "device allocation failed (text)");
    const hipError_t e = hipMemcpyAsync(d_text, text, n_bytes, hipMemcpyHostToDevice, bl_ctx_stream(ctx));
    if (e != hipSuccess) return bl_set_error(BL_ERR_HIP, hipGetErrorString(e));
    const uint64_t ends_n = n_bytes < 64 ? n_bytes : 64;
    const int rc = bl_parse_device_text(ctx, d_text, n_bytes, text[0], text + (n_bytes - ends_n), ends_n, out, n_seqs, n_bases);
    if (rc != BL_OK) (void)hipStreamSynchronize(bl_ctx_stream(ctx));  // the copy out of the caller's buffer is over when we return
    return rc;
}

int bl_parse_device_text(bl_ctx* ctx, const uint8_t* d_text_in, uint64_t n_bytes, char first_byte, const char* ends, uint64_t ends_n, bl_batch** out,
                         uint64_t* n_seqs, uint64_t* n_bases)
{
    return bl_parse_device_text_lines(ctx, d_text_in, n_bytes, first_byte, ends, ends_n, out, n_seqs, n_bases, nullptr);
}

int bl_parse_device_text_lines(bl_ctx* ctx, const uint8_t* d_text_in, uint64_t n_bytes, char first_byte, const char* ends, uint64_t ends_n, bl_batch** out,
                               uint64_t* n_seqs, uint64_t* n_bases, bl_parse::LineIndex* lines)
{
    if (lines) *lines = bl_parse::LineIndex{};
    if (!ctx || !out || !d_text_in || !ends || ends_n == 0 || ends_n > n_bytes) return bl_set_error(BL_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (n_seqs) *n_seqs = 0;
    if (n_bases) *n_bases = 0;
    auto last = [&](uint64_t back) { return ends[ends_n - 1 - back]; };  // the text's byte `back` places in front of its last one
    // the format is decided by the first character
    const bool fastq = first_byte == '@';
    if (!fastq && first_byte != '>') return bl_set_error(BL_ERR_INVALID, "text starts with neither '>' nor '@': use bl_reader_* for irregular files");
    if (drops_trailing_marker(fastq, ends, ends_n, n_bytes)) {
        --n_bytes;
        --ends_n;
        if (n_bytes == 0) return bl_batch_upload(ctx, "", 0, nullptr, 0, out);
    }
    const bool open_last_line = last(0) != '\n';  // the last line has no terminator: a virtual one is added

    hipStream_t s = bl_ctx_stream(ctx);
    // Temporary arrays come from the context's grow-only scratch (slot 0: block counts, slot 1: per-line arrays, slot 2: scan
    // workspace; slot 3 holds the text when it came from the host): a file is parsed span after span, and a dozen hipMalloc /
    // hipFree per span cost more than the kernels.  Only the two arrays the batch keeps are allocated here.
    const uint8_t* d_text = nullptr;
    unsigned long long *d_blk = nullptr, *d_line_end = nullptr, *d_len = nullptr, *d_hdr = nullptr, *d_rec = nullptr, *d_dst = nullptr;
    unsigned int* d_err = nullptr;
    blh::Pooled<uint8_t> d_bases;  // the outputs go on every exit path unless adopted ...
    blh::Pooled<unsigned long long> d_offsets;
    Drain drain{s};  // ... behind the wait for the stream (declared last: it goes first)
    auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };

    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    const uint64_t n = n_bytes;
    const unsigned n_blocks = (unsigned)((n + BYTES_PER_BLOCK - 1) / BYTES_PER_BLOCK);
    const size_t blk_bytes = up256(2 * ((size_t)n_blocks + 1) * sizeof(unsigned long long));
    unsigned char* a0 = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 0, blk_bytes + 256));
    if (!a0) return bl_set_error(BL_ERR_OOM, "device allocation failed (block scratch)");
    d_text = d_text_in;
    d_blk = reinterpret_cast<unsigned long long*>(a0);  // counts, then their exclusive prefix
    d_err = reinterpret_cast<unsigned int*>(a0 + blk_bytes);
    unsigned long long* d_blk_base = d_blk + n_blocks + 1;
    BLH_TRY(hipMemsetAsync(d_blk + n_blocks, 0, sizeof(unsigned long long), s));
    BLH_TRY(hipMemsetAsync(d_err, 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(count_newlines_kernel, dim3(n_blocks), dim3(PB), 0, s, d_text, n, d_blk);

    // the three scans: each takes its workspace from slot 2 (which grows with the largest of them)
    auto scan = [&](auto&& call) {
        const hipError_t e = blh::with_workspace(ctx, 2, call);
        if (e == hipErrorOutOfMemory) return bl_set_error(BL_ERR_OOM, "device allocation failed (scan scratch)");
        return e == hipSuccess ? (int)BL_OK : blh::hip_rc(e);
    };
    const rocprim::plus<unsigned long long> plus;
    int rc = scan([&](void* ws, size_t& bytes) { return rocprim::exclusive_scan(ws, bytes, d_blk, d_blk_base, 0ull, (size_t)n_blocks + 1, plus, s); });
    if (rc != BL_OK) return rc;
    unsigned long long n_newlines = 0;
    BLH_TRY(hipMemcpyAsync(&n_newlines, d_blk_base + n_blocks, sizeof(n_newlines), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    const uint64_t n_lines_raw = n_newlines + (open_last_line ? 1 : 0);
    uint64_t n_lines = n_lines_raw;
    if (fastq && (n_lines & 3)) {  // blank lines after the last record are tolerated, anything else is not 4-line FASTQ
        const uint64_t excess = n_lines & 3;
        if (!trailing_lines_blank(ends, ends_n, n_bytes, open_last_line, excess))
            return bl_set_error(BL_ERR_INVALID, "FASTQ text is not made of 4-line records: use bl_reader_*");
        n_lines -= excess;
        if (n_lines == 0) {  // a span of the blank lines behind a file's last record
            drain.armed = false;  // (the stream has just been waited for)
            return bl_batch_upload(ctx, "", 0, nullptr, 0, out);
        }
    }

    {
        const size_t per = up256((n_lines_raw + 2) * sizeof(unsigned long long));
        unsigned char* a1 = static_cast<unsigned char*>(bl_ctx_scratch(ctx, 1, 5 * per));
        if (!a1) return bl_set_error(BL_ERR_OOM, "device allocation failed (line scratch)");
        d_line_end = reinterpret_cast<unsigned long long*>(a1);
        d_len = reinterpret_cast<unsigned long long*>(a1 + per);
        d_hdr = reinterpret_cast<unsigned long long*>(a1 + 2 * per);
        d_rec = reinterpret_cast<unsigned long long*>(a1 + 3 * per);
        d_dst = reinterpret_cast<unsigned long long*>(a1 + 4 * per);
    }
    hipLaunchKernelGGL(newline_positions_kernel, dim3(n_blocks), dim3(PB), 0, s, d_text, n, d_blk_base, d_line_end);
    if (open_last_line) BLH_TRY(hipMemcpyAsync(d_line_end + n_newlines, &n, sizeof(unsigned long long), hipMemcpyHostToDevice, s));  // virtual '\n'
    BLH_TRY(hipMemsetAsync(d_len + n_lines, 0, sizeof(unsigned long long), s));
    const unsigned lb = (unsigned)((n_lines + 255) / 256);
    hipLaunchKernelGGL(classify_lines_kernel, dim3(lb), dim3(256), 0, s, d_text, d_line_end, n_lines, fastq ? 1 : 0, d_len, d_hdr, d_err);

    rc = scan([&](void* ws, size_t& bytes) { return rocprim::inclusive_scan(ws, bytes, d_hdr, d_rec, (size_t)n_lines, plus, s); });
    if (rc != BL_OK) return rc;
    if (!fastq) hipLaunchKernelGGL(mask_leading_lines_kernel, dim3(lb), dim3(256), 0, s, d_rec, d_len, n_lines);
    rc = scan([&](void* ws, size_t& bytes) { return rocprim::exclusive_scan(ws, bytes, d_len, d_dst, 0ull, (size_t)n_lines + 1, plus, s); });
    if (rc != BL_OK) return rc;

    unsigned long long total = 0, n_records = 0;
    unsigned int err = 0;
    BLH_TRY(hipMemcpyAsync(&total, d_dst + n_lines, sizeof(total), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipMemcpyAsync(&n_records, d_rec + (n_lines - 1), sizeof(n_records), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (err & ERR_MASK) return bl_set_error(BL_ERR_INVALID, refusal_message(err));
    const bool lone_cr_seen = (err & NOTE_FASTA_LONE_CR) != 0;  // FASTA only: refused where such a line opens its record

    d_bases = blh::Pooled<uint8_t>(ctx, total + 64);
    d_offsets = blh::Pooled<unsigned long long>(ctx, (n_records + 1) * sizeof(unsigned long long));
    if (!d_bases || !d_offsets) return bl_set_error(BL_ERR_OOM, "device allocation failed (batch)");
    BLH_TRY(hipMemsetAsync(d_bases.get() + (total & ~15ull), 0, 64 + (total & 15ull), s));
    if (total) {
        const uint64_t threads = (total + 15) / 16;
        hipLaunchKernelGGL(gather_bases_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, d_text, d_line_end, d_dst, d_len, n_lines,
                           d_bases.get(), (uint64_t)total);
    }
    hipLaunchKernelGGL(record_offsets_kernel, dim3(lb), dim3(256), 0, s, d_hdr, d_rec, d_dst, n_lines, d_offsets.get(), (uint64_t)n_records, (uint64_t)total);
    // reads of one length (the usual short-read file) make a fixed-length batch: the read-tiled scan kernels, no start-bit vector
    if (lone_cr_seen) {
        hipLaunchKernelGGL(lone_cr_lines_kernel, dim3(lb), dim3(256), 0, s, d_text, d_line_end, d_hdr, d_rec, d_dst, d_offsets.get(), n_lines, d_err);
        BLH_TRY(hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
    }
    uint64_t fixed_len = n_records > 1 && total % n_records == 0 ? total / n_records : 0;
    unsigned int ragged = 0;
    if (fixed_len) {
        BLH_TRY(hipMemsetAsync(d_err + 1, 0, sizeof(unsigned int), s));
        hipLaunchKernelGGL(uniform_length_kernel, dim3(uniform_length_blocks(n_records)), dim3(256), 0, s, d_offsets.get(), (uint64_t)n_records, fixed_len, d_err + 1);
        BLH_TRY(hipMemcpyAsync(&ragged, d_err + 1, sizeof(ragged), hipMemcpyDeviceToHost, s));
    }
    BLH_TRY(hipGetLastError());
    BLH_TRY(hipStreamSynchronize(s));
    if (err & ERR_MASK) return bl_set_error(BL_ERR_INVALID, refusal_message(err));
    if (ragged) fixed_len = 0;
    drain.now();
    if (lines) *lines = bl_parse::LineIndex{d_line_end, d_hdr, d_rec, d_dst, n_lines, n_records, total, fastq ? 1 : 0};
    rc = bl_batch_adopt_device(ctx, d_bases.release(), total, reinterpret_cast<uint64_t*>(d_offsets.release()), n_records, fixed_len, out);  // takes ownership of both
    if (rc != BL_OK) return rc;
    if (n_seqs) *n_seqs = n_records;
    if (n_bases) *n_bases = total;
    return BL_OK;
}
