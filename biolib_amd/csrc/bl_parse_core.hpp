// bl_parse_core.hpp — the per-thread bodies of the device-side FASTA / FASTQ parser (bl_parse.hip) and the few decisions its
// host driver takes on the first byte and the last 64 bytes of a text.
//
// Written once and compiled two ways, like bl_scan_core.hpp:
//   * by hipcc for gfx950 (bl_parse.hip): BL_PDEV = __device__ __forceinline__; the kernels keep the launch shapes and the
//     cross-lane steps (shuffles, LDS, atomics) and call these functions
//   * by a host compiler for tests/emu/emu_parse.cpp, which runs the same pipeline thread by thread under the sanitizers over
//     buffers of exactly the sizes the library allocates.  The harness is test infrastructure; the product is the HIP build.
//
// What a text must look like to be parsed here, and what is refused, is stated at the head of bl_parse.hip.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) && !defined(BL_CPU_EMU)
#define BL_PDEV __device__ __forceinline__
#else
#define BL_PDEV static inline
#endif

namespace bl_parse {

constexpr int PB = 256;                  // threads per block of the two newline kernels
constexpr int BYTES_PER_BLOCK = PB * 16;  // 16 bytes of text per thread
constexpr int LINE_THREADS = 256;        // threads per block of the per-line, per-record and gather kernels

enum { KIND_OTHER = 0, KIND_SEQ = 1, KIND_HEADER = 2 };
// refusals (the first six) and one notice: FASTA_LONE_CR says that the text holds a sequence line that is a lone '\r'; whether
// it is refused is known only after the scans (lone_cr_line below)
enum {
    ERR_FASTQ_HEADER = 1,
    ERR_FASTQ_PLUS = 2,
    ERR_FASTQ_QUAL = 4,
    ERR_FASTA_SEQLINE = 8,
    ERR_FASTQ_SEQLINE = 16,
    ERR_LONE_CR = 32,
    NOTE_FASTA_LONE_CR = 64,
    ERR_MASK = 63
};

// What a parse leaves behind for the record index of bl_format.hip: the per-line arrays (device, the context's scratch) of the text
// just parsed.  All zero where the text held no record.
struct LineIndex {
    const unsigned long long *line_end, *hdr, *rec_incl, *dst;  // [n_lines] (dst: n_lines + 1)
    uint64_t n_lines, n_records, total;
    int fastq;
};

// bit b set <=> text[at + b] == '\n', for the 16 bytes at `at` (a multiple of 16; text is 16-byte aligned).  Whole chunks are
// tested four bytes at a time, the text's last partial chunk byte by byte: nothing behind text[n - 1] is read.
BL_PDEV uint32_t newline_mask16(const uint8_t* text, uint64_t n, uint64_t at)
{
    uint32_t m = 0;
    if (at + 16 <= n) {
#if defined(__HIPCC__) && !defined(BL_CPU_EMU)
        const uint4 v = *reinterpret_cast<const uint4*>(text + at);
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#else
        uint32_t d[4];
        memcpy(d, text + at, 16);
#endif
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = d[i] ^ 0x0a0a0a0au;                                        // zero byte <=> '\n'
            const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;  // bit 7 of every zero byte
            m |= (((z >> 7) * 0x00204081u >> 21) & 0xfu) << (4 * i);
        }
    } else {
        for (int b = 0; b < 16 && at + b < n; ++b)
            if (text[at + b] == '\n') m |= 1u << b;
    }
    return m;
}

// the chunk a thread of the newline kernels owns, and its mask (0 behind the text)
BL_PDEV uint64_t chunk_at(uint64_t block, int thread) { return (block * PB + (uint64_t)thread) * 16; }
BL_PDEV uint32_t chunk_mask(const uint8_t* text, uint64_t n, uint64_t at) { return at < n ? newline_mask16(text, n, at) : 0; }

// one step of the wave's inclusive scan: `o` is the value of the lane `d` places below (meaningless where there is none)
BL_PDEV unsigned int scan_step(unsigned int incl, unsigned int o, int lane, int d) { return lane >= d ? incl + o : incl; }

// line_end[idx ...] = byte offsets of the chunk's newlines
BL_PDEV void write_newline_positions(uint32_t m, uint64_t at, unsigned long long idx, unsigned long long* line_end)
{
    while (m) {
        const int b = __builtin_ctz(m);
        m &= m - 1;
        line_end[idx++] = at + b;
    }
}

// [start, end) of line li without its terminator: '\n', or "\r\n" (one '\r' is dropped, as the reference reader does)
BL_PDEV void line_span(const uint8_t* text, const unsigned long long* line_end, uint64_t li, uint64_t& start, uint64_t& end)
{
    start = li ? line_end[li - 1] + 1 : 0;
    end = line_end[li];
    if (end > start && text[end - 1] == '\r') --end;
}

// is line li a '\r' and nothing else?  The reference reader drops a trailing '\r' only from more than one gathered byte, so such
// a line adds a base where nothing of its record has been gathered yet; line_span makes it an empty line.
BL_PDEV bool lone_cr(const uint8_t* text, const unsigned long long* line_end, uint64_t li)
{
    const uint64_t start = li ? line_end[li - 1] + 1 : 0;
    return line_end[li] == start + 1 && text[start] == '\r';
}

// one line: sequence length (0 unless a sequence line), header flag; returns the ERR_ / NOTE_ bits of the format checks
BL_PDEV unsigned int classify_line(const uint8_t* text, const unsigned long long* line_end, uint64_t li, int fastq, unsigned long long& len,
                                   unsigned long long& h)
{
    uint64_t s, e;
    line_span(text, line_end, li, s, e);
    const uint8_t first = e > s ? text[s] : 0;
    unsigned int err = 0;
    len = 0;
    h = 0;
    if (fastq) {
        const int f = (int)(li & 3);
        if (f == 0) {
            h = 1;
            if (first != '@') err |= ERR_FASTQ_HEADER;
        } else if (f == 1) {
            len = e - s;
            if (first == '>' || first == '@' || first == '+') err |= ERR_FASTQ_SEQLINE;  // ends the sequence in the reference reader
            if (lone_cr(text, line_end, li)) err |= ERR_LONE_CR;                          // is the base "\r" there
        } else if (f == 2) {
            if (first != '+') err |= ERR_FASTQ_PLUS;
        } else {
            uint64_t s2, e2;
            line_span(text, line_end, li - 2, s2, e2);
            if (e - s != e2 - s2) err |= ERR_FASTQ_QUAL;
            if (lone_cr(text, line_end, li)) err |= ERR_LONE_CR;  // one quality byte there
        }
    } else {
        if (first == '>') h = 1;
        else {
            len = e - s;  // masked later for lines in front of the first header
            if (first == '@' || first == '+') err |= ERR_FASTA_SEQLINE;  // would end the record in the reference reader
            if (lone_cr(text, line_end, li)) err |= NOTE_FASTA_LONE_CR;
        }
    }
    return err;
}

// FASTA: lines in front of the first header belong to no record
BL_PDEV void mask_leading_line(const unsigned long long* rec_incl, unsigned long long* seq_len, uint64_t li)
{
    if (rec_incl[li] == 0) seq_len[li] = 0;
}

// offsets[r] = first base of record r (r = rec_incl - 1 at its header line); offsets[n_records] = total
BL_PDEV void record_offset_line(const unsigned long long* hdr, const unsigned long long* rec_incl, const unsigned long long* dst, uint64_t n_lines,
                                unsigned long long* offsets, uint64_t n_records, uint64_t total, uint64_t li)
{
    if (li == 0) offsets[n_records] = total;
    if (li < n_lines && hdr[li]) offsets[rec_incl[li] - 1] = dst[li];
}

// FASTA, after the scans and the record offsets: is line li a lone '\r' with nothing of its record gathered in front of it?
// (The same line behind bases vanishes in the reference reader as it does here.)
BL_PDEV bool lone_cr_opens_record(const uint8_t* text, const unsigned long long* line_end, const unsigned long long* hdr, const unsigned long long* rec_incl,
                                  const unsigned long long* dst, const unsigned long long* offsets, uint64_t li)
{
    if (hdr[li] || rec_incl[li] == 0 || !lone_cr(text, line_end, li)) return false;
    return dst[li] == offsets[rec_incl[li] - 1];
}

// does entry r of the offsets (0 .. n_records, the total included) break "all records hold exactly `len` bases"?
BL_PDEV bool breaks_uniform_length(const unsigned long long* offsets, uint64_t n_records, uint64_t len, uint64_t r)
{
    return r <= n_records && offsets[r] != r * len;
}
inline unsigned uniform_length_blocks(uint64_t n_records) { return (unsigned)((n_records + LINE_THREADS) / LINE_THREADS); }  // n_records + 1 entries

// 16 output bytes at x0 (a multiple of 16, < total): find the sequence line that holds output byte x0 (last line with dst <= x0)
// and gather from there.  All 16 bytes are stored: bases has at least 16 bytes of slack behind `total`.
BL_PDEV void gather16(const uint8_t* text, const unsigned long long* line_end, const unsigned long long* dst, const unsigned long long* seq_len,
                      uint64_t n_lines, uint8_t* bases, uint64_t total, uint64_t x0)
{
    uint64_t lo = 0, hi = n_lines;  // first line with dst > x0
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (dst[mid] <= x0) lo = mid + 1;
        else hi = mid;
    }
    uint64_t li = lo - 1;  // dst[0] = 0 <= x0, so lo >= 1; this line has seq_len > 0
    uint32_t w[4] = {0, 0, 0, 0};
    uint64_t x = x0;
    int filled = 0;
    while (filled < 16 && x < total) {
        while (li < n_lines && seq_len[li] == 0) ++li;  // header / quality lines in between
        if (li >= n_lines) break;                        // cannot happen while x < total; keeps a logic error from running away
        const uint64_t ls = li ? line_end[li - 1] + 1 : 0;
        const uint64_t in_line = x - dst[li];
        uint64_t take = seq_len[li] - in_line;
        if (take > (uint64_t)(16 - filled)) take = 16 - filled;
        const uint8_t* src = text + ls + in_line;
        for (uint64_t b = 0; b < take; ++b, ++filled) w[filled >> 2] |= (uint32_t)src[b] << (8 * (filled & 3));
        x += take;
        if (in_line + take == seq_len[li]) ++li;
    }
#if defined(__HIPCC__) && !defined(BL_CPU_EMU)
    *reinterpret_cast<uint4*>(bases + x0) = make_uint4(w[0], w[1], w[2], w[3]);
#else
    memcpy(bases + x0, w, 16);
#endif
}

// ---- the host's decisions: the first byte, and `ends`, its copy of the text's last ends_n <= 64 bytes (all of it when shorter) ----

// a '>' that is the very last byte of the file and alone on its line opens no record in the reference reader (kseq meets end of
// file while looking for the name and reports end of input): it is dropped
inline bool drops_trailing_marker(bool fastq, const char* ends, uint64_t ends_n, uint64_t n_bytes)
{
    return !fastq && ends[ends_n - 1] == '>' && (n_bytes == 1 || ends[ends_n - 2] == '\n');
}

// FASTQ whose line count is `excess` (1..3) over a multiple of four: blank lines ("\n" or "\r\n") after the last record are
// tolerated, anything else is not 4-line FASTQ.  Are the last `excess` lines blank?  Running out of `ends` means "not blank".
inline bool trailing_lines_blank(const char* ends, uint64_t ends_n, uint64_t n_bytes, bool open_last_line, uint64_t excess)
{
    uint64_t blank = 0, pos = ends_n;
    while (blank < excess && pos > 0) {  // walk back over empty lines
        if (open_last_line && blank == 0) break;  // the last line is not empty
        if (ends[pos - 1] != '\n') break;
        uint64_t q = pos - 1;
        if (q > 0 && ends[q - 1] == '\r') --q;
        if (q == 0 && ends_n < n_bytes) break;     // cannot see the byte in front
        if (q > 0 && ends[q - 1] != '\n') break;  // the line ending here has content
        ++blank;
        pos = q;
    }
    return blank >= excess;
}

inline const char* refusal_message(unsigned int err)
{
    return (err & ERR_FASTQ_HEADER)    ? "FASTQ record does not start with '@' every 4 lines: use bl_reader_*"
           : (err & ERR_FASTQ_PLUS)    ? "FASTQ separator line does not start with '+': use bl_reader_*"
           : (err & ERR_FASTQ_QUAL)    ? "FASTQ quality length differs from the sequence length"
           : (err & ERR_FASTQ_SEQLINE) ? "FASTQ sequence line starts with '>', '@' or '+': use bl_reader_*"
           : (err & ERR_LONE_CR)       ? "a line that is a lone '\\r' stands where it counts as a base: use bl_reader_*"
                                       : "FASTA sequence line starts with '@' or '+': use bl_reader_*";
}

}  // namespace bl_parse
