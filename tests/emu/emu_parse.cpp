// emu_parse.cpp — TEST INFRASTRUCTURE: the device-side FASTA / FASTQ parser (biolib_amd/csrc/bl_parse.hip) on the host, under the sanitizers.
//
// The per-thread bodies of the seven kernels and the host's decisions on the text's ends live in bl_parse_core.hpp; this program runs them
// thread by thread in the kernels' launch shapes (blocks of 256 threads, waves of 64 lanes, every launched thread run, the ones behind the
// data included), with plain host prefix sums where the library calls rocPRIM, in the order bl_parse_device_text runs them.  The text is
// allocated as exactly n + 64 bytes and the bases as exactly total + 64 bytes on the heap, as the library does, and the offsets as exactly
// n_records + 1 entries, so that any access beyond what the library guarantees is reported.  The per-line arrays come from a scratch that
// only grows and is never cleared, as the library's does: a result must not depend on the text parsed before.
//
//   emu_parse FILE     FILE: per case  u32 name length, name, u64 text length, text  (written by tests/test_parse_cases.py)
// prints per case one line:  name TAB "refused: " message   or   name TAB n_seqs TAB fixed_len TAB lengths (comma separated) TAB bases in hex
#define BL_CPU_EMU
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../biolib_amd/csrc/bl_parse_core.hpp"

using namespace bl_parse;
typedef unsigned long long u64;

namespace {

// grow-only scratch slot, garbage where it was never written
struct Slot {
    unsigned char* p = nullptr;
    size_t cap = 0;
    unsigned char* get(size_t bytes)
    {
        if (bytes > cap) {
            std::free(p);
            p = static_cast<unsigned char*>(std::malloc(bytes));
            std::memset(p, 0xcd, bytes);
            cap = bytes;
        }
        return p;
    }
    ~Slot() { std::free(p); }
};
Slot slot0, slot1;

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Parsed {
    bool refused = false;
    std::string message;
    std::vector<u64> offsets;
    std::vector<uint8_t> bases;
    u64 fixed_len = 0;
};

Parsed refuse(const char* msg)
{
    Parsed r;
    r.refused = true;
    r.message = msg;
    return r;
}

// bl_batch_from_text + bl_parse_device_text
Parsed parse(const std::string& input)
{
    Parsed out;
    u64 n_bytes = input.size();
    if (n_bytes == 0) {
        out.offsets.push_back(0);
        return out;
    }
    uint8_t* text = static_cast<uint8_t*>(std::malloc(n_bytes + 64));  // bl_ctx_scratch(ctx, 3, n_bytes + 64): the slack is never read
    std::memcpy(text, input.data(), n_bytes);
    struct Free {
        void* p;
        ~Free() { std::free(p); }
    } free_text{text};
    u64 ends_n = n_bytes < 64 ? n_bytes : 64;
    std::vector<char> ends_copy(input.end() - ends_n, input.end());  // its own allocation: the walk must stay inside it
    const char* ends = ends_copy.data();
    const char first_byte = input[0];

    const bool fastq = first_byte == '@';
    if (!fastq && first_byte != '>') return refuse("text starts with neither '>' nor '@': use bl_reader_* for irregular files");
    if (drops_trailing_marker(fastq, ends, ends_n, n_bytes)) {
        --n_bytes;
        --ends_n;
        if (n_bytes == 0) {
            out.offsets.push_back(0);
            return out;
        }
    }
    const bool open_last_line = ends[ends_n - 1] != '\n';
    const u64 n = n_bytes;
    const unsigned n_blocks = (unsigned)((n + BYTES_PER_BLOCK - 1) / BYTES_PER_BLOCK);
    const size_t blk_bytes = up256(2 * ((size_t)n_blocks + 1) * sizeof(u64));
    unsigned char* a0 = slot0.get(blk_bytes + 256);
    u64* d_blk = reinterpret_cast<u64*>(a0);
    unsigned int* d_err = reinterpret_cast<unsigned int*>(a0 + blk_bytes);
    u64* d_blk_base = d_blk + n_blocks + 1;
    d_blk[n_blocks] = 0;
    d_err[0] = 0;
    // count_newlines_kernel
    for (unsigned b = 0; b < n_blocks; ++b) {
        unsigned int sum = 0;
        for (int t = 0; t < PB; ++t) sum += __builtin_popcount(chunk_mask(text, n, chunk_at(b, t)));
        d_blk[b] = sum;
    }
    for (u64 i = 0, run = 0; i <= n_blocks; ++i) {  // exclusive scan over n_blocks + 1 items
        const u64 v = d_blk[i];
        d_blk_base[i] = run;
        run += v;
    }
    const u64 n_newlines = d_blk_base[n_blocks];
    const u64 n_lines_raw = n_newlines + (open_last_line ? 1 : 0);
    u64 n_lines = n_lines_raw;
    if (fastq && (n_lines & 3)) {
        const u64 excess = n_lines & 3;
        if (!trailing_lines_blank(ends, ends_n, n_bytes, open_last_line, excess)) return refuse("FASTQ text is not made of 4-line records: use bl_reader_*");
        n_lines -= excess;
        if (n_lines == 0) {
            out.offsets.push_back(0);
            return out;
        }
    }
    const size_t per = up256((n_lines_raw + 2) * sizeof(u64));
    unsigned char* a1 = slot1.get(5 * per);
    u64* d_line_end = reinterpret_cast<u64*>(a1);
    u64* d_len = reinterpret_cast<u64*>(a1 + per);
    u64* d_hdr = reinterpret_cast<u64*>(a1 + 2 * per);
    u64* d_rec = reinterpret_cast<u64*>(a1 + 3 * per);
    u64* d_dst = reinterpret_cast<u64*>(a1 + 4 * per);
    // newline_positions_kernel: per wave an inclusive scan by shuffles (all lanes read, then all lanes write), per block the waves' sums
    for (unsigned b = 0; b < n_blocks; ++b) {
        unsigned int wsum[PB / 64], incl[PB], c[PB];
        uint32_t m[PB];
        for (int t = 0; t < PB; ++t) {
            m[t] = chunk_mask(text, n, chunk_at(b, t));
            incl[t] = c[t] = __builtin_popcount(m[t]);
        }
        for (int wv = 0; wv < PB / 64; ++wv) {
            unsigned int* w = incl + 64 * wv;
            for (int d = 1; d < 64; d <<= 1) {
                unsigned int o[64];
                for (int lane = 0; lane < 64; ++lane) o[lane] = lane >= d ? w[lane - d] : w[lane];  // __shfl_up: own value where there is no lane below
                for (int lane = 0; lane < 64; ++lane) w[lane] = scan_step(w[lane], o[lane], lane, d);
            }
            wsum[wv] = w[63];
        }
        for (int t = 0; t < PB; ++t) {
            unsigned int before = 0;
            for (int i = 0; i < (t >> 6); ++i) before += wsum[i];
            write_newline_positions(m[t], chunk_at(b, t), d_blk_base[b] + before + incl[t] - c[t], d_line_end);
        }
    }
    if (open_last_line) d_line_end[n_newlines] = n;
    d_len[n_lines] = 0;
    const unsigned lb = (unsigned)((n_lines + 255) / 256);
    const u64 line_threads = (u64)lb * LINE_THREADS;
    for (u64 li = 0; li < line_threads; ++li) {  // classify_lines_kernel
        if (li >= n_lines) continue;
        u64 len, h;
        d_err[0] |= classify_line(text, d_line_end, li, fastq ? 1 : 0, len, h);
        d_len[li] = len;
        d_hdr[li] = h;
    }
    for (u64 i = 0, run = 0; i < n_lines; ++i) d_rec[i] = run += d_hdr[i];  // inclusive scan
    if (!fastq)
        for (u64 li = 0; li < line_threads; ++li)
            if (li < n_lines) mask_leading_line(d_rec, d_len, li);
    for (u64 i = 0, run = 0; i <= n_lines; ++i) {  // exclusive scan over n_lines + 1 items
        const u64 v = d_len[i];
        d_dst[i] = run;
        run += v;
    }
    const u64 total = d_dst[n_lines], n_records = d_rec[n_lines - 1];
    unsigned int err = d_err[0];
    if (err & ERR_MASK) return refuse(refusal_message(err));
    const bool lone_cr_seen = (err & NOTE_FASTA_LONE_CR) != 0;

    uint8_t* d_bases = static_cast<uint8_t*>(std::malloc(total + 64));
    u64* d_offsets = static_cast<u64*>(std::malloc((n_records + 1) * sizeof(u64)));
    Free free_bases{d_bases}, free_offsets{d_offsets};
    std::memset(d_bases, 0xcd, total + 64);
    std::memset(d_offsets, 0xcd, (n_records + 1) * sizeof(u64));
    std::memset(d_bases + (total & ~15ull), 0, 64 + (total & 15ull));
    if (total) {
        const u64 threads = (total + 15) / 16, launched = (threads + 255) / 256 * 256;
        for (u64 t = 0; t < launched; ++t)  // gather_bases_kernel
            if (t * 16 < total) gather16(text, d_line_end, d_dst, d_len, n_lines, d_bases, total, t * 16);
    }
    for (u64 li = 0; li < line_threads; ++li) record_offset_line(d_hdr, d_rec, d_dst, n_lines, d_offsets, n_records, total, li);
    if (lone_cr_seen) {
        for (u64 li = 0; li < line_threads; ++li)
            if (li < n_lines && lone_cr_opens_record(text, d_line_end, d_hdr, d_rec, d_dst, d_offsets, li)) d_err[0] |= ERR_LONE_CR;
        err = d_err[0];
    }
    u64 fixed_len = n_records > 1 && total % n_records == 0 ? total / n_records : 0;
    unsigned int ragged = 0;
    if (fixed_len) {
        const u64 launched = (u64)uniform_length_blocks(n_records) * LINE_THREADS;
        for (u64 r = 0; r < launched; ++r)
            if (breaks_uniform_length(d_offsets, n_records, fixed_len, r)) ragged |= 1;
    }
    if (err & ERR_MASK) return refuse(refusal_message(err));
    if (ragged) fixed_len = 0;
    for (u64 i = total; i < total + 64; ++i)
        if (d_bases[i] != 0) return refuse("EMULATION: the slack behind the bases is not zero");
    out.offsets.assign(d_offsets, d_offsets + n_records + 1);
    out.bases.assign(d_bases, d_bases + total);
    out.fixed_len = fixed_len;
    return out;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: emu_parse CASE_FILE\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "emu_parse: cannot open %s\n", argv[1]);
        return 2;
    }
    size_t cases = 0;
    for (;;) {
        uint32_t name_len;
        uint64_t text_len;
        if (std::fread(&name_len, 4, 1, f) != 1) break;
        std::string name(name_len, '\0');
        if (std::fread(&name[0], 1, name_len, f) != name_len || std::fread(&text_len, 8, 1, f) != 1) return 2;
        std::string text(text_len, '\0');
        if (text_len && std::fread(&text[0], 1, text_len, f) != text_len) return 2;
        const Parsed p = parse(text);
        ++cases;
        if (p.refused) {
            std::printf("%s\trefused: %s\n", name.c_str(), p.message.c_str());
            continue;
        }
        std::printf("%s\t%zu\t%llu\t", name.c_str(), p.offsets.size() - 1, (u64)p.fixed_len);
        for (size_t i = 0; i + 1 < p.offsets.size(); ++i) std::printf(i ? ",%llu" : "%llu", p.offsets[i + 1] - p.offsets[i]);
        std::printf("\t");
        for (uint8_t b : p.bases) std::printf("%02x", b);
        std::printf("\n");
    }
    std::fclose(f);
    std::printf("emu_parse: OK %zu cases\n", cases);
    return 0;
}
