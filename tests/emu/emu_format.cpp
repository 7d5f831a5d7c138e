// TEST INFRASTRUCTURE: the bodies of bl_text_index_build and bl_batch_format (biolib_amd/csrc/bl_format_core.hpp) run on the host under
// AddressSanitizer / UBSan: every stage of bl_format.hip walked as it is written there, the threads as loops, rocPRIM's sums as plain
// loops.  Every array is a heap array of EXACTLY its length — the bases n_bases bytes, the text n_text bytes, the records, offsets,
// spans and tags their counts, the output exactly the n_bytes the sizing stage reports — so that an index outside one of them is a
// sanitizer report.  Built and run by tests/test_emu_format.py, which compares the files written with the model (tests/format_cases.py).
//
//   emu_format format <bases> <offsets | -> <text | -> <records | -> <index offsets | -> <source index | -> <spans | -> <tags | ->
//                     <n_bases> <n_seqs> <read_len> <n_text> <n_records> <n_spans> <index_fastq> <format> <flags> <line_width> <fill>
//                     <prefix hex | -> <label hex | -> <first_number> <capacity> <out file>
//     Prints "n_bytes n_records register_waves memory_waves window_chunks piece_chunks", or "capacity n_bytes n_records" where capacity is
//     smaller than n_bytes (nothing is written then: there is no output array at all).
//   emu_format index <text> <n_bytes> <out prefix>
//     The parser's per-line arrays (bl_parse_core.hpp, as emu_parse.cpp walks them) and index_line over them, for a text the parser
//     accepts.  Writes <prefix>.records, <prefix>.offsets and prints "n_records fastq".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../biolib_amd/csrc/bl_format_core.hpp"
#include "../../biolib_amd/csrc/bl_parse_core.hpp"

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            std::fprintf(stderr, "emu_format: " __VA_ARGS__); \
            std::fprintf(stderr, "\n");                       \
            std::exit(1);                                     \
        }                                                     \
    } while (0)

using namespace blfmt;
typedef unsigned long long ull;

template <typename T>
struct Exact {  // a heap array of exactly n elements, filled with 0xC5
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p(static_cast<T*>(std::malloc(n_ ? n_ * sizeof(T) : 1))), n(n_)
    {
        CHECK(p && (reinterpret_cast<uintptr_t>(p) & 15) == 0, "out of memory, or malloc is not 16-byte aligned");
        std::memset(p, 0xC5, n_ * sizeof(T));
    }
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};
struct ExactBytes {
    uint8_t* p;
    size_t n;
    explicit ExactBytes(size_t n_) : p(static_cast<uint8_t*>(std::malloc(n_ ? n_ : 1))), n(n_)
    {
        CHECK(p && (reinterpret_cast<uintptr_t>(p) & 15) == 0, "out of memory, or malloc is not 16-byte aligned");
        std::memset(p, 0xC5, n_);
    }
    ~ExactBytes() { std::free(p); }
    ExactBytes(const ExactBytes&) = delete;
    ExactBytes& operator=(const ExactBytes&) = delete;
};

static void read_into(const char* path, void* p, size_t bytes)
{
    FILE* f = std::fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    CHECK(bytes == 0 || std::fread(p, 1, bytes, f) == bytes, "%s: short file", path);
    CHECK(std::fgetc(f) == EOF, "%s: longer than %zu bytes", path, bytes);
    std::fclose(f);
}
template <typename T>
static Exact<T>* read_words(const char* path, size_t want)
{
    if (std::strcmp(path, "-") == 0) return nullptr;
    Exact<T>* a = new Exact<T>(want);
    read_into(path, a->p, want * sizeof(T));
    return a;
}
static ExactBytes* read_bytes(const char* path, size_t want)
{
    if (std::strcmp(path, "-") == 0) return nullptr;
    ExactBytes* a = new ExactBytes(want);
    read_into(path, a->p, want);
    return a;
}
static void write_file(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f, "cannot write %s", path.c_str());
    CHECK(bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes, "%s: short write", path.c_str());
    std::fclose(f);
}
static void exclusive_sum(const uint64_t* in, uint64_t* out, size_t n)
{
    uint64_t acc = 0;
    for (size_t i = 0; i < n; ++i) {
        out[i] = acc;
        acc += in[i];
    }
}
static uint64_t blocks_for(uint64_t threads) { return (threads + TPB - 1) / TPB; }
static uint32_t unhex(const char* s, uint64_t w[2])
{
    w[0] = w[1] = 0;
    if (std::strcmp(s, "-") == 0) return 0;
    const size_t n = std::strlen(s) / 2;
    CHECK(n <= 15, "more than 15 bytes");
    for (size_t i = 0; i < n; ++i) {
        unsigned v = 0;
        std::sscanf(s + 2 * i, "%2x", &v);
        w[i >> 3] |= (uint64_t)v << (8 * (i & 7));
    }
    return (uint32_t)n;
}

static int run_format(char** a)
{
    FormatParams p{};
    auto num = [&](int i) { return std::strtoull(a[i], nullptr, 10); };
    p.n_bases = num(8);
    p.n_seqs = num(9);
    const uint64_t read_len = num(10);
    p.n_text = num(11);
    p.n_records = num(12);
    const uint64_t n_spans = num(13);
    p.index_fastq = (uint32_t)num(14);
    p.format = (uint32_t)num(15);
    p.flags = (uint32_t)num(16);
    p.line_width = (uint32_t)num(17);
    p.quality_fill = (uint32_t)num(18);
    p.prefix_len = unhex(a[19], p.prefix);
    p.label_len = unhex(a[20], p.label);
    p.first_number = num(21);
    const uint64_t capacity = num(22);
    ExactBytes* bases = read_bytes(a[0], (size_t)p.n_bases);
    Exact<uint64_t>* offsets = read_words<uint64_t>(a[1], (size_t)p.n_seqs + 1);
    ExactBytes* text = read_bytes(a[2], (size_t)p.n_text);
    Exact<TextRecord>* records = read_words<TextRecord>(a[3], (size_t)p.n_records);
    Exact<uint64_t>* ioffsets = read_words<uint64_t>(a[4], (size_t)p.n_records + 1);
    Exact<uint64_t>* source = read_words<uint64_t>(a[5], (size_t)p.n_seqs);
    Exact<uint64_t>* spans = read_words<uint64_t>(a[6], 2 * (size_t)n_spans);
    Exact<uint64_t>* tags = read_words<uint64_t>(a[7], (size_t)p.n_seqs);
    CHECK(bases, "no bases");
    CHECK(!text == !records && !text == !ioffsets, "text, records and index offsets come together");
    CHECK(!spans || n_spans == p.n_records, "one span per record of the index");
    p.bases = bases->p;
    p.offsets = offsets ? offsets->p : nullptr;
    p.read_len = offsets ? 0 : (read_len ? read_len : (p.n_bases ? p.n_bases : 1));  // bl_format.hip
    p.full_reads = p.read_len ? p.n_bases / p.read_len : 0;
    if (text && p.n_records) {                                                       // bl_format.hip: an index without records is none
        p.text = text->p;
        p.records = records->p;
        p.index_offsets = ioffsets->p;
    } else {
        p.n_text = p.n_records = 0;
        p.index_fastq = 0;
    }
    p.source_index = source ? source->p : nullptr;
    p.spans = spans ? spans->p : nullptr;
    p.tags = tags ? tags->p : nullptr;

    const size_t n1 = (size_t)p.n_seqs + 1;
    Exact<uint64_t> rec_len(n1), written(n1), rec_off(n1), written_sum(n1);
    Exact<Desc> desc((size_t)p.n_seqs);
    p.desc = desc.p;
    p.rec_len = rec_len.p;
    p.written = written.p;
    p.rec_off = rec_off.p;
    for (uint64_t t = 0; t < blocks_for(n1) * TPB; ++t) record_length(p, t);
    exclusive_sum(rec_len.p, rec_off.p, n1);
    exclusive_sum(written.p, written_sum.p, n1);
    p.total = rec_off.p[p.n_seqs];
    const uint64_t n_written = written_sum.p[p.n_seqs];
    auto release = [&] {
        delete bases;
        delete offsets;
        delete text;
        delete records;
        delete ioffsets;
        delete source;
        delete spans;
        delete tags;
    };
    if (capacity < p.total) {
        std::printf("capacity %llu %llu\n", (ull)p.total, (ull)n_written);
        release();
        return 0;
    }
    ExactBytes out((size_t)p.total);
    p.out = out.p;
    uint64_t memory_waves = 0, register_waves = 0, window_chunks = 0, piece_chunks = 0;
    if (p.total) {
        const uint64_t waves = blocks_for(((p.total + WAVE_BYTES - 1) / WAVE_BYTES) * 64) * (TPB / 64);  // the grid's, the idle ones included
        for (uint64_t wave = 0; wave < waves; ++wave) {
            const uint64_t x_first = blsel::wave_first_byte(wave);
            if (x_first >= p.total) continue;
            uint64_t lo = 0, e = p.n_seqs;
            while (e - lo > 1) {  // the ballot: a prefix of the lanes
                uint64_t below = 0;
                bool open = true;
                for (int lane = 0; lane < 64; ++lane) {
                    const bool pred = blsel::kary_probe(p.rec_off, lo, e, lane, x_first);
                    CHECK(open || !pred, "wave %llu: the probes at or below the byte are no prefix of the lanes", (ull)wave);
                    open = pred;
                    below += pred ? 1 : 0;
                }
                blsel::kary_narrow(lo, e, below);
            }
            CHECK(lo == blsel::seq_of(p.rec_off, x_first, 0, p.n_seqs - 1), "wave %llu: the 64-ary search differs from the bisection", (ull)wave);
            const uint64_t x_last = wave_last_byte(p, wave);
            uint64_t o[64];  // the lanes' registers
            int inside = 0;
            for (int lane = 0; lane < 64; ++lane) {
                o[lane] = lane_offset(p, lo, lane);
                inside += o[lane] <= x_last ? 1 : 0;
            }
            const uint64_t o_lo = p.rec_off[lo];
            const bool in_registers = inside < 64;
            ++(in_registers ? register_waves : memory_waves);
            const uint64_t hi = in_registers ? lo + (uint64_t)inside : blsel::seq_of(p.rec_off, x_last, lo + 64, p.n_seqs - 1);
            CHECK(lo <= hi && hi < p.n_seqs, "wave %llu: bounds %llu %llu", (ull)wave, (ull)lo, (ull)hi);
            for (int u = 0; u < CHUNKS_PER_LANE; ++u)
                for (int lane = 0; lane < 64; ++lane) {
                    const uint64_t x0 = blsel::chunk_first_byte(wave, u, lane);
                    const uint64_t x = x0 < p.total ? x0 : p.total - 1;
                    RecAt s;
                    if (in_registers) {
                        uint32_t cnt = 0;
                        for (uint32_t step = 32; step >= 1; step >>= 1) blsel::count_step(cnt, step, o[(cnt + step - 1) & 63], x);  // (a shuffle's index wraps)
                        CHECK(cnt <= (uint32_t)inside, "wave %llu: record %u of the wave's %d", (ull)wave, cnt, inside);
                        s.j = lo + cnt;
                        s.begin = cnt ? o[cnt - 1] : o_lo;
                        s.end = o[cnt & 63];
                    } else {
                        s = rec_from_memory(p, x, lo, hi);
                    }
                    if (x0 >= p.total) continue;
                    CHECK(s.begin <= x0 && x0 < s.end && s.end - s.begin == rec_len.p[s.j], "wave %llu: byte %llu is not in record %llu", (ull)wave, (ull)x0, (ull)s.j);
                    uint32_t w[4];
                    const Rec d = load_rec(p, s.j);
                    const uint8_t* src;
                    uint64_t vsrc;
                    if (x0 + CHUNK <= s.end && chunk_window(p, d, x0 - s.begin, src, vsrc)) {
                        uint32_t v[5];
                        blsel::window_load(src, vsrc, v);
                        blsel::window_shift(v, vsrc, w);
                        ++window_chunks;
                    } else {
                        format_pieces(p, x0, s, w);
                        ++piece_chunks;
                    }
                    store_chunk(p.out, p.total, x0, w);
                }
        }
    }
    // the definition, byte by byte: record_byte of every record
    for (uint64_t i = 0; i < p.n_seqs; ++i) {
        if (!rec_len.p[i]) continue;
        const Rec d = describe(p, i);
        for (uint64_t r = 0; r < d.total; ++r)
            CHECK(out.p[rec_off.p[i] + r] == (uint8_t)record_byte(p, d, r), "sequence %llu: byte %llu of its record differs from record_byte", (ull)i, (ull)r);
    }
    write_file(a[23], out.p, (size_t)p.total);
    std::printf("%llu %llu %llu %llu %llu %llu\n", (ull)p.total, (ull)n_written, (ull)register_waves, (ull)memory_waves, (ull)window_chunks, (ull)piece_chunks);
    release();
    return 0;
}

static int run_index(char** a)
{
    using namespace bl_parse;
    uint64_t n = std::strtoull(a[1], nullptr, 10);
    CHECK(n > 0, "an empty text has no lines");
    ExactBytes* text = read_bytes(a[0], (size_t)n);
    const std::string prefix = a[2];
    const bool fastq = text->p[0] == '@';
    const uint64_t ends_n = n < 64 ? n : 64;
    const char* ends = reinterpret_cast<const char*>(text->p) + (n - ends_n);
    if (drops_trailing_marker(fastq, ends, ends_n, n)) --n;
    CHECK(n > 0, "a text of one marker");
    const bool open_last_line = text->p[n - 1] != '\n';
    std::vector<ull> found;
    for (uint64_t at = 0; at < (n + 15) / 16 * 16; at += 16) {
        ull tmp[16];
        const uint32_t m = chunk_mask(text->p, n, at);
        write_newline_positions(m, at, 0, tmp);
        for (int i = 0; i < __builtin_popcount(m); ++i) found.push_back(tmp[i]);
    }
    if (open_last_line) found.push_back(n);
    uint64_t n_lines = found.size();
    if (fastq) n_lines -= n_lines & 3;  // (the test hands over accepted texts: the excess lines are blank)
    Exact<ull> line_end(found.size()), len(n_lines + 1), hdr(n_lines), rec(n_lines), dst(n_lines + 1);
    std::memcpy(line_end.p, found.data(), found.size() * sizeof(ull));
    len.p[n_lines] = 0;
    unsigned int err = 0;
    for (uint64_t li = 0; li < n_lines; ++li) err |= classify_line(text->p, line_end.p, li, fastq ? 1 : 0, len.p[li], hdr.p[li]);
    CHECK(!(err & ERR_MASK), "the parser refuses this text");
    ull acc = 0;
    for (uint64_t li = 0; li < n_lines; ++li) rec.p[li] = acc += hdr.p[li];
    if (!fastq)
        for (uint64_t li = 0; li < n_lines; ++li) mask_leading_line(rec.p, len.p, li);
    acc = 0;
    for (uint64_t li = 0; li <= n_lines; ++li) {
        dst.p[li] = acc;
        acc += len.p[li];
    }
    const uint64_t total = dst.p[n_lines], n_records = n_lines ? rec.p[n_lines - 1] : 0;
    Exact<TextRecord> records((size_t)n_records);
    Exact<uint64_t> offsets((size_t)n_records + 1);
    uint32_t index_err = 0;
    for (uint64_t t = 0; t < blocks_for(n_lines) * TPB; ++t)
        index_err |= index_line(text->p, line_end.p, hdr.p, rec.p, dst.p, n_lines, fastq ? 1 : 0, n_records, total, records.p, offsets.p, t);
    CHECK(!index_err, "a record does not fit 32 bits");
    write_file(prefix + ".records", records.p, records.n * sizeof(TextRecord));
    write_file(prefix + ".offsets", offsets.p, offsets.n * sizeof(uint64_t));
    std::printf("%llu %d\n", (ull)n_records, fastq ? 1 : 0);
    delete text;
    return 0;
}

int main(int argc, char** argv)
{
    CHECK(argc >= 2, "usage: see the head of the source");
    if (std::strcmp(argv[1], "format") == 0 && argc == 26) return run_format(argv + 2);
    if (std::strcmp(argv[1], "index") == 0 && argc == 5) return run_index(argv + 2);
    CHECK(false, "usage: see the head of the source");
    return 1;
}
