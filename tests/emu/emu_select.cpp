// TEST INFRASTRUCTURE: the bodies of bl_batch_select and bl_read_spans (biolib_amd/csrc/bl_select_core.hpp) run on the host under
// AddressSanitizer / UBSan: every stage of bl_select.hip walked as it is written there, the threads as loops, rocPRIM's two exclusive sums
// as plain loops.  Every array is a heap array of EXACTLY its length — the source bases n_bases bytes with nothing behind them, the
// result round_up(total, 16) bytes (the library's buffer has 64 bytes of slack: any store behind the last chunk is a bug here) — so that
// an index outside one of them is a sanitizer report.  Built and run by tests/test_emu_select.py, which compares the files written with
// the model (tests/select_cases.py).
//
//   emu_select select <bases> <offsets | -> <spans> <read_len> <n_bases> <n_seqs> <flags> <out prefix>
//     offsets: n_seqs + 1 u64 words (they may be wrong on purpose); "-": NULL with read_len as the batch's (0: one sequence).  spans: 2 *
//     n_seqs u64 words.  Writes <prefix>.bases, .offsets (the caller's copy), .index and prints "n_out total fixed_len register_waves memory_waves".
//   emu_select spans <records> <stat | -> <offsets | -> <read_len> <n_bases> <n_seqs> <out file> <11 rule numbers in field order>
//     Writes the 2 * n_seqs u64 words of the spans.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../biolib_amd/csrc/bl_select_core.hpp"

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::fprintf(stderr, "emu_select: " __VA_ARGS__); \
            std::fprintf(stderr, "\n");                    \
            std::exit(1);                                  \
        }                                                  \
    } while (0)

using namespace blsel;

template <typename T>
struct Exact {  // a heap array of exactly n elements, filled with 0xC5
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p(static_cast<T*>(std::malloc(n_ ? n_ * sizeof(T) : 1))), n(n_)
    {
        CHECK(p, "out of memory");
        std::memset(p, 0xC5, n_ * sizeof(T));
    }
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

template <typename T>
static Exact<T>* read_file(const char* path, size_t want)
{
    FILE* f = std::fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    Exact<T>* a = new Exact<T>(want);
    CHECK(want == 0 || std::fread(a->p, sizeof(T), want, f) == want, "%s: short file", path);
    CHECK(std::fgetc(f) == EOF, "%s: longer than %zu elements", path, want);
    std::fclose(f);
    return a;
}

template <typename T>
static void write_file(const std::string& path, const T* p, size_t n)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f, "cannot write %s", path.c_str());
    CHECK(n == 0 || std::fwrite(p, sizeof(T), n, f) == n, "%s: short write", path.c_str());
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

static int run_select(char** a)
{
    SelectParams p{};
    const bool null_offsets = std::strcmp(a[1], "-") == 0;
    const uint64_t read_len = std::strtoull(a[3], nullptr, 10);
    p.n_bases = std::strtoull(a[4], nullptr, 10);
    p.n_seqs = std::strtoull(a[5], nullptr, 10);
    p.flags = (uint32_t)std::strtoul(a[6], nullptr, 10);
    const std::string prefix = a[7];
    Exact<uint8_t>* bases = read_file<uint8_t>(a[0], (size_t)p.n_bases);
    Exact<uint64_t>* offsets = null_offsets ? nullptr : read_file<uint64_t>(a[1], (size_t)p.n_seqs + 1);
    Exact<uint64_t>* spans = read_file<uint64_t>(a[2], 2 * (size_t)p.n_seqs);
    CHECK((reinterpret_cast<uintptr_t>(bases->p) & 15) == 0, "the bases are not 16-byte aligned");
    p.bases = bases->p;
    p.offsets = offsets ? offsets->p : nullptr;
    p.read_len = offsets ? 0 : (read_len ? read_len : (p.n_bases ? p.n_bases : 1));  // bl_select.hip: describe_source
    p.spans = spans->p;
    const size_t n1 = (size_t)p.n_seqs + 1;
    Exact<uint64_t> len(n1), keep(n1), start((size_t)p.n_seqs), len_sum(n1), keep_sum(n1), user_offsets(n1), source_index((size_t)p.n_seqs);
    p.len = len.p;
    p.keep = keep.p;
    p.start = start.p;
    p.len_sum = len_sum.p;
    p.keep_sum = keep_sum.p;
    p.user_offsets = user_offsets.p;
    p.source_index = source_index.p;

    for (uint64_t t = 0; t < blocks_for(n1) * TPB; ++t) span_lengths(p, t);
    exclusive_sum(len.p, len_sum.p, n1);
    exclusive_sum(keep.p, keep_sum.p, n1);
    p.total = len_sum.p[p.n_seqs];
    p.n_out = keep_sum.p[p.n_seqs];
    CHECK(p.n_out <= p.n_seqs, "more sequences kept than there are");

    const size_t out_bytes = (size_t)((p.total + 15) / 16 * 16);
    Exact<uint8_t> out(out_bytes);
    Exact<uint64_t> out_offsets((size_t)p.n_out + 1), src_start((size_t)p.n_out);
    p.out = out.p;
    p.out_offsets = out_offsets.p;
    p.src_start = src_start.p;
    for (uint64_t t = 0; t < blocks_for(n1) * TPB; ++t) place_sequence(p, t);
    uint64_t memory_waves = 0, register_waves = 0;  // waves whose chunks look their sequences up in memory / in the lanes' registers
    if (p.total) {
        const uint64_t waves = blocks_for(((p.total + WAVE_BYTES - 1) / WAVE_BYTES) * 64) * (TPB / 64);  // the grid's, the idle ones included
        for (uint64_t wave = 0; wave < waves; ++wave) {
            const uint64_t x_first = wave_first_byte(wave);
            if (x_first >= p.total) continue;
            uint64_t lo = 0, e = p.n_out;
            while (e - lo > 1) {  // the ballot: a prefix of the lanes
                uint64_t below = 0;
                bool open = true;
                for (int lane = 0; lane < 64; ++lane) {
                    const bool pred = kary_probe(p.out_offsets, lo, e, lane, x_first);
                    CHECK(open || !pred, "wave %llu: the probes at or below the byte are no prefix of the lanes", (unsigned long long)wave);
                    open = pred;
                    below += pred ? 1 : 0;
                }
                kary_narrow(lo, e, below);
            }
            CHECK(lo == seq_of(p.out_offsets, x_first, 0, p.n_out - 1), "wave %llu: the 64-ary search differs from the bisection", (unsigned long long)wave);
            const uint64_t x_last = wave_last_byte(p, wave);
            uint64_t o[64], src[64];  // the lanes' registers
            int inside = 0;
            for (int lane = 0; lane < 64; ++lane) {
                o[lane] = lane_offset(p, lo, lane);
                src[lane] = lane_source(p, lo, lane);
                inside += o[lane] <= x_last ? 1 : 0;
            }
            const uint64_t o_lo = p.out_offsets[lo];
            const bool in_registers = inside < 64;
            ++(in_registers ? register_waves : memory_waves);
            const uint64_t hi = in_registers ? lo + (uint64_t)inside : seq_of(p.out_offsets, x_last, lo + 64, p.n_out - 1);
            CHECK(lo <= hi && hi < p.n_out, "wave %llu: bounds %llu %llu", (unsigned long long)wave, (unsigned long long)lo, (unsigned long long)hi);
            for (int u = 0; u < CHUNKS_PER_LANE; ++u)
                for (int lane = 0; lane < 64; ++lane) {
                    const uint64_t x0 = chunk_first_byte(wave, u, lane);
                    const uint64_t x = x0 < p.total ? x0 : p.total - 1;
                    SeqAt s;
                    if (in_registers) {
                        uint32_t cnt = 0;
                        for (uint32_t step = 32; step >= 1; step >>= 1) count_step(cnt, step, o[(cnt + step - 1) & 63], x);  // (a shuffle's index wraps)
                        CHECK(cnt <= (uint32_t)inside, "wave %llu: sequence %u of the wave's %d", (unsigned long long)wave, cnt, inside);
                        s.j = lo + cnt;
                        s.begin = cnt ? o[cnt - 1] : o_lo;
                        s.end = o[cnt & 63];
                        s.src = src[cnt & 63];
                    } else {
                        s = seq_from_memory(p, x, lo, hi);
                    }
                    if (x0 >= p.total) continue;
                    uint32_t w[4];
                    if (chunk_is_one_window(p, s, x0)) {
                        uint32_t v[5];
                        window_load(p.bases, (uint64_t)chunk_vsrc(s, x0), v);
                        window_shift(v, (uint64_t)chunk_vsrc(s, x0), w);
                    } else {
                        gather_pieces(p, x0, s, w);
                    }
                    for (int i = 0; i < 4; ++i)
                        for (int b = 0; b < 4; ++b) out.p[x0 + 4 * i + b] = (uint8_t)(w[i] >> (8 * b));
                }
        }
    }
    for (uint64_t x = p.total; x < out_bytes; ++x) CHECK(out.p[x] == 0, "byte %llu behind the total is not 0", (unsigned long long)x);
    uint64_t fixed_len = p.n_out > 1 && p.total != 0 && p.total % p.n_out == 0 ? p.total / p.n_out : 0;
    if (fixed_len)
        for (uint64_t t = 0; t < blocks_for(p.n_out + 1) * TPB; ++t)
            if (breaks_uniform(p.out_offsets, p.n_out, fixed_len, t)) {
                fixed_len = 0;
                break;
            }
    for (uint64_t j = 0; j <= p.n_out; ++j) CHECK(out_offsets.p[j] == user_offsets.p[j], "the caller's offsets differ from the library's at %llu", (unsigned long long)j);
    write_file(prefix + ".bases", out.p, (size_t)p.total);
    write_file(prefix + ".offsets", user_offsets.p, (size_t)p.n_out + 1);
    write_file(prefix + ".index", source_index.p, (size_t)p.n_out);
    std::printf("%llu %llu %llu %llu %llu\n", (unsigned long long)p.n_out, (unsigned long long)p.total, (unsigned long long)fixed_len,
                (unsigned long long)register_waves, (unsigned long long)memory_waves);
    delete bases;
    delete offsets;
    delete spans;
    return 0;
}

static int run_spans(char** a)
{
    SpanParams p{};
    const bool null_stat = std::strcmp(a[1], "-") == 0, null_offsets = std::strcmp(a[2], "-") == 0;
    const uint64_t read_len = std::strtoull(a[3], nullptr, 10);
    p.n_bases = std::strtoull(a[4], nullptr, 10);
    p.n_seqs = std::strtoull(a[5], nullptr, 10);
    uint64_t w[11];
    for (int i = 0; i < 11; ++i) w[i] = std::strtoull(a[7 + i], nullptr, 10);
    p.rule = SpanRule{(uint32_t)w[0], (uint32_t)w[1], w[2], (uint32_t)w[3], (uint32_t)w[4], (uint32_t)w[5], (uint32_t)w[6], (uint32_t)w[7], (uint32_t)w[8],
                      (uint32_t)w[9], (uint32_t)w[10]};
    if (!rule_valid(p.rule)) {
        std::printf("invalid\n");
        return 0;
    }
    Exact<Record>* records = read_file<Record>(a[0], (size_t)p.n_seqs);
    Exact<uint32_t>* stat = null_stat ? nullptr : read_file<uint32_t>(a[1], (size_t)p.n_seqs);
    Exact<uint64_t>* offsets = null_offsets ? nullptr : read_file<uint64_t>(a[2], (size_t)p.n_seqs + 1);
    p.offsets = offsets ? offsets->p : nullptr;
    p.read_len = offsets ? 0 : (read_len ? read_len : (p.n_bases ? p.n_bases : 1));
    p.records = records->p;
    p.stat = stat ? stat->p : nullptr;
    Exact<uint64_t> spans(2 * (size_t)p.n_seqs);
    p.spans = spans.p;
    for (uint64_t t = 0; t < blocks_for(p.n_seqs) * TPB; ++t) read_span(p, t);
    write_file(a[6], spans.p, spans.n);
    std::printf("ok\n");
    delete records;
    delete stat;
    delete offsets;
    return 0;
}

int main(int argc, char** argv)
{
    CHECK(argc >= 2, "usage: see the head of the source");
    if (std::strcmp(argv[1], "select") == 0 && argc == 10) return run_select(argv + 2);
    if (std::strcmp(argv[1], "spans") == 0 && argc == 20) return run_spans(argv + 2);
    CHECK(false, "usage: see the head of the source");
    return 1;
}
