// TEST INFRASTRUCTURE: the bodies of bl_select_read_counts (biolib_amd/csrc/bl_read_quantiles_core.hpp) run on the host under
// AddressSanitizer / UBSan: the lanes as loops, the ballots, shuffles and the workgroup's LDS over plain arrays, the one atomic (the list
// of long sequences) as a plain increment.  Both kernels of bl_read_quantiles.hip are walked as they are written there: the wave kernel
// over a grid of waves that stride over the sequences, then the workgroup kernel over the list it left.  counts, valid, offsets, the
// list and both outputs are heap arrays of EXACTLY their lengths, so that any index outside one of them is a sanitizer report.  Built
// and run by tests/test_emu_read_quantiles.py, which compares what is printed with the model (tests/read_quantiles_cases.py).
//
//   emu_read_quantiles <counts file> <valid file> <offsets file | -> <read_len> <n_bases> <n_seqs> <first> <n> <grid> <n_q> <num> <den> ...
//     counts file: the u32 words of the range [first, first + n) (n = 0: to n_bases), valid file: its bytes.  offsets file: n_seqs + 1
//     u64 words (they may be wrong on purpose); "-": NULL, with read_len as the batch's (0: one sequence).  grid: workgroups of either
//     kernel.  Prints one line "seq <i> <n_kmers> <quantile> ..." per sequence; both outputs start as 0xC5 bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../biolib_amd/csrc/bl_read_quantiles_core.hpp"

#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            std::fprintf(stderr, "emu_read_quantiles: " __VA_ARGS__); \
            std::fprintf(stderr, "\n");                          \
            std::exit(1);                                        \
        }                                                        \
    } while (0)

using namespace blrq;

template <typename T>
struct Exact {  // a heap array of exactly n elements
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p(static_cast<T*>(std::malloc(n_ ? n_ * sizeof(T) : 1))), n(n_) { CHECK(p, "out of memory"); }
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

constexpr int WAVES = WG_TPB / 64;

static void write_answers(const SelectParams& p, uint64_t seq, uint32_t m, const uint32_t* answers)
{
    for (uint32_t j = 0; j < p.n_q; ++j) p.quantiles[seq * p.n_q + j] = answers[j];
    if (p.n_kmers) p.n_kmers[seq] = m;
}

template <int NS>
static void select_in_wave(const SelectParams& p, uint64_t seq, uint64_t r0, uint32_t len)
{
    LaneVals<NS> L[64];
    for (int lane = 0; lane < 64; ++lane) wave_load_lane<NS>(p, r0, len, lane, L[lane]);
    uint32_t m = 0, ors = 0;
    for (int lane = 0; lane < 64; ++lane) {
        m += (uint32_t)__builtin_popcount(L[lane].ok);
        ors |= lane_or<NS>(L[lane]);
    }
    uint32_t answers[MAX_Q] = {0, 0, 0, 0};
    if (ors) {
        const int hb = highest_bit(ors);
        for (uint32_t j = 0; j < p.n_q; ++j) {
            uint64_t k = rank_of(m, p.q_num[j], p.q_den[j]);
            uint32_t prefix = 0;
            for (int bit = hb; bit >= 0; --bit) {
                uint32_t zeros = 0;
                for (int s = 0; s < NS; ++s)
                    for (int lane = 0; lane < 64; ++lane) zeros += slot_in_zero_half<NS>(L[lane], s, prefix, bit) ? 1u : 0u;
                narrow_bit(k, prefix, bit, zeros);
            }
            answers[j] = prefix;
        }
    }
    write_answers(p, seq, m, answers);
}

static void wave_kernel(const SelectParams& p, uint64_t grid)
{
    for (uint64_t wave = 0; wave < grid * WAVES; ++wave) {
        const uint64_t lo = work_bound(p, 0), hi = work_bound(p, 1);
        for (uint64_t seq = lo + wave; seq < hi; seq += grid * WAVES) {
            uint64_t r0, len;
            if (!sequence_span(p, seq, r0, len)) continue;
            if (len > (uint64_t)WAVE_MAX) {
                const unsigned long long slot = (*p.long_count)++;
                if (slot < p.long_cap) p.long_list[slot] = seq;
            } else if (len <= 64u * WAVE_SLOTS_SHORT) {
                select_in_wave<WAVE_SLOTS_SHORT>(p, seq, r0, (uint32_t)len);
            } else {
                select_in_wave<WAVE_SLOTS>(p, seq, r0, (uint32_t)len);
            }
        }
    }
}

static void wg_kernel(const SelectParams& p, uint64_t grid)
{
    const unsigned long long listed = *p.long_count;
    const uint64_t n_long = listed < p.long_cap ? listed : p.long_cap;
    for (uint64_t block = 0; block < grid; ++block) {
        for (uint64_t t = block; t < n_long; t += grid) {
            const uint64_t seq = p.long_list[t];
            uint64_t r0, len;
            if (seq >= p.n_seqs || !sequence_span(p, seq, r0, len)) continue;
            const uint64_t n_steps = wg_steps(len);
            uint32_t m = 0, ors = 0;
            for (int tid = 0; tid < WG_TPB; ++tid)
                for (uint64_t step = 0; step < n_steps; ++step)
                    for (int u = 0; u < WG_UNROLL; ++u) {
                        uint64_t j;
                        const bool inside = wg_position(len, step, u, tid, j);
                        wg_census(p, r0, j, inside, m, ors);
                    }
            uint32_t prefix[MAX_Q] = {0, 0, 0, 0};
            uint64_t k[MAX_Q] = {0, 0, 0, 0};
            for (uint32_t q = 0; q < p.n_q; ++q) k[q] = m ? rank_of(m, p.q_num[q], p.q_den[q]) : 0;
            if (ors) {
                for (int shift = top_shift(ors); shift >= 0; shift -= 8) {
                    Exact<uint32_t> hist((size_t)MAX_Q * 256);  // the LDS histograms: exactly their size
                    std::memset(hist.p, 0, sizeof(uint32_t) * MAX_Q * 256);
                    for (int tid = 0; tid < WG_TPB; ++tid)
                        for (uint64_t step = 0; step < n_steps; ++step)
                            for (int u = 0; u < WG_UNROLL; ++u) {
                                uint64_t j;
                                const bool inside = wg_position(len, step, u, tid, j);
                                uint32_t v;
                                bool ok;
                                wg_fetch(p, r0, j, inside, v, ok);
                                for (uint32_t q = 0; q < p.n_q; ++q)
                                    if (ok && digit_candidate(v, prefix[q], shift)) ++hist.p[q * 256 + digit_of(v, shift)];
                            }
                    for (uint32_t q = 0; q < p.n_q; ++q) {  // wave q
                        uint64_t below = 0;
                        int takers = 0;
                        uint64_t k_new = k[q];
                        uint32_t prefix_new = prefix[q];
                        for (int lane = 0; lane < 64; ++lane) {
                            uint32_t h[4];
                            for (int d = 0; d < 4; ++d) h[d] = hist.p[q * 256 + 4 * lane + d];
                            uint64_t kk = k[q];
                            uint32_t pp = prefix[q];
                            if (narrow_digit(h, below, lane, shift, kk, pp)) {
                                ++takers;
                                k_new = kk;
                                prefix_new = pp;
                            }
                            below += (uint64_t)h[0] + h[1] + h[2] + h[3];
                        }
                        CHECK(takers == 1, "sequence %llu: %d lanes hold the rank", (unsigned long long)seq, takers);
                        k[q] = k_new;
                        prefix[q] = prefix_new;
                    }
                }
            }
            write_answers(p, seq, m, prefix);
        }
    }
}

int main(int argc, char** argv)
{
    CHECK(argc >= 13, "usage: see the head of the source");
    SelectParams p{};
    const bool null_offsets = std::strcmp(argv[3], "-") == 0;
    const uint64_t read_len = std::strtoull(argv[4], nullptr, 10);
    p.n_bases = std::strtoull(argv[5], nullptr, 10);
    p.n_seqs = std::strtoull(argv[6], nullptr, 10);
    p.first = std::strtoull(argv[7], nullptr, 10);
    const uint64_t n = std::strtoull(argv[8], nullptr, 10);
    const uint64_t grid = std::strtoull(argv[9], nullptr, 10);
    p.n_q = (uint32_t)std::strtoul(argv[10], nullptr, 10);
    CHECK(p.n_q >= 1 && p.n_q <= (uint32_t)MAX_Q && argc == 11 + 2 * (int)p.n_q && grid >= 1 && p.n_seqs >= 1, "bad arguments");
    for (uint32_t j = 0; j < p.n_q; ++j) {
        p.q_num[j] = (uint32_t)std::strtoul(argv[11 + 2 * j], nullptr, 10);
        p.q_den[j] = (uint32_t)std::strtoul(argv[12 + 2 * j], nullptr, 10);
        CHECK(p.q_den[j] >= 1 && p.q_num[j] <= p.q_den[j], "bad quantile");
    }
    CHECK(p.first <= p.n_bases, "range starts beyond the batch");
    p.end = (n == 0 || n > p.n_bases - p.first) ? p.n_bases : p.first + n;
    CHECK(p.end > p.first && p.end - p.first <= (1ull << 31), "empty or too long a range");
    const size_t span = (size_t)(p.end - p.first);
    Exact<uint32_t>* counts = read_file<uint32_t>(argv[1], span);
    Exact<uint8_t>* valid = read_file<uint8_t>(argv[2], span);
    Exact<uint64_t>* offsets = null_offsets ? nullptr : read_file<uint64_t>(argv[3], (size_t)p.n_seqs + 1);
    p.counts = counts->p;
    p.valid = valid->p;
    p.offsets = offsets ? offsets->p : nullptr;
    p.read_len = offsets ? 0 : (read_len ? read_len : p.n_bases);
    Exact<uint32_t> quantiles((size_t)p.n_seqs * p.n_q), n_kmers((size_t)p.n_seqs);
    std::memset(quantiles.p, 0xC5, sizeof(uint32_t) * quantiles.n);
    std::memset(n_kmers.p, 0xC5, sizeof(uint32_t) * n_kmers.n);
    p.quantiles = quantiles.p;
    p.n_kmers = n_kmers.p;
    const uint64_t by_length = (p.end - p.first) / ((uint64_t)WAVE_MAX + 1);
    p.long_cap = by_length < p.n_seqs ? by_length : p.n_seqs;
    Exact<uint64_t> list((size_t)p.long_cap);
    unsigned long long long_count = 0;
    p.long_list = list.p;
    p.long_count = &long_count;

    wave_kernel(p, grid);
    if (p.long_cap) wg_kernel(p, grid);

    for (uint64_t i = 0; i < p.n_seqs; ++i) {
        std::printf("seq %llu %u", (unsigned long long)i, n_kmers.p[i]);
        for (uint32_t j = 0; j < p.n_q; ++j) std::printf(" %u", quantiles.p[i * p.n_q + j]);
        std::printf("\n");
    }
    delete counts;
    delete valid;
    delete offsets;
    return 0;
}
