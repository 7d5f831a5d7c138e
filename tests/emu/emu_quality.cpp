// TEST INFRASTRUCTURE: bl_scan_read_quality and bl_spans_intersect on the host.  The per-lane bodies are the kernel's own
// (biolib_amd/csrc/bl_quality_core.hpp under BL_CPU_EMU); the groups of bl_quality.hip are restated here with the lanes as loops and the
// ballots, shuffles and scans as loops over the lanes' values.  Every array is a heap array of exactly its stated size, so that
// AddressSanitizer sees any access outside it.
//
//   emu_quality quality <text> <index records> <offsets> <bases> <n_seqs> <fastq> <with records> <out prefix> <17 rule words>
//       writes <out>.records and <out>.spans; prints: short-body fours, wave-body reads, swept reads, then the ten statistics
//   emu_quality intersect <offsets | -> <a> <b | -> <read_len> <n_bases> <n_seqs> <flags> <out>
#define BL_CPU_EMU 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../biolib_amd/csrc/bl_quality_core.hpp"

using namespace blq;

namespace {

// a file as a heap array of exactly its size (16-byte aligned, as the library's buffers are)
template <typename T>
T* load(const char* path, size_t& n)
{
    n = 0;
    if (std::strcmp(path, "-") == 0) return nullptr;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    void* p = nullptr;
    if (posix_memalign(&p, 16, (size_t)bytes) != 0) std::exit(2);  // exactly `bytes`, which need be no multiple of 16
    if (bytes && std::fread(p, 1, (size_t)bytes, f) != (size_t)bytes) std::exit(2);
    std::fclose(f);
    n = (size_t)bytes / sizeof(T);
    return static_cast<T*>(p);
}

void save(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes)) std::exit(2);
    std::fclose(f);
}

// bl_quality.hip's ReadPass with the G lanes as loops
template <int G, bool RESIDENT>
struct ReadPass {
    static constexpr uint64_t CH = (uint64_t)G * LANE;
    const QualityParams& p;
    Place d;
    uint32_t held[G][LANE];

    ReadPass(const QualityParams& p_, uint64_t i, bool live) : p(p_)
    {
        d.first = d.L = d.q_src = d.qn = 0;
        if (live) d = place_read(p, i);  // (the kernel loads it one round ahead)
        if (RESIDENT)
            for (int l = 0; l < G; ++l) fetch_values(p, d, (uint64_t)l * LANE, held[l]);
    }
    uint64_t chunk_of(uint64_t pos) const { return RESIDENT ? 0 : pos / CH; }
    uint64_t lane_pos(uint64_t c, int l) const { return c * CH + (uint64_t)l * LANE; }
    void values(uint64_t c, int l, uint32_t v[LANE]) const
    {
        if (RESIDENT) std::memcpy(v, held[l], sizeof(held[l]));
        else fetch_values(p, d, lane_pos(c, l), v);
    }

    uint64_t first_at_least(uint64_t lo, uint64_t hi, uint32_t threshold) const
    {
        if (hi <= lo) return hi;
        const uint64_t c_last = chunk_of(hi - 1);
        for (uint64_t c = chunk_of(lo);; ++c) {
            for (int l = 0; l < G; ++l) {
                uint32_t v[LANE];
                values(c, l, v);
                const uint32_t m = ge_mask(v, threshold) & range_mask(lane_pos(c, l), lo, hi);
                if (m) return c * CH + (uint64_t)(l * LANE + lowest_bit(m));
            }
            if (c == c_last) return hi;
        }
    }
    uint64_t behind_last_at_least(uint64_t lo, uint64_t hi, uint32_t threshold) const
    {
        if (hi <= lo) return lo;
        const uint64_t c_first = chunk_of(lo);
        for (uint64_t c = chunk_of(hi - 1);; --c) {
            for (int l = G - 1; l >= 0; --l) {
                uint32_t v[LANE];
                values(c, l, v);
                const uint32_t m = ge_mask(v, threshold) & range_mask(lane_pos(c, l), lo, hi);
                if (m) return c * CH + (uint64_t)(l * LANE + highest_bit(m)) + 1;
            }
            if (c == c_first) return lo;
        }
    }
    uint64_t maxsum_back(uint64_t lo, uint64_t hi, uint32_t cutoff) const
    {
        if (hi <= lo) return hi;
        const uint64_t c_first = chunk_of(lo);
        long long carry = 0, best = 0;
        uint64_t best_at = hi;
        for (uint64_t c = chunk_of(hi - 1);; --c) {
            int32_t s[G][LANE], total[G], behind[G];
            uint32_t mask[G], neg[G];
            for (int l = 0; l < G; ++l) {
                uint32_t v[LANE];
                values(c, l, v);
                mask[l] = range_mask(lane_pos(c, l), lo, hi);
                total[l] = sums_behind(v, mask[l], cutoff, s[l]);
            }
            int32_t acc = 0;
            for (int l = G - 1; l >= 0; --l) {
                behind[l] = acc;
                acc += total[l];
            }
            int src = -1;
            for (int l = 0; l < G; ++l) {
                neg[l] = negative_mask(s[l], carry + behind[l], mask[l]);
                if (neg[l]) src = l;
            }
            const int bit = src >= 0 ? highest_bit(neg[src]) : 0;
            long long top = 0;
            int top_lane = -1, top_at = -1;
            for (int l = 0; l < G; ++l) {
                uint32_t candidates = mask[l];
                if (src >= 0) candidates = l > src ? mask[l] : (l == src ? mask[l] & ~((2u << bit) - 1u) : 0u);
                int at;
                const long long mine = best_sum(s[l], carry + behind[l], candidates, true, at);
                if (at >= 0 && mine >= top) top = mine, top_lane = l, top_at = at;  // (the highest lane on a tie)
            }
            if (top > best) {
                best = top;
                best_at = c * CH + (uint64_t)(top_lane * LANE + top_at);
            }
            if (src >= 0 || c == c_first) return best_at;
            carry += acc;
        }
    }
    uint64_t maxsum_front(uint64_t lo, uint64_t hi, uint32_t cutoff) const
    {
        if (hi <= lo) return lo;
        const uint64_t c_last = chunk_of(hi - 1);
        long long carry = 0, best = 0;
        uint64_t best_begin = lo;
        for (uint64_t c = chunk_of(lo);; ++c) {
            int32_t s[G][LANE], total[G], front[G];
            uint32_t mask[G], neg[G];
            int32_t acc = 0;
            for (int l = 0; l < G; ++l) {
                uint32_t v[LANE];
                values(c, l, v);
                mask[l] = range_mask(lane_pos(c, l), lo, hi);
                total[l] = sums_in_front(v, mask[l], cutoff, s[l]);
                front[l] = acc;
                acc += total[l];
            }
            int src = -1;
            for (int l = G - 1; l >= 0; --l) {
                neg[l] = negative_mask(s[l], carry + front[l], mask[l]);
                if (neg[l]) src = l;
            }
            const int bit = src >= 0 ? lowest_bit(neg[src]) : 0;
            long long top = 0;
            int top_lane = -1, top_at = -1;
            for (int l = G - 1; l >= 0; --l) {
                uint32_t candidates = mask[l];
                if (src >= 0) candidates = l < src ? mask[l] : (l == src ? mask[l] & ((1u << bit) - 1u) : 0u);
                int at;
                const long long mine = best_sum(s[l], carry + front[l], candidates, false, at);
                if (at >= 0 && mine >= top) top = mine, top_lane = l, top_at = at;  // (the lowest lane on a tie)
            }
            if (top > best) {
                best = top;
                best_begin = c * CH + (uint64_t)(top_lane * LANE + top_at) + 1;
            }
            if (src >= 0 || c == c_last) return best_begin;
            carry += acc;
        }
    }
    uint64_t window_cut(uint64_t lo, uint64_t hi, uint32_t W, uint32_t window_q) const
    {
        if (hi <= lo || hi - lo < W) return hi;
        int32_t first_sum = 0;
        {
            const uint64_t c_last = chunk_of(lo + W - 1);
            for (uint64_t c = chunk_of(lo);; ++c) {
                for (int l = 0; l < G; ++l) {
                    uint32_t v[LANE];
                    values(c, l, v);
                    first_sum += (int32_t)masked_sum(v, range_mask(lane_pos(c, l), lo, lo + W));
                }
                if (c == c_last) break;
            }
        }
        const int32_t limit = (int32_t)(W * window_q);
        const uint64_t last = hi - W, c_last = chunk_of(last);
        int32_t carry = first_sum;
        for (uint64_t c = chunk_of(lo);; ++c) {
            int32_t acc = 0;
            for (int l = 0; l < G; ++l) {
                uint32_t v[LANE], u[LANE];
                int32_t x[LANE];
                values(c, l, v);
                fetch_values(p, d, lane_pos(c, l) + W, u);
                const int32_t total = window_gains(v, u, range_mask(lane_pos(c, l), lo, last), x);
                const uint32_t fails = below_mask(x, carry + acc, range_mask(lane_pos(c, l), lo, last + 1), limit);
                if (fails) return behind_last_at_least(lo, c * CH + (uint64_t)(l * LANE + lowest_bit(fails)), window_q);
                acc += total;
            }
            if (c == c_last) return hi;
            carry += acc;
        }
    }
    Stats span_stats(uint64_t b, uint64_t e, const uint32_t* err) const
    {
        Stats all = stats_zero();
        const uint32_t need = p.need;
        for (int l = 0; l < G && need; ++l) {
            Stats st = stats_zero();
            if (e > b) {
                const uint64_t c_last = chunk_of(e - 1);
                for (uint64_t c = chunk_of(b);; ++c) {
                    uint32_t v[LANE];
                    values(c, l, v);
                    const uint32_t mask = range_mask(lane_pos(c, l), b, e);
                    stats_add(st, v, mask, p.rule.low_q, need, err);
                    if (need & NEED_AMBIGUOUS) st.n_ambiguous += (uint64_t)__builtin_popcount(ambiguous_mask(p, d, lane_pos(c, l)) & mask);
                    if (c == c_last) break;
                }
            }
            all.sum += st.sum;
            all.ee += st.ee;
            all.n_low += st.n_low;
            all.n_ambiguous += st.n_ambiguous;
            all.q_min = st.q_min < all.q_min ? st.q_min : all.q_min;
            all.q_max = st.q_max > all.q_max ? st.q_max : all.q_max;
        }
        return all;
    }
    void run(uint64_t i, bool live, const uint32_t* err, unsigned long long* counts) const
    {
        const Rule& r = p.rule;
        uint64_t b = 0, e = d.L;
        if (r.front_q) b = first_at_least(b, e, r.front_q);
        if (r.back_q) e = behind_last_at_least(b, e, r.back_q);
        if (r.maxsum_front_q || r.maxsum_back_q) {
            const uint64_t e2 = r.maxsum_back_q ? maxsum_back(b, e, r.maxsum_back_q) : e;
            const uint64_t b2 = r.maxsum_front_q ? maxsum_front(b, e, r.maxsum_front_q) : b;
            b = b2;
            e = e2 > b2 ? e2 : b2;
        }
        if (r.window_len) e = window_cut(b, e, r.window_len, r.window_q);
        const Stats st = span_stats(b, e, err);
        if (!live) return;
        const uint64_t n = e - b;
        const uint32_t failed = failed_bits(r, n, st);
        if (p.out_records) p.out_records[i] = make_record(b, e, st, failed);
        if (p.out_spans) {
            p.out_spans[2 * i] = failed ? 0 : b;
            p.out_spans[2 * i + 1] = failed ? 0 : e;
        }
        const bool kept = failed == 0 && n > 0;
        counts[C_READS] += 1;
        counts[C_KEPT] += kept ? 1 : 0;
        counts[C_BASES_IN] += d.L;
        counts[C_BASES_KEPT] += kept ? n : 0;
        for (int k = 0; k < 6; ++k) counts[C_FAIL0 + k] += (failed >> k) & 1u;
    }
};

int run_quality(char** a)
{
    QualityParams p{};
    size_t n_text, n_rec, n_off, n_bases;
    p.text = load<uint8_t>(a[0], n_text);
    p.records = load<blfmt::TextRecord>(a[1], n_rec);
    p.offsets = load<uint64_t>(a[2], n_off);
    p.bases = load<uint8_t>(a[3], n_bases);
    p.n_text = n_text;
    p.n_bases = n_bases;
    p.n_seqs = std::strtoull(a[4], nullptr, 10);
    p.fastq = (uint32_t)std::atoi(a[5]);
    const bool with_records = std::atoi(a[6]) != 0;  // 0: a call for the spans alone, which takes only the statistics its filters need
    const std::string out = a[7];
    uint64_t w[17];
    for (int i = 0; i < 17; ++i) w[i] = std::strtoull(a[8 + i], nullptr, 10);
    uint32_t* r32 = reinterpret_cast<uint32_t*>(&p.rule);
    for (int i = 0; i < 14; ++i) r32[i] = (uint32_t)w[i];
    p.rule.min_len = w[14], p.rule.max_len = w[15], p.rule.max_ee = w[16];
    auto free_inputs = [&] {
        std::free(const_cast<uint8_t*>(p.text));
        std::free(const_cast<blfmt::TextRecord*>(p.records));
        std::free(const_cast<uint64_t*>(p.offsets));
        std::free(const_cast<uint8_t*>(p.bases));
    };
    if (!rule_valid(p.rule)) {
        std::puts("invalid");
        free_inputs();
        return 0;
    }
    if (n_off != p.n_seqs + 1 || (p.fastq && n_rec != p.n_seqs)) return 2;
    p.need = stats_needed(p.rule, with_records);
    p.out_records = static_cast<Record*>(std::aligned_alloc(16, (p.n_seqs ? p.n_seqs : 1) * sizeof(Record)));
    p.out_spans = static_cast<uint64_t*>(std::malloc(p.n_seqs * 2 * sizeof(uint64_t)));
    std::memset(p.out_records, 0, (p.n_seqs ? p.n_seqs : 1) * sizeof(Record));
    unsigned long long counts[N_COUNTERS] = {}, n_short = 0, n_wave = 0, n_sweep = 0;
    // the kernel's loop: four reads to a wave
    const uint64_t n_fours = (p.n_seqs + READS_PER_WAVE - 1) / READS_PER_WAVE;
    for (uint64_t four = 0; four < n_fours; ++four) {
        uint64_t L[READS_PER_WAVE] = {};
        bool all_short = true;
        for (int k = 0; k < READS_PER_WAVE; ++k) {
            const uint64_t i = four * READS_PER_WAVE + (uint64_t)k;
            uint64_t first;
            if (i < p.n_seqs) blsel::read_extent(p.offsets, 0, p.n_bases, i, first, L[k]);
            all_short = all_short && L[k] <= (uint64_t)SHORT_MAX;
        }
        if (all_short) {
            ++n_short;
            for (int k = 0; k < READS_PER_WAVE; ++k) {
                const uint64_t i = four * READS_PER_WAVE + (uint64_t)k;
                const ReadPass<SHORT_LANES, true> pass(p, i, i < p.n_seqs);
                pass.run(i, i < p.n_seqs, BL_PHRED_ERR, counts);
            }
        } else {
            for (int k = 0; k < READS_PER_WAVE; ++k) {
                const uint64_t i = four * READS_PER_WAVE + (uint64_t)k;
                if (i >= p.n_seqs) break;
                if (L[k] <= (uint64_t)WAVE_MAX) {
                    ++n_wave;
                    const ReadPass<64, true> pass(p, i, true);
                    pass.run(i, true, BL_PHRED_ERR, counts);
                } else {
                    ++n_sweep;
                    const ReadPass<64, false> pass(p, i, true);
                    pass.run(i, true, BL_PHRED_ERR, counts);
                }
            }
        }
    }
    save(out + ".records", p.out_records, p.n_seqs * sizeof(Record));
    save(out + ".spans", p.out_spans, p.n_seqs * 2 * sizeof(uint64_t));
    std::printf("%llu %llu %llu", n_short, n_wave, n_sweep);
    for (int k = 0; k < N_COUNTERS; ++k) std::printf(" %llu", counts[k]);
    std::puts("");
    free_inputs();
    std::free(p.out_records);
    std::free(p.out_spans);
    return 0;
}

int run_intersect(char** a)
{
    IntersectParams p{};
    size_t n_off, n_a, n_b;
    p.offsets = load<uint64_t>(a[0], n_off);
    uint64_t* sa = load<uint64_t>(a[1], n_a);
    uint64_t* sb = load<uint64_t>(a[2], n_b);
    p.read_len = std::strtoull(a[3], nullptr, 10);
    p.n_bases = std::strtoull(a[4], nullptr, 10);
    p.n_seqs = std::strtoull(a[5], nullptr, 10);
    p.flags = (uint32_t)std::strtoul(a[6], nullptr, 10);
    if (n_a != 2 * p.n_seqs || (sb && n_b != 2 * p.n_seqs) || (p.offsets && n_off != p.n_seqs + 1)) return 2;
    p.a = sa;
    p.b = sb;
    p.out = sa;  // in place: the out array may be an input
    for (uint64_t t = 0; t < p.n_seqs + 3; ++t) intersect_spans(p, t);
    save(a[7], p.out, p.n_seqs * 2 * sizeof(uint64_t));
    std::free(const_cast<uint64_t*>(p.offsets));
    std::free(sa);
    std::free(sb);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 27 && std::strcmp(argv[1], "quality") == 0) return run_quality(argv + 2);
    if (argc == 10 && std::strcmp(argv[1], "intersect") == 0) return run_intersect(argv + 2);
    std::fprintf(stderr, "usage: see the head of emu_quality.cpp\n");
    return 2;
}
