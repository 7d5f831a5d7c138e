// TEST INFRASTRUCTURE: bl_scan_read_adapters on the host.  The per-lane bodies are the kernel's own (biolib_amd/csrc/bl_adapters_core.hpp
// under BL_CPU_EMU), and so are the order of a read's steps (read_steps) and what a round of the poly walk decides from its ballots
// (poly_join); only the ballots and the shuffle maximum themselves are restated here, as loops over the lanes' values.  Every array is a heap array of exactly its stated size, the wave's staging arrays included, so that AddressSanitizer
// sees any access outside it.
//
//   emu_adapters <bases> <offsets | -> <read_len> <n_seqs> <spans_in | -> <rule: 616 bytes> <packed copy: 0 | 1> <out prefix>
//       writes <out>.records and <out>.spans; prints "invalid: <message>" for a rule that is refused, else seven counts of the bodies
//       that ran (chunks from the packed copy, from ASCII, behind the read; reversed chunks; d(I); adapter keys; poly lanes), then the
//       eleven statistics and the eight per-adapter counts
#define BL_CPU_EMU 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../biolib_amd/csrc/bl_adapters_core.hpp"

using namespace bla;

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

unsigned long long ran[7];
enum { RAN_PACKED = 0, RAN_ASCII, RAN_BEHIND, RAN_REVERSED, RAN_DIFF, RAN_KEY, RAN_POLY };

// the wave's LDS: heap arrays of exactly the kernel's sizes
struct WaveStage {
    uint32_t *codes, *inv, *r1_codes, *r1_inv, *r2_codes, *r2_inv, *rc_codes, *rc_inv;
    WaveStage()
    {
        uint32_t** all[8] = {&codes, &inv, &r1_codes, &r1_inv, &r2_codes, &r2_inv, &rc_codes, &rc_inv};
        for (int k = 0; k < 8; ++k) {
            const size_t n = k < 2 ? STAGE_CHUNKS : PAIR_CHUNKS;
            *all[k] = static_cast<uint32_t*>(std::malloc(n * sizeof(uint32_t)));
            std::memset(*all[k], 0xA5, n * sizeof(uint32_t));
        }
    }
    ~WaveStage()
    {
        uint32_t* all[8] = {codes, inv, r1_codes, r1_inv, r2_codes, r2_inv, rc_codes, rc_inv};
        for (uint32_t* p : all) std::free(p);
    }
};

void count_stage(int how) { ++ran[how == 1 ? RAN_PACKED : (how == 2 ? RAN_ASCII : RAN_BEHIND)]; }

// bl_adapters.hip's ReadPass with the 64 lanes as loops
struct ReadPass {
    const AdapterParams& p;
    WaveStage& s;
    uint64_t first, L, staged;

    ReadPass(const AdapterParams& p_, WaveStage& s_, uint64_t i) : p(p_), s(s_), staged(~0ull) { blsel::read_extent(p.offsets, p.read_len, p.n_bases, i, first, L); }

    void stage(uint64_t block)
    {
        if (block == staged) return;
        for (int lane = 0; lane < 64; ++lane)
            for (int c = lane; c < STAGE_CHUNKS; c += 64) {
                uint32_t code, inv;
                count_stage(stage_chunk(p, first, L, block * BLOCK_CHUNKS + (uint64_t)c, code, inv));
                s.codes[c] = code;
                s.inv[c] = inv;
            }
        staged = block;
    }

    uint64_t poly(uint64_t b, uint64_t e, uint32_t mask)
    {
        const KRule& r = p.rule;
        uint64_t best = e;
        for (uint32_t X = 0; X < 4; ++X) {
            if (!((mask >> X) & 1u)) continue;
            uint64_t carry = 0, n = e - b, left = e;
            for (uint64_t q0 = (e - 1) & ~63ull;; q0 -= 64) {
                stage(q0 / BLOCK);
                uint64_t not_x = 0, is_x = 0, stops = 0;
                uint32_t code[64];
                bool active[64];
                for (int lane = 0; lane < 64; ++lane) {
                    const uint64_t pos = q0 + (uint64_t)lane;
                    active[lane] = pos >= b && pos < e;
                    code[lane] = active[lane] ? base_at(s.codes, s.inv, (uint32_t)(pos % BLOCK)) : 4u;
                    if (active[lane]) ++ran[RAN_POLY];
                    if (active[lane] && code[lane] != X) not_x |= 1ull << lane;
                    if (active[lane] && code[lane] == X) is_x |= 1ull << lane;
                }
                for (int lane = 0; lane < 64; ++lane) {
                    const uint64_t pos = q0 + (uint64_t)lane;
                    if (active[lane] && poly_stops(r, e - pos, poly_count(carry, not_x, lane))) stops |= 1ull << lane;
                }
                if (poly_join(stops, is_x, q0, e, n, left) || q0 <= b) break;
                carry += (uint64_t)__builtin_popcountll(not_x);
            }
            if (n >= r.poly_min_len && left < best) best = left;
        }
        return best;
    }

    uint64_t adapters(uint64_t b, uint64_t e)
    {
        const KRule& r = p.rule;
        uint64_t key = 0;
        if (e <= b) return 0;
        for (uint64_t block = b / BLOCK; block <= (e - 1) / BLOCK; ++block) {
            stage(block);
            const uint64_t lo = b > block * BLOCK ? b : block * BLOCK, hi = e < (block + 1) * BLOCK ? e : (block + 1) * BLOCK;
            for (int lane = 0; lane < 64; ++lane)
                for (uint64_t pos = lo + (uint64_t)lane; pos < hi; pos += 64)
                    for (uint32_t a = 0; a < r.n_adapters; ++a) {
                        const uint32_t O = r.min_overlap < r.adapter_len[a] ? r.min_overlap : r.adapter_len[a];
                        if (pos + O > e) continue;
                        int o, m;
                        const uint64_t k = adapter_key(r, (int)a, s.codes, s.inv, (uint32_t)(pos - block * BLOCK), pos, e, o, m);
                        ++ran[RAN_KEY];
                        key = k > key ? k : key;  // (the wave's maximum)
                    }
        }
        return key;
    }

    void run(uint64_t i, bool paired, uint32_t insert, uint32_t pair_mismatches, bool skipped, unsigned long long* counts)
    {
        bool input_empty;
        Outcome o = read_steps(*this, p, i, L, paired, insert, pair_mismatches, skipped, input_empty);
        uint64_t sb, se;
        finish_read(p.rule, o, input_empty, L, sb, se, counts);
        if (p.out_records) p.out_records[i] = make_record(o);
        if (p.out_spans) {
            p.out_spans[2 * i] = sb;
            p.out_spans[2 * i + 1] = se;
        }
    }
};

void pair_step(const AdapterParams& p, WaveStage& s, uint64_t i, uint32_t& insert, uint32_t& mismatches, bool& skipped)
{
    const KRule& r = p.rule;
    insert = mismatches = 0;
    uint64_t f1, L1, f2, L2;
    blsel::read_extent(p.offsets, p.read_len, p.n_bases, i, f1, L1);
    blsel::read_extent(p.offsets, p.read_len, p.n_bases, i + 1, f2, L2);
    const uint64_t shorter = L1 < L2 ? L1 : L2;
    skipped = shorter > (uint64_t)PAIR_MAX;
    if (skipped || shorter < r.pair_min_overlap) return;
    const int M = (int)shorter, least = (int)r.pair_min_overlap;
    for (int lane = 0; lane < PAIR_CHUNKS; ++lane) {
        uint32_t code, inv;
        count_stage(stage_chunk(p, f1, L1, (uint64_t)lane, code, inv));
        s.r1_codes[lane] = code;
        s.r1_inv[lane] = inv;
        count_stage(stage_chunk(p, f2, L2, (uint64_t)lane, code, inv));
        s.r2_codes[lane] = code;
        s.r2_inv[lane] = inv;
    }
    for (int lane = 0; lane < PAIR_CHUNKS; ++lane) {
        uint32_t code, inv;
        reverse_chunk(s.r2_codes, s.r2_inv, M, lane, code, inv);
        ++ran[RAN_REVERSED];
        s.rc_codes[lane] = code;
        s.rc_inv[lane] = inv;
    }
    for (int top = M; top >= least; top -= 64) {
        for (int lane = 0; lane < 64; ++lane) {  // (the ballot's lowest lane)
            const int I = top - lane;
            if (I < least) continue;
            const uint32_t d = pair_diff(s.r1_codes, s.r1_inv, s.rc_codes, s.rc_inv, M, I, r.pair_max_diff);
            ++ran[RAN_DIFF];
            if (pair_qualifies(r, I, d)) {
                insert = (uint32_t)I;
                mismatches = d;
                return;
            }
        }
    }
}

// bl_kernels.hip's pack_codes_kernel on the host: packed_total chunks of codes and as many bad bits, from the first guard chunk on
void pack_codes(const uint8_t* bases, uint64_t n_bases, uint32_t*& codes, uint32_t*& bad, size_t& total)
{
    total = (size_t)bl::packed_total((int64_t)n_bases);
    codes = static_cast<uint32_t*>(std::calloc(total, sizeof(uint32_t)));
    bad = static_cast<uint32_t*>(std::calloc(total / 32, sizeof(uint32_t)));
    for (size_t t = 0; t < total; ++t) {
        const int64_t c = (int64_t)t - bl::PACK_LEAD;
        bool is_bad = c < 0;
        uint32_t code = 0;
        for (int j = 0; j < 16 && c >= 0; ++j) {
            const uint64_t at = (uint64_t)c * 16 + (uint64_t)j;
            const int x = at < n_bases ? base_code(bases[at]) : -1;
            if (x < 0) is_bad = true;
            else code |= (uint32_t)x << (30 - 2 * j);
        }
        codes[t] = code;
        if (is_bad) bad[t >> 5] |= 1u << (t & 31);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 9) {
        std::fprintf(stderr, "usage: see the head of emu_adapters.cpp\n");
        return 2;
    }
    size_t n_bases, n_off, n_spans, n_rule;
    uint8_t* bases = load<uint8_t>(argv[1], n_bases);
    uint64_t* offsets = load<uint64_t>(argv[2], n_off);
    const uint64_t read_len = std::strtoull(argv[3], nullptr, 10), n_seqs = std::strtoull(argv[4], nullptr, 10);
    uint64_t* spans_in = load<uint64_t>(argv[5], n_spans);
    uint8_t* rule_bytes = load<uint8_t>(argv[6], n_rule);
    const bool packed = std::atoi(argv[7]) != 0;
    const std::string out = argv[8];
    if (n_rule != sizeof(Rule) || (offsets && n_off != n_seqs + 1) || (spans_in && n_spans != 2 * n_seqs)) {
        std::fprintf(stderr, "sizes\n");
        return 2;
    }
    Rule rule;
    std::memcpy(&rule, rule_bytes, sizeof(rule));
    if (const char* what = rule_error(rule, n_seqs)) {
        std::printf("invalid: %s\n", what);
        std::free(bases);
        std::free(offsets);
        std::free(spans_in);
        std::free(rule_bytes);
        return 0;
    }
    AdapterParams p{};
    pack_rule(rule, p.rule);
    p.bases = bases;
    p.n_bases = n_bases;
    p.offsets = offsets;
    p.read_len = offsets ? 0 : (read_len ? read_len : (n_bases ? n_bases : 1));
    p.n_seqs = n_seqs;
    p.spans_in = spans_in;
    uint32_t *codes = nullptr, *bad = nullptr;
    size_t total = 0;
    if (packed) {
        pack_codes(bases, n_bases, codes, bad, total);
        p.codes_packed = codes + bl::PACK_LEAD;
        p.chunk_bad = bad + bl::PACK_LEAD / 32;
    }
    p.out_records = static_cast<Record*>(std::malloc((n_seqs ? n_seqs : 1) * sizeof(Record)));
    p.out_spans = static_cast<uint64_t*>(std::malloc((n_seqs ? n_seqs : 1) * 2 * sizeof(uint64_t)));
    unsigned long long counts[N_COUNTERS] = {};
    {
        WaveStage s;
        const bool paired = (p.rule.flags & FLAG_PAIRED) != 0;
        const uint64_t per = paired ? 2 : 1;
        for (uint64_t u = 0; u < n_seqs / per; ++u) {
            uint32_t insert = 0, mismatches = 0;
            bool skipped = false;
            if (paired) pair_step(p, s, 2 * u, insert, mismatches, skipped);
            for (uint64_t i = per * u; i < per * u + per; ++i) {
                ReadPass pass(p, s, i);
                pass.run(i, paired, insert, mismatches, skipped, counts);
            }
        }
    }
    save(out + ".records", p.out_records, n_seqs * sizeof(Record));
    save(out + ".spans", p.out_spans, n_seqs * 2 * sizeof(uint64_t));
    for (unsigned long long x : ran) std::printf("%llu ", x);
    for (int k = 0; k < N_COUNTERS; ++k) std::printf("%llu ", counts[k]);
    std::printf("\n");
    std::free(p.out_records);
    std::free(p.out_spans);
    std::free(codes);
    std::free(bad);
    std::free(bases);
    std::free(offsets);
    std::free(spans_in);
    std::free(rule_bytes);
    return 0;
}
