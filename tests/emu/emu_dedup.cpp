// TEST INFRASTRUCTURE: bl_scan_read_duplicates on the host.  The per-lane bodies are the kernels' own (biolib_amd/csrc/bl_dedup_core.hpp
// under BL_CPU_EMU): the words of a key from the packed copy or from ASCII, their reversal, the hash's parts, the sort key, what a
// place does in a round, the comparison of a unit with its head, the members' entries and the records.  Only the joins over lanes
// (the sums and the AND of sixteen lanes' values), the two sorts, the segmented scan and the reduction by class are restated here as
// loops, with the operators the kernels hand to them.  Every array is a heap array of exactly its stated size, the packed copy with its
// guard chunks included, so that AddressSanitizer sees any access outside it.
//
//   emu_dedup <bases> <offsets | -> <read_len> <n_seqs> <spans_in | -> <scores | -> <rule: 32 bytes> <packed copy: 0 | 1> <out prefix>
//       writes <out>.records and <out>.spans; prints "invalid: <message>" for a rule that is refused, else the counts of the bodies
//       that ran (bld::RAN_*), then n_empty n_classes n_duplicates n_reversed largest_class n_reads_kept n_bases_kept, the sixteen
//       class_hist entries, n_mixed_groups and rounds
#define BL_CPU_EMU 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../biolib_amd/csrc/bl_dedup_core.hpp"

using namespace bld;

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

template <typename T>
T* array(size_t n)  // exactly n elements, filled with a pattern no body may rely on
{
    void* p = nullptr;
    if (posix_memalign(&p, 16, (n ? n : 1) * sizeof(T)) != 0) std::exit(2);
    std::memset(p, 0xA5, (n ? n : 1) * sizeof(T));
    return static_cast<T*>(p);
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
            const int x = at < n_bases ? bla::base_code(bases[at]) : -1;
            if (x < 0) is_bad = true;
            else code |= (uint32_t)x << (30 - 2 * j);
        }
        codes[t] = code;
        if (is_bad) bad[t >> 5] |= 1u << (t & 31);
    }
}

// dedup_hash_kernel's sum over the SUB lanes of a unit
Hash key_hash(const DedupParams& p, uint64_t start, uint64_t n, bool reversed)
{
    Hash sum;
    sum.lo = sum.hi = 0;
    for (int sub = 0; sub < SUB; ++sub) sum = hash_add(sum, hash_part(p, start, n, reversed, sub));
    return hash_length(p, sum, n);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 10) {
        std::fprintf(stderr, "usage: see the head of emu_dedup.cpp\n");
        return 2;
    }
    size_t n_bases, n_off, n_spans, n_scores, n_rule;
    uint8_t* bases = load<uint8_t>(argv[1], n_bases);
    uint64_t* offsets = load<uint64_t>(argv[2], n_off);
    const uint64_t read_len = std::strtoull(argv[3], nullptr, 10), n_seqs = std::strtoull(argv[4], nullptr, 10);
    uint64_t* spans_in = load<uint64_t>(argv[5], n_spans);
    uint64_t* scores = load<uint64_t>(argv[6], n_scores);
    uint8_t* rule_bytes = load<uint8_t>(argv[7], n_rule);
    const bool packed = std::atoi(argv[8]) != 0;
    const std::string out = argv[9];
    if (n_rule != sizeof(Rule) || (offsets && n_off != n_seqs + 1) || (spans_in && n_spans != 2 * n_seqs) || (scores && n_scores != n_seqs)) {
        std::fprintf(stderr, "sizes\n");
        return 2;
    }
    Rule rule;
    std::memcpy(&rule, rule_bytes, sizeof(rule));
    std::free(rule_bytes);
    if (const char* what = rule_error(rule, n_seqs)) {
        std::printf("invalid: %s\n", what);
        std::free(bases);
        std::free(offsets);
        std::free(spans_in);
        std::free(scores);
        return 0;
    }
    // bl_dedup.hip's entry point
    DedupParams p{};
    p.src.bases = bases;
    p.src.n_bases = n_bases;
    p.src.offsets = offsets;
    p.src.read_len = offsets ? 0 : (read_len ? read_len : (n_bases ? n_bases : 1));
    p.src.n_seqs = n_seqs;
    p.src.spans_in = spans_in;
    uint32_t *codes = nullptr, *bad = nullptr;
    size_t total = 0;
    if (packed) {
        pack_codes(bases, n_bases, codes, bad, total);
        p.src.codes_packed = codes + bl::PACK_LEAD;
        p.src.chunk_bad = bad + bl::PACK_LEAD / 32;
    }
    p.scores = scores;
    p.flags = rule.flags;
    p.hash_bits = rule.hash_bits ? rule.hash_bits : HASH_BITS;
    p.prefix_len = rule.prefix_len;
    p.seed_lo = fmix64(rule.seed + 0x2545f4914f6cdd1dull);
    p.seed_hi = fmix64(rule.seed ^ 0x9fb21c651e98df25ull);
    const uint64_t n = (rule.flags & FLAG_PAIRED) ? n_seqs / 2 : n_seqs;
    p.n_units = n;
    p.out_records = array<Record>(n);
    p.out_spans = array<uint64_t>(2 * n_seqs);
    p.keys = array<Key>(n);
    p.notes = array<uint8_t>(n);
    p.rep = array<uint32_t>(n);
    uint64_t *words_a = array<uint64_t>(n), *words_b = array<uint64_t>(n);
    p.members = array<Best>(n);
    p.member_class = array<uint32_t>(n);
    Best* classes = array<Best>(n);
    p.classes = classes;
    uint32_t flag_words[2] = {0, 0};
    p.flag_words = flag_words;
    unsigned long long counts[N_COUNTERS] = {};
    uint64_t rounds = 0;

    if (n) {
        // 1: hash
        for (uint64_t u = 0; u < n; ++u) {
            const UnitSpan s = unit_span(p, u);
            Hash fwd[2], rev0;
            fwd[1].lo = fwd[1].hi = rev0.lo = rev0.hi = 0;
            for (int t = 0; t < s.reads; ++t) fwd[t] = key_hash(p, s.start[t], s.empty ? 0 : s.n[t], false);
            if ((p.flags & (FLAG_CANONICAL | FLAG_PAIRED)) == FLAG_CANONICAL) rev0 = key_hash(p, s.start[0], s.empty ? 0 : s.n[0], true);
            p.keys[u] = make_key(unit_hash(p, fwd, rev0), p.hash_bits, u, s.empty);
            p.notes[u] = s.empty ? U_EMPTY : 0;
            if (s.empty) p.flag_words[1] = 1u;
        }
        // 2: sort (the keys hold the used bits only)
        std::sort(p.keys, p.keys + n, [](const Key& a, const Key& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); });
        // 3: rounds
        for (;;) {
            p.round = (uint32_t)(++rounds);
            p.flag_words[0] = 0;
            p.scan = words_a;
            for (uint64_t j = 0; j < n; ++j) mark_place(p, j);
            words_b[0] = words_a[0];  // the inclusive scan
            for (uint64_t j = 1; j < n; ++j) words_b[j] = scan_join(words_b[j - 1], words_a[j]);
            p.scan = words_b;
            for (uint64_t j = 0; j < n; ++j) {
                const uint32_t head = place_head(p, j);
                if (head == NONE32) continue;
                uint32_t ok = ~0u;
                if (head != (uint32_t)j) {
                    const UnitSpan a = unit_span(p, key_unit(p.keys[j])), h = unit_span(p, key_unit(p.keys[head]));
                    for (int sub = 0; sub < SUB; ++sub) ok &= compare_unit(p, a, h, sub);
                }
                if (resolve_place(p, j, head, ok)) counts[C_MIXED] += 1;
            }
            if (!p.flag_words[0]) break;
        }
        // 4: finish
        if (rounds > 1 || p.flag_words[1]) {
            for (uint64_t j = 0; j < n; ++j) words_a[j] = order_key(p, j);
            std::sort(words_a, words_a + n);
            p.order = words_a;
        }
        for (uint64_t t = 0; t < n; ++t) member_entry(p, t);
        for (uint64_t t = 0; t < n;) {  // the reduction by class and the scatter to the heads' places
            Best sum = p.members[t];
            uint64_t e = t + 1;
            for (; e < n && p.member_class[e] == p.member_class[t]; ++e) sum = best_join(sum, p.members[e]);
            classes[p.member_class[t]] = sum;
            t = e;
        }
        for (uint64_t j = 0; j < n; ++j) {
            const Tally t = finish_place(p, j);
            counts[C_EMPTY] += t.empty;
            counts[C_CLASSES] += t.head;
            counts[C_DUP] += t.dup;
            counts[C_REV] += t.rev;
            counts[C_READS_KEPT] += t.reads_kept;
            counts[C_BASES_KEPT] += t.bases_kept;
            if (t.copies) counts[C_HIST0 + (t.copies < 16 ? t.copies : 16) - 1] += 1;
            if (t.copies > counts[C_LARGEST]) counts[C_LARGEST] = t.copies;
        }
    }
    save(out + ".records", p.out_records, n * sizeof(Record));
    save(out + ".spans", p.out_spans, n_seqs * 2 * sizeof(uint64_t));
    for (unsigned long long x : ran) std::printf("%llu ", x);
    std::printf("%llu %llu %llu %llu %llu %llu %llu ", counts[C_EMPTY], counts[C_CLASSES], counts[C_DUP], counts[C_REV], counts[C_LARGEST], counts[C_READS_KEPT],
                counts[C_BASES_KEPT]);
    for (int k = 0; k < 16; ++k) std::printf("%llu ", counts[C_HIST0 + k]);
    std::printf("%llu %llu\n", counts[C_MIXED], (unsigned long long)rounds);
    std::free(p.out_records);
    std::free(p.out_spans);
    std::free(p.keys);
    std::free(p.notes);
    std::free(p.rep);
    std::free(words_a);
    std::free(words_b);
    std::free(p.members);
    std::free(p.member_class);
    std::free(classes);
    std::free(codes);
    std::free(bad);
    std::free(bases);
    std::free(offsets);
    std::free(spans_in);
    std::free(scores);
    return 0;
}
