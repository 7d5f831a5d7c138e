// TEST INFRASTRUCTURE: the per-thread bodies of the count-table calls (biolib_amd/csrc/bl_lookup_core.hpp) run on the host, lane by lane,
// under AddressSanitizer / UBSan, against a plain std::lower_bound loop over `unsigned __int128` written here.  The table's arrays, the
// prefix index, the queries and the outputs are heap arrays of EXACTLY their lengths, so that any index outside one is a sanitizer
// report.  Built and run by tests/test_emu_lookup.py, which compares what is printed with Python dicts and its own model.
//
//   emu_lookup table <table file>
//     table file: u64 key_words, key_bits, n, nq, n_opt; i64 option[n_opt] ("table_prefix_bits": -1 automatic, 0 .. 24 forced);
//                 u64 keys[n * key_words] (sorted, distinct), u64 counts[n], u64 queries[nq * key_words]
//     for every option: the index is filled word by word (index_entry), checked against its definition, and the queries are looked up in
//     the lookup kernel's layout (256 lanes, G queries a lane).  Prints "P <option> <P>" and "counts <nq numbers>".
//   emu_lookup scan <batch file> <table file> <k> <canonical> <drop_last> <first> <n> [<first> <n> ...]
//     batch file as emu_kmers128's; the table file's first option is used, its queries are ignored.  For every range the scan thread runs
//     over all tiles; prints "scan <first> <n> count xor_lo xor_hi found sum" and "counts <numbers>", "valid <numbers>".
// Exits non-zero on the first disagreement with the plain loop.
#define EMU_NAME "emu_lookup"
#include <algorithm>

#include "emu128_common.hpp"
#include "../../biolib_amd/csrc/bl_lookup_core.hpp"

template <typename T>
struct Exact {  // a heap array of exactly n elements (16-byte aligned as device memory is); n = 0: a one-byte block nobody may read
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p(nullptr), n(n_)
    {
        void* m = nullptr;
        CHECK(posix_memalign(&m, 16, n_ ? n_ * sizeof(T) : 1) == 0, "out of memory");
        p = static_cast<T*>(m);
    }
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

struct TableFile {
    uint64_t key_words = 0, key_bits = 0, n = 0, nq = 0;
    std::vector<int64_t> options;
    std::vector<uint64_t> keys, counts, queries;

    explicit TableFile(const char* path)
    {
        FILE* f = std::fopen(path, "rb");
        CHECK(f, "cannot open %s", path);
        uint64_t hdr[5];
        CHECK(std::fread(hdr, 8, 5, f) == 5, "short file");
        key_words = hdr[0];
        key_bits = hdr[1];
        n = hdr[2];
        nq = hdr[3];
        CHECK((key_words == 1 || key_words == 2) && key_bits >= 1 && key_bits <= 64 * key_words && hdr[4] >= 1, "bad table header");
        options.resize(hdr[4]);
        keys.resize(n * key_words);
        counts.resize(n);
        queries.resize(nq * key_words);
        CHECK(std::fread(options.data(), 8, options.size(), f) == options.size(), "short file");
        CHECK(keys.empty() || std::fread(keys.data(), 8, keys.size(), f) == keys.size(), "short file");
        CHECK(counts.empty() || std::fread(counts.data(), 8, counts.size(), f) == counts.size(), "short file");
        CHECK(queries.empty() || std::fread(queries.data(), 8, queries.size(), f) == queries.size(), "short file");
        std::fclose(f);
    }
    u128 key(size_t i) const { return key_words == 2 ? ((u128)keys[2 * i + 1] << 64) | keys[2 * i] : (u128)keys[i]; }
    u128 query(size_t i) const { return key_words == 2 ? ((u128)queries[2 * i + 1] << 64) | queries[2 * i] : (u128)queries[i]; }
};

// the table as the library holds it: exact-size arrays, the index filled by the body under test
struct EmuTable {
    Exact<uint64_t> keys;
    Exact<uint32_t> counts;
    Exact<uint32_t> index;
    std::vector<u128> plain;
    bllk::TableView v{};

    EmuTable(const TableFile& f, uint32_t P) : keys(f.keys.size()), counts(f.n), index(((size_t)1 << P) + 1)
    {
        for (size_t i = 0; i < f.keys.size(); ++i) keys.p[i] = f.keys[i];
        for (size_t i = 0; i < f.n; ++i) counts.p[i] = (uint32_t)f.counts[i];
        for (size_t i = 0; i < f.n; ++i) plain.push_back(f.key(i));
        for (size_t i = 1; i < f.n; ++i) CHECK(plain[i - 1] < plain[i], "table keys must be sorted and distinct (slot %zu)", i);
        v.keys = f.n ? keys.p : nullptr;
        v.counts = f.n ? counts.p : nullptr;
        v.index = index.p;
        v.n = (uint32_t)f.n;
        v.key_words = (uint32_t)f.key_words;
        v.key_bits = (uint32_t)f.key_bits;
        v.prefix_bits = P;
        for (uint64_t j = 0; j <= (1ull << P); ++j) index.p[j] = bllk::index_entry(v, (uint32_t)j);
        // the definition: index[j] = the first slot whose key >> (key_bits - P) >= j
        size_t slot = 0;
        for (uint64_t j = 0; j <= (1ull << P); ++j) {
            while (slot < f.n && (uint64_t)(f.key_bits - P >= 128 ? 0 : plain[slot] >> (f.key_bits - P)) < j) ++slot;
            CHECK(index.p[j] == slot, "index[%llu] = %u, want %zu (P = %u)", (unsigned long long)j, index.p[j], slot, P);
        }
    }
    uint32_t want(u128 q) const
    {
        const auto it = std::lower_bound(plain.begin(), plain.end(), q);
        return it != plain.end() && *it == q ? counts.p[it - plain.begin()] : 0u;
    }
};

static int run_table(int argc, char** argv)
{
    CHECK(argc == 3, "usage: emu_lookup table <table file>");
    const TableFile f(argv[2]);
    Exact<uint64_t> q(f.queries.size());
    for (size_t i = 0; i < f.queries.size(); ++i) q.p[i] = f.queries[i];
    for (const int64_t option : f.options) {
        const uint32_t P = bllk::choose_prefix_bits((int)option, f.n, (uint32_t)f.key_bits);
        CHECK(P <= f.key_bits && P <= (uint32_t)bllk::MAX_PREFIX_BITS && (option < 0 || P == std::min<uint64_t>((uint64_t)option, std::min<uint64_t>(f.key_bits, 24))),
              "option %lld gives P = %u", (long long)option, P);
        const EmuTable t(f, P);
        Exact<uint32_t> out(f.nq);
        for (size_t i = 0; i < f.nq; ++i) out.p[i] = 0xdeadbeefu;
        constexpr uint64_t LANES = 256;
        for (uint64_t base = 0; base < f.nq; base += LANES * bllk::G)
            for (uint64_t tid = 0; tid < LANES; ++tid) bllk::lookup_thread(t.v, q.p, f.nq, base + tid, LANES, out.p);
        std::printf("P %lld %u\ncounts", (long long)option, P);
        for (size_t i = 0; i < f.nq; ++i) {
            CHECK(out.p[i] == t.want(f.query(i)), "query %zu: %u, want %u (P = %u)", i, out.p[i], t.want(f.query(i)), P);
            std::printf(" %u", out.p[i]);
        }
        std::printf("\n");
    }
    return 0;
}

struct Plain {
    std::vector<u128> value;
    std::vector<uint8_t> valid;
};

static Plain plain_scan(const std::vector<uint8_t>& seq, const std::vector<uint64_t>& offs, int k, bool canonical, bool drop_last)
{
    const size_t n = seq.size();
    Plain r{std::vector<u128>(n, 0), std::vector<uint8_t>(n, 0)};
    const u128 mask = k == 64 ? ~(u128)0 : (((u128)1 << (2 * k)) - 1);
    for (size_t q = 0; q + 1 < offs.size(); ++q) {
        u128 fwd = 0, rc = 0;
        int run = 0;
        for (uint64_t i = offs[q]; i < offs[q + 1]; ++i) {
            const int c = nt4(seq[i]);
            if (c > 3) { run = 0; continue; }
            fwd = ((fwd << 2) | (u128)c) & mask;
            rc = (rc >> 2) | ((u128)(3 ^ c) << (2 * (k - 1)));
            if (++run < k) continue;
            if (drop_last && i + 1 == offs[q + 1]) continue;
            const uint64_t p = i + 1 - k;
            r.value[p] = canonical && rc < fwd ? rc : fwd;
            r.valid[p] = 1;
        }
    }
    return r;
}

static int run_scan(int argc, char** argv)
{
    CHECK(argc >= 9 && (argc - 7) % 2 == 0, "usage: emu_lookup scan <batch file> <table file> <k> <canonical> <drop_last> <first> <n> [<first> <n> ...]");
    const EmuBatch batch(argv[2]);
    const TableFile f(argv[3]);
    const int k = std::atoi(argv[4]);
    const int canonical = std::atoi(argv[5]), drop_last = std::atoi(argv[6]);
    CHECK(k >= 1 && k <= bl::MAX_UNIT128 && (uint64_t)(2 * k) <= f.key_bits && (f.key_words == 2 || k <= 32), "bad k for this table");
    const EmuTable t(f, bllk::choose_prefix_bits((int)f.options[0], f.n, (uint32_t)f.key_bits));
    const Plain want = plain_scan(batch.seq, batch.offs, k, canonical != 0, drop_last != 0);
    for (int a = 7; a + 1 < argc; a += 2) {
        const uint64_t first = std::strtoull(argv[a], nullptr, 10), n_arg = std::strtoull(argv[a + 1], nullptr, 10);
        const uint64_t end = (n_arg == 0 || first + n_arg > batch.n_bases) ? batch.n_bases : first + n_arg;
        CHECK(first < end, "empty range");
        bllk::ScanCountParams p{};
        batch.describe(p.km);
        bl::plan_kmers128((int64_t)first, (int64_t)end, p.km);
        p.km.unit = k;
        p.km.canonical = canonical;
        p.km.drop_last = drop_last;
        p.table = t.v;
        const size_t span = end - first;
        Exact<uint32_t> counts(span);  // exact-size outputs: a store outside [0, span) is a finding
        Exact<uint8_t> valid(span);
        for (size_t i = 0; i < span; ++i) counts.p[i] = 0xdeadbeefu, valid.p[i] = 0xee;
        std::vector<uint32_t> codes(bl::NCHUNK_POS), flags(bl::NCHUNK_POS);
        bl::Kmer128Acc acc{0, 0, 0, 0, 0}, digest_only{0, 0, 0, 0, 0};
        for (int tile = 0; tile < p.km.n_tiles; ++tile) {
            const int64_t q0 = p.km.origin + (int64_t)tile * bl::H;
            stage_all(p.km, codes, flags, q0);
            for (int tid = 0; tid < bl::TPB; ++tid) {
                p.out_counts = counts.p;
                p.out_valid = valid.p;
                bllk::scan_counts_thread(p, codes.data(), flags.data(), tid, q0, acc);
                p.out_counts = nullptr;
                p.out_valid = nullptr;
                bllk::scan_counts_thread(p, codes.data(), flags.data(), tid, q0, digest_only);  // the path that stores nothing
            }
        }
        unsigned long long w_cnt = 0, w_lo = 0, w_hi = 0, w_found = 0, w_sum = 0;
        for (uint64_t q = first; q < end; ++q) {
            const size_t o = q - first;
            const uint32_t c = want.valid[q] ? t.want(want.value[q]) : 0u;
            CHECK(valid.p[o] == want.valid[q] && counts.p[o] == c, "scan k=%d canonical=%d drop_last=%d position %llu: count %u valid %u, want %u %u", k, canonical,
                  drop_last, (unsigned long long)q, counts.p[o], valid.p[o], c, want.valid[q]);
            if (!want.valid[q]) continue;
            w_cnt += 1;
            w_lo ^= (uint64_t)want.value[q];
            w_hi ^= (uint64_t)(want.value[q] >> 64);
            const auto it = std::lower_bound(t.plain.begin(), t.plain.end(), want.value[q]);
            w_found += it != t.plain.end() && *it == want.value[q];
            w_sum += c;
        }
        CHECK(acc.cnt == w_cnt && acc.xlo == w_lo && acc.xhi == w_hi && acc.xh == w_found && acc.sx == w_sum, "scan digest k=%d first=%llu", k, (unsigned long long)first);
        CHECK(std::memcmp(&acc, &digest_only, sizeof(acc)) == 0, "digest-only path differs k=%d", k);
        std::printf("scan %llu %llu %llu %llu %llu %llu %llu\ncounts", (unsigned long long)first, (unsigned long long)n_arg, acc.cnt, acc.xlo, acc.xhi, acc.xh, acc.sx);
        for (size_t i = 0; i < span; ++i) std::printf(" %u", counts.p[i]);
        std::printf("\nvalid");
        for (size_t i = 0; i < span; ++i) std::printf(" %u", valid.p[i]);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    CHECK(argc >= 2, "usage: emu_lookup table|scan ...");
    if (std::strcmp(argv[1], "table") == 0) return run_table(argc, argv);
    if (std::strcmp(argv[1], "scan") == 0) return run_scan(argc, argv);
    CHECK(false, "unknown mode %s", argv[1]);
    return 2;
}
