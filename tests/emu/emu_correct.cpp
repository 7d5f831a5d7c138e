// TEST INFRASTRUCTURE: the per-thread bodies of bl_scan_read_edits and bl_batch_apply_edits (biolib_amd/csrc/bl_correct_core.hpp) run on the
// host, lane by lane, under AddressSanitizer / UBSan.  The bases, the table's arrays, the states, the candidates and the edits are heap
// arrays of EXACTLY their lengths, so that any index outside one is a sanitizer report.  Built and run by tests/test_emu_correct.py, which
// compares what is printed with its Python model (tests/correct_cases.py).
//
//   emu_correct <batch file> <table file> <k> <canonical> <min_count> <min_support> <capacity|-1> <first> <n> [<first> <n> ...]
//     batch file as emu_kmers128's; table file as emu_lookup's (its first option is the prefix width, its queries are ignored).
//     capacity -1: exactly the number of edits.  For every range prints
//       range <first> <n> <n_runs> <n_edits> <n_ambiguous> <n_no_base> <n_misfit> <n_low_support> <stored>
//       edit <pos> <from> <to> <support> <anchor>     (one line per stored edit)
//     and after the last range "applied <hex bytes of the batch with the LAST range's edits applied>".
#define EMU_NAME "emu_correct"
#include <algorithm>

#include "emu128_common.hpp"
#include "../../biolib_amd/csrc/bl_correct_core.hpp"

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

struct Table {
    uint64_t key_words = 0, key_bits = 0, n = 0;
    int64_t option = -1;
    Exact<uint64_t>* keys = nullptr;
    Exact<uint32_t>* counts = nullptr;
    Exact<uint32_t>* index = nullptr;
    bllk::TableView v{};

    explicit Table(const char* path)
    {
        FILE* f = std::fopen(path, "rb");
        CHECK(f, "cannot open %s", path);
        uint64_t hdr[5];
        CHECK(std::fread(hdr, 8, 5, f) == 5, "short file");
        key_words = hdr[0];
        key_bits = hdr[1];
        n = hdr[2];
        std::vector<int64_t> options(hdr[4]);
        CHECK(!options.empty() && std::fread(options.data(), 8, options.size(), f) == options.size(), "short file");
        option = options[0];
        std::vector<uint64_t> k(n * key_words), c(n);
        CHECK(k.empty() || std::fread(k.data(), 8, k.size(), f) == k.size(), "short file");
        CHECK(c.empty() || std::fread(c.data(), 8, c.size(), f) == c.size(), "short file");
        std::fclose(f);
        const uint32_t P = bllk::choose_prefix_bits((int)option, n, (uint32_t)key_bits);
        keys = new Exact<uint64_t>(k.size());
        counts = new Exact<uint32_t>(n);
        index = new Exact<uint32_t>(((size_t)1 << P) + 1);
        for (size_t i = 0; i < k.size(); ++i) keys->p[i] = k[i];
        for (size_t i = 0; i < n; ++i) counts->p[i] = (uint32_t)c[i];
        v.keys = n ? keys->p : nullptr;
        v.counts = n ? counts->p : nullptr;
        v.index = index->p;
        v.n = (uint32_t)n;
        v.key_words = (uint32_t)key_words;
        v.key_bits = (uint32_t)key_bits;
        v.prefix_bits = P;
        for (uint64_t j = 0; j <= (1ull << P); ++j) index->p[j] = bllk::index_entry(v, (uint32_t)j);
    }
    ~Table()
    {
        delete keys;
        delete counts;
        delete index;
    }
};

int main(int argc, char** argv)
{
    using namespace blcr;
    CHECK(argc >= 10 && (argc - 8) % 2 == 0, "usage: emu_correct <batch> <table> <k> <canonical> <min_count> <min_support> <capacity|-1> <first> <n> [...]");
    const EmuBatch batch(argv[1]);
    const Table table(argv[2]);
    const int k = std::atoi(argv[3]), canonical = std::atoi(argv[4]);
    const uint32_t min_count = (uint32_t)std::atoi(argv[5]), min_support = (uint32_t)std::atoi(argv[6]);
    const long long cap_arg = std::atoll(argv[7]);
    CHECK(k >= 1 && k <= bl::MAX_UNIT128 && (uint64_t)(2 * k) <= table.key_bits && (table.key_words == 2 || k <= 32), "bad k for this table");
    CHECK(min_count >= 1 && min_support >= 1 && min_support <= (uint32_t)k, "bad min_count / min_support");
    const int64_t n_bases = (int64_t)batch.n_bases;
    std::vector<Edit> last;

    for (int arg = 8; arg + 1 < argc; arg += 2) {
        const uint64_t first = std::strtoull(argv[arg], nullptr, 10), n_arg = std::strtoull(argv[arg + 1], nullptr, 10);
        CHECK(first <= batch.n_bases, "range starts beyond the batch");
        const uint64_t end = (n_arg == 0 || n_arg > batch.n_bases - first) ? batch.n_bases : first + n_arg;
        unsigned long long stats[STAT_WORDS] = {};
        std::vector<Edit> stored;
        if (end > first) {
            // ---- pass 1
            const int64_t s0 = first ? (int64_t)first - 1 : 0, s1 = std::min<int64_t>((int64_t)end + k + 1, n_bases);
            Exact<uint8_t> states((size_t)(s1 - s0));
            for (size_t i = 0; i < states.n; ++i) states.p[i] = 0xee;
            StateParams sp{};
            batch.describe(sp.km);
            bl::plan_kmers128(s0, s1, sp.km);
            sp.km.unit = k;
            sp.km.canonical = canonical;
            sp.table = table.v;
            sp.min_count = min_count;
            sp.states = states.p;
            std::vector<uint32_t> codes(bl::NCHUNK_POS), flags(bl::NCHUNK_POS);
            for (int tile = 0; tile < sp.km.n_tiles; ++tile) {
                const int64_t q0 = sp.km.origin + (int64_t)tile * bl::H;
                stage_all(sp.km, codes, flags, q0);
                for (int tid = 0; tid < bl::TPB; ++tid) state_thread(sp, codes.data(), flags.data(), tid, q0);
            }
            for (size_t i = 0; i < states.n; ++i) CHECK(states.p[i] < 8, "state %zu was not written", i);
            // ---- pass 2: the workgroups' counts, their exclusive sum, the candidates
            RunParams rp{states.p, s0, s1, (int64_t)first, (int64_t)end, (uint32_t)k, min_support};
            const uint64_t n_blocks = (end - first + CTPB - 1) / CTPB;
            std::vector<uint64_t> block_base(n_blocks + 1, 0);
            for (uint64_t blk = 0; blk < n_blocks; ++blk) {
                uint64_t cnt = 0;
                for (int tid = 0; tid < CTPB; ++tid) {
                    const int64_t a = (int64_t)first + (int64_t)blk * CTPB + tid;
                    Candidate c{};
                    const int cls = a < (int64_t)end ? run_at(rp, a, c) : RUN_NOT_A_START;
                    stats[STAT_RUNS] += cls != RUN_NOT_A_START;
                    stats[STAT_MISFIT] += cls == RUN_MISFIT;
                    stats[STAT_LOW_SUPPORT] += cls == RUN_LOW_SUPPORT;
                    cnt += cls == RUN_CANDIDATE;
                }
                block_base[blk + 1] = block_base[blk] + cnt;
            }
            const uint64_t n_cand = block_base[n_blocks];
            Exact<Candidate> cand(n_cand);
            for (uint64_t blk = 0; blk < n_blocks; ++blk) {
                uint64_t at = block_base[blk];
                for (int tid = 0; tid < CTPB; ++tid) {
                    const int64_t a = (int64_t)first + (int64_t)blk * CTPB + tid;
                    Candidate c{};
                    if (a < (int64_t)end && run_at(rp, a, c) == RUN_CANDIDATE) cand.p[at++] = c;
                }
                CHECK(at == block_base[blk + 1], "the two run passes disagree");
            }
            // ---- pass 3
            Exact<Edit> edits(n_cand);
            Exact<uint8_t> verdicts(n_cand);
            Exact<uint64_t> flag(n_cand + 1), sum(n_cand + 1);
            TestParams tp{};
            tp.bases = batch.exact;
            tp.n_bases = n_bases;
            tp.table = table.v;
            tp.k = (uint32_t)k;
            tp.min_count = min_count;
            tp.canonical = (uint32_t)canonical;
            tp.cand = cand.p;
            tp.n_cand = n_cand;
            flag.p[n_cand] = 0;
            for (uint64_t i = 0; i < n_cand; ++i) {
                const Candidate c = cand.p[i];
                CHECK(c.len >= 1 && c.len <= (uint32_t)MAX_RUN && c.len <= (uint32_t)k, "candidate length %u", c.len);
                Exact<uint32_t> words(CODE_WORDS_PADDED);
                uint8_t* bytes = reinterpret_cast<uint8_t*>(words.p);
                for (int lane = 0; lane < 64; ++lane) {
                    if (lane < 4 * CODE_WORDS) bytes[code_byte_index(lane)] = (uint8_t)code_byte(tp.bases, n_bases, (int64_t)c.a + 4 * lane);
                    else if (lane < 4 * CODE_WORDS + (CODE_WORDS_PADDED - CODE_WORDS)) words.p[CODE_WORDS + lane - 4 * CODE_WORDS] = 0;
                }
                uint32_t any_fail = 0, orig0 = 0;
                for (int lane = 0; lane < (int)c.len; ++lane) {
                    uint32_t orig = 0;
                    any_fail |= test_lane(tp, words.p, c, lane, orig);
                    if (lane == 0) orig0 = orig;
                    CHECK(orig == orig0, "the lanes of a candidate see different bases at p");
                }
                Edit e{};
                const uint64_t pos = edit_position(c, (uint32_t)k);
                CHECK(pos < (uint64_t)n_bases, "p lies behind the batch");
                const uint32_t v = verdict(~any_fail & 7u, orig0, batch.exact[pos], c, (uint32_t)k, e);
                verdicts.p[i] = (uint8_t)v;
                flag.p[i] = v == V_EDIT;
                if (v == V_EDIT) edits.p[i] = e;
                stats[STAT_EDITS] += v == V_EDIT;
                stats[STAT_AMBIGUOUS] += v == V_AMBIGUOUS;
                stats[STAT_NO_BASE] += v == V_NO_BASE;
            }
            // ---- pass 4
            sum.p[0] = 0;
            for (uint64_t i = 0; i < n_cand; ++i) sum.p[i + 1] = sum.p[i] + flag.p[i];
            const uint64_t capacity = cap_arg < 0 ? stats[STAT_EDITS] : (uint64_t)cap_arg;
            Exact<Edit> out(capacity);
            for (uint64_t i = 0; i < n_cand; ++i) compact_edit(edits.p, verdicts.p, sum.p, i, out.p, capacity);
            const uint64_t n_stored = std::min<uint64_t>(capacity, stats[STAT_EDITS]);
            stored.assign(out.p, out.p + n_stored);
        }
        std::printf("range %llu %llu %llu %llu %llu %llu %llu %llu %zu\n", (unsigned long long)first, (unsigned long long)n_arg, stats[STAT_RUNS], stats[STAT_EDITS],
                    stats[STAT_AMBIGUOUS], stats[STAT_NO_BASE], stats[STAT_MISFIT], stats[STAT_LOW_SUPPORT], stored.size());
        for (const Edit& e : stored) std::printf("edit %llu %u %u %u %u\n", (unsigned long long)e.pos, e.from, e.to, e.support, e.anchor);
        last = stored;
    }
    // ---- pass 5 on an exact-size copy, with two records that must be ignored: a repeated pos and one behind the batch
    if (!last.empty()) {
        Edit dup = last.back();
        dup.to = '#';
        last.push_back(dup);
    }
    Edit beyond{};
    beyond.pos = (uint64_t)n_bases;
    beyond.to = '#';
    last.push_back(beyond);
    Exact<Edit> ed(last.size());
    std::copy(last.begin(), last.end(), ed.p);
    Exact<uint8_t> copy((size_t)n_bases);
    std::memcpy(copy.p, batch.exact, (size_t)n_bases);
    for (uint64_t i = 0; i < last.size() + 3; ++i) edit_at(ed.p, last.size(), i, copy.p, (uint64_t)n_bases);
    std::printf("applied ");
    for (int64_t i = 0; i < n_bases; ++i) std::printf("%02x", copy.p[i]);
    std::printf("\n");
    return 0;
}
