// TEST INFRASTRUCTURE: the bodies of bl_scan_read_counts (biolib_amd/csrc/bl_read_counts_core.hpp) run on the host under AddressSanitizer /
// UBSan: the lanes as loops between the kernel's barriers and shuffles, the wave's shuffles and ballot over arrays of 64 entries, the
// atomics as plain operations.  The records are a heap array of EXACTLY n_seqs entries and the offsets one of EXACTLY n_seqs + 1 words,
// so that any index outside either is a sanitizer report.  Built and run by tests/test_emu_read_counts.py, which compares what is printed
// with the Python model (tests/read_counts_cases.py).
//
//   emu_read_counts <batch file> <table file> <offsets file | -> <read_len> <k> <canonical> <drop_last> <min_count> <first> <n> <mode> [<first> <n> <mode> ...]
//     batch file as emu_kmers128's, table file as emu_lookup's (its first option is used, its queries are ignored).
//     offsets file: n_seqs + 1 u64 words, what the call gets as d_offsets (it may be wrong on purpose); "-": NULL, with read_len as the
//     batch's (0: one sequence).  mode: 0 INIT, 1 ACCUMULATE, 2 no call: every record is set to the identity, as a caller does in front of
//     ACCUMULATE calls alone.  The calls run one after the other on one record array that starts as 0xC5 bytes.  Prints
//     "result <first> <n> count xor_lo xor_hi found sum" per call and at the end one line "record <i> <nine fields>" per record.
#define EMU_NAME "emu_read_counts"
#include "emu128_common.hpp"
#include "../../biolib_amd/csrc/bl_read_counts_core.hpp"

template <typename T>
struct Exact {  // a heap array of exactly n elements, 16-byte aligned as device memory is
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

static std::vector<uint64_t> read_words(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    std::vector<uint64_t> w;
    uint64_t x;
    while (std::fread(&x, 8, 1, f) == 1) w.push_back(x);
    std::fclose(f);
    return w;
}

// the table as the library holds it: exact-size arrays, the index filled by bl_lookup_core.hpp's body (tested by emu_lookup)
struct EmuTable {
    std::vector<uint64_t> file;
    Exact<uint64_t>* keys = nullptr;
    Exact<uint32_t>* counts = nullptr;
    Exact<uint32_t>* index = nullptr;
    bllk::TableView v{};

    explicit EmuTable(const char* path) : file(read_words(path))
    {
        CHECK(file.size() >= 5, "short table file");
        const uint64_t kw = file[0], kb = file[1], n = file[2], n_opt = file[4];
        CHECK((kw == 1 || kw == 2) && kb >= 1 && kb <= 64 * kw && n_opt >= 1 && file.size() >= 5 + n_opt + n * kw + n, "bad table file");
        const uint64_t* k = file.data() + 5 + n_opt;
        const uint64_t* c = k + n * kw;
        keys = new Exact<uint64_t>(n * kw);
        counts = new Exact<uint32_t>(n);
        for (size_t i = 0; i < n * kw; ++i) keys->p[i] = k[i];
        for (size_t i = 0; i < n; ++i) counts->p[i] = (uint32_t)c[i];
        v.keys = n ? keys->p : nullptr;
        v.counts = n ? counts->p : nullptr;
        v.n = (uint32_t)n;
        v.key_words = (uint32_t)kw;
        v.key_bits = (uint32_t)kb;
        v.prefix_bits = bllk::choose_prefix_bits((int)(int64_t)file[5], n, (uint32_t)kb);
        index = new Exact<uint32_t>(((size_t)1 << v.prefix_bits) + 1);
        v.index = index->p;
        for (uint64_t j = 0; j <= (1ull << v.prefix_bits); ++j) index->p[j] = bllk::index_entry(v, (uint32_t)j);
    }
    ~EmuTable()
    {
        delete keys;
        delete counts;
        delete index;
    }
    EmuTable(const EmuTable&) = delete;
    EmuTable& operator=(const EmuTable&) = delete;
};

// one call: the identity fill as read_counts_init_kernel does it, then read_counts_kernel's tile loop
static void run_call(blrc::ReadCountParams& p, uint32_t mode, bl::Kmer128Acc& acc)
{
    if (mode == 0) {
        uint64_t lo, hi;
        blrc::touched_span(p, lo, hi);
        if (lo <= hi)
            for (uint64_t i = 0; i <= hi - lo; ++i) p.records[lo + i] = blrc::identity_record();
    }
    std::vector<uint32_t> codes(bl::NCHUNK_POS), flags(bl::NCHUNK_POS);
    for (int tile = 0; tile < p.km.n_tiles; ++tile) {
        const int64_t q0 = p.km.origin + (int64_t)tile * bl::H;
        stage_all(p.km, codes, flags, q0);
        for (int wv = 0; wv < bl::TPB / 64; ++wv) {
            uint64_t bound[2] = {0, 0};
            if (p.offsets)
                for (int lane = 0; lane < 2; ++lane) bound[lane] = blrc::seq_of(p.offsets, blrc::wave_bound_position(p, q0, wv, lane), 0, p.n_seqs - 1);
            uint32_t start16[64];
            blrc::Part head[64], run[64], prev[64];
            uint64_t starts = 0;  // the ballot
            for (int lane = 0; lane < 64; ++lane) {
                blrc::read_counts_lane(p, codes.data(), flags.data(), wv * 64 + lane, q0, bound[0], bound[1], acc, start16[lane], head[lane], run[lane]);
                if (start16[lane]) starts |= 1ull << lane;
            }
            for (int d = 1; d < 64; d <<= 1) {
                for (int lane = 0; lane < 64; ++lane) prev[lane] = run[lane];
                for (int lane = 0; lane < 64; ++lane) {
                    const blrc::Part theirs = prev[lane >= d ? lane - d : lane];  // __shfl_up: a lane below d gets its own
                    if (blrc::wave_scan_takes(lane, d, blrc::wave_seg_head(starts, lane))) run[lane] = blrc::merge(theirs, run[lane]);
                }
            }
            for (int lane = 0; lane < 64; ++lane) {
                const blrc::Part below = lane ? run[lane - 1] : blrc::identity_part();
                blrc::wave_close(p, wv * 64 + lane, q0, start16[lane], head[lane], run[lane], below, bound[0], bound[1]);
            }
        }
    }
}

int main(int argc, char** argv)
{
    CHECK(argc >= 12 && (argc - 9) % 3 == 0,
          "usage: emu_read_counts <batch> <table> <offsets|-> <read_len> <k> <canonical> <drop_last> <min_count> <first> <n> <mode> [...]");
    const EmuBatch batch(argv[1]);
    const EmuTable table(argv[2]);
    const bool null_offsets = std::strcmp(argv[3], "-") == 0;
    const std::vector<uint64_t> offs_file = null_offsets ? std::vector<uint64_t>() : read_words(argv[3]);
    CHECK(null_offsets || offs_file.size() == batch.n_seqs + 1, "the offsets file must hold n_seqs + 1 words");
    Exact<uint64_t> offsets(offs_file.size());
    for (size_t i = 0; i < offs_file.size(); ++i) offsets.p[i] = offs_file[i];
    const uint64_t read_len = std::strtoull(argv[4], nullptr, 10);
    const int k = std::atoi(argv[5]);
    const int canonical = std::atoi(argv[6]), drop_last = std::atoi(argv[7]);
    const uint32_t min_count = (uint32_t)std::strtoull(argv[8], nullptr, 10);
    CHECK(k >= 1 && k <= bl::MAX_UNIT128 && (uint32_t)(2 * k) <= table.v.key_bits && (table.v.key_words == 2 || k <= 32), "bad k for this table");
    CHECK(min_count >= 1 && batch.n_seqs >= 1, "min_count and n_seqs are at least 1");
    CHECK(!null_offsets || read_len != 0 || batch.n_seqs == 1, "NULL offsets: a single sequence or fixed-length reads");

    Exact<blrc::Record> records(batch.n_seqs);
    std::memset(records.p, 0xC5, batch.n_seqs * sizeof(blrc::Record));
    for (int a = 9; a + 2 < argc; a += 3) {
        const uint64_t first = std::strtoull(argv[a], nullptr, 10), n_arg = std::strtoull(argv[a + 1], nullptr, 10);
        const uint32_t mode = (uint32_t)std::atoi(argv[a + 2]);
        if (mode == 2) {
            for (uint64_t i = 0; i < batch.n_seqs; ++i) records.p[i] = blrc::identity_record();
            continue;
        }
        const uint64_t end = (n_arg == 0 || first + n_arg > batch.n_bases) ? batch.n_bases : first + n_arg;
        CHECK(first < end && mode <= 1, "empty range or bad mode");
        blrc::ReadCountParams p{};
        batch.describe(p.km);
        bl::plan_kmers128((int64_t)first, (int64_t)end, p.km);
        p.km.unit = k;
        p.km.canonical = canonical;
        p.km.drop_last = drop_last;
        p.table = table.v;
        p.min_count = min_count;
        p.offsets = null_offsets ? nullptr : offsets.p;
        p.n_seqs = batch.n_seqs;
        p.read_len = null_offsets ? read_len : 0;
        p.records = records.p;
        bl::Kmer128Acc acc{0, 0, 0, 0, 0};
        run_call(p, mode, acc);
        std::printf("result %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)first, (unsigned long long)n_arg, acc.cnt, acc.xlo, acc.xhi, acc.xh, acc.sx);
    }
    for (uint64_t i = 0; i < batch.n_seqs; ++i) {
        const blrc::Record& r = records.p[i];
        std::printf("record %llu %u %u %u %u %u %u %llu %llu %llu\n", (unsigned long long)i, r.n_kmers, r.n_found, r.n_solid, r.min_count, r.max_count, r.reserved,
                    (unsigned long long)r.sum_counts, (unsigned long long)r.weak_begin, (unsigned long long)r.weak_end);
    }
    return 0;
}
