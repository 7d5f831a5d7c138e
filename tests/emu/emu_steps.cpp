// CPU emulation of the reads' steps, the link support and the GAF writer (biolib_amd/csrc/bl_steps_core.hpp), built with -DBL_CPU_EMU under
// AddressSanitizer / UBSan by tests/test_emu_steps.py.  Every pass of bl_scan_read_steps, bl_link_support and bl_steps_format_gaf runs lane
// by lane in the order the host driver of bl_steps.hip launches them: the node pass tile by tile, the heads counted per workgroup, their
// sum, the heads and tails, the records; then the support and the five stages of the text.  The table, its prefix index, the nodes, the
// offsets, the bases with their start bits, the words, the records and the text are heap arrays of EXACTLY the needed lengths, so that
// an access one element outside is a sanitizer report.
// usage: emu_steps input.bin out.gaf
//   input.bin: tests/steps_cases.py: steps_file.  mode 0: for every range the lines "range <first> <n>", "stats <six words>" and
//   "steps <six words per record>"; then, over the whole batch, "support <n_links words>", "sstats <two words>" and the text in out.gaf.
//   mode 1: besides, the batch cut at every position: the records of the two ranges folded must be the whole call's and the statistics
//   must add up ("cuts <number>").  mode 2: nodes, offsets, records and link words are overwritten with anything first (trusted for
//   content, not for safety): only the sanitizers judge ("garbage ok").
#define EMU_NAME "emu_steps"
#include <algorithm>
#include <memory>
#include <string>

#include "emu128_common.hpp"
#include "../../biolib_amd/csrc/bl_graph_core.hpp"
#include "../../biolib_amd/csrc/bl_steps_core.hpp"

typedef unsigned long long ull;
using namespace blst;

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

struct Input {
    bllk::TableView t{};
    uint32_t k = 0;
    uint64_t n_unitigs = 0, n_bases = 0, n_seqs = 0, fixed = 0, n_links = 0;
    Node* nodes = nullptr;
    uint64_t* unitig_offsets = nullptr;
    uint64_t* seq_offsets = nullptr;  // NULL for a fixed-length or a single-sequence batch
    uint8_t* bases = nullptr;
    uint32_t* start_bits = nullptr;   // NULL: one sequence
    uint64_t* link_offsets = nullptr;
    LinkWords* links = nullptr;
};

struct Result {
    std::vector<Step> steps;
    ull stats[6] = {0, 0, 0, 0, 0, 0};  // n_valid, n_found, n_steps, n_chains, n_linked, longest_step
};

// bl_scan_read_steps as the driver runs it, at the capacities n_steps (an array of exactly that length), n_steps - 1 and the sizing call
static void run_steps(const Input& in, uint64_t first, uint64_t n_arg, Result& out)
{
    out = Result();
    const uint64_t end = (n_arg == 0 || n_arg > in.n_bases - first) ? in.n_bases : first + n_arg;
    if (end <= first) return;
    const int64_t s0 = first ? (int64_t)first - 1 : 0;
    Exact<uint64_t> words((size_t)(end - s0));
    for (size_t i = 0; i < words.n; ++i) words.p[i] = 0xEEEEEEEEEEEEEEEEull;
    NodeParams np{};
    np.km.bases = in.bases;
    np.km.n_bases = (int64_t)in.n_bases;
    np.km.start_bits = in.start_bits;
    bl::plan_kmers128(s0, (int64_t)end, np.km);
    np.km.unit = (int32_t)in.k;
    np.km.canonical = 1;
    np.table = in.t;
    np.nodes = in.nodes;
    np.unitig_offsets = in.unitig_offsets;
    np.n_unitigs = in.n_unitigs;
    np.first = (int64_t)first;
    np.words = words.p;
    std::vector<uint32_t> codes(bl::NCHUNK_POS), flags(bl::NCHUNK_POS);
    for (int tile = 0; tile < np.km.n_tiles; ++tile) {
        const int64_t q0 = np.km.origin + (int64_t)tile * bl::H;
        stage_all(np.km, codes, flags, q0);
        for (int tid = 0; tid < bl::TPB; ++tid) {
            uint32_t v = 0, f = 0;
            node_thread(np, codes.data(), flags.data(), tid, q0, v, f);
            out.stats[0] += v;
            out.stats[1] += f;
        }
    }
    for (size_t i = 0; i < words.n; ++i) CHECK(words.p[i] != 0xEEEEEEEEEEEEEEEEull, "word %zu was not written", i);

    StepParams sp{words.p, s0, in.start_bits, (int64_t)first, (int64_t)end};
    const uint64_t n_blocks = (end - first + STPB - 1) / STPB;
    std::vector<uint64_t> block_base(n_blocks + 1, 0);
    uint64_t n_tails = 0;
    for (uint64_t blk = 0; blk < n_blocks; ++blk) {
        uint64_t cnt = 0;
        for (int tid = 0; tid < STPB; ++tid) {
            const int64_t pos = (int64_t)first + (int64_t)blk * STPB + tid;
            const uint32_t cls = pos < (int64_t)end ? classify(sp, pos) : 0u;
            cnt += cls & HEAD;
            n_tails += (cls & TAIL) ? 1 : 0;
        }
        block_base[blk + 1] = block_base[blk] + cnt;
    }
    const uint64_t n_steps = block_base[n_blocks];
    CHECK(n_tails == n_steps, "%llu heads and %llu tails", (ull)n_steps, (ull)n_tails);
    out.stats[2] = n_steps;
    if (n_steps == 0) return;
    Exact<uint32_t> heads(n_steps), tails(n_steps);
    for (uint64_t j = 0; j < n_steps; ++j) heads.p[j] = tails.p[j] = 0xEEEEEEEEu;
    for (uint64_t blk = 0; blk < n_blocks; ++blk) {
        uint64_t before = block_base[blk];
        for (int tid = 0; tid < STPB; ++tid) {
            const int64_t pos = (int64_t)first + (int64_t)blk * STPB + tid;
            const uint32_t cls = pos < (int64_t)end ? classify(sp, pos) : 0u;
            if (cls) emit_ends(sp, pos, cls, before, n_steps, heads.p, tails.p);
            before += cls & HEAD;
        }
    }
    FinishParams fp{};
    fp.sp = sp;
    fp.heads = heads.p;
    fp.tails = tails.p;
    fp.n_steps = n_steps;
    fp.seq_offsets = in.seq_offsets;
    fp.n_seqs = in.n_seqs;
    fp.read_len = in.seq_offsets ? 0 : in.fixed;
    Exact<Step> steps(n_steps);  // capacity n_steps; a smaller capacity and the sizing call store nothing at all
    for (uint64_t j = 0; j < n_steps; ++j) {
        CHECK(heads.p[j] != 0xEEEEEEEEu && tails.p[j] != 0xEEEEEEEEu && heads.p[j] <= tails.p[j], "step %llu has no head or no tail", (ull)j);
        CHECK(j == 0 || tails.p[j - 1] < heads.p[j], "heads and tails do not alternate at step %llu", (ull)j);
        const Step st = make_step(fp, j);
        steps.p[j] = st;
        out.stats[3] += st.flags == 0;
        out.stats[4] += (st.flags & LINKED) ? 1 : 0;
        out.stats[5] = std::max<ull>(out.stats[5], st.n_kmers);
    }
    out.steps.assign(steps.p, steps.p + n_steps);
}

static void print_result(const Result& r)
{
    std::printf("stats");
    for (int j = 0; j < 6; ++j) std::printf(" %llu", r.stats[j]);
    std::printf("\nsteps");
    for (const Step& s : r.steps) std::printf(" %llu %llu %u %u %u %u", (ull)s.pos, (ull)s.seq, s.end, s.offset, s.n_kmers, s.flags);
    std::printf("\n");
}

// bl_link_support as the driver runs it
static void run_support(const Input& in, const Step* steps, uint64_t n_steps, std::vector<uint32_t>& support, ull stats[2])
{
    Exact<uint32_t> sup(in.n_links);
    for (uint64_t i = 0; i < in.n_links; ++i) sup.p[i] = 0;
    stats[0] = stats[1] = 0;
    if (n_steps > 1 && in.n_unitigs) {
        SupportParams p{steps, n_steps, in.link_offsets, in.links, in.n_links, in.n_unitigs, sup.p};
        const uint64_t threads = (n_steps - 1 + STPB - 1) / STPB * STPB;
        for (uint64_t i = 0; i < threads; ++i) {
            const int r = support_thread(p, i);
            stats[0] += r != 0;
            stats[1] += r == 2;
        }
    }
    support.assign(sup.p, sup.p + in.n_links);
}

// bl_steps_format_gaf as the driver runs it; false: a step carries CONTINUED
static bool run_gaf(const Input& in, const Step* steps, uint64_t n_steps, const uint64_t head[16], const char* prefixes, std::vector<uint8_t>& text)
{
    text.clear();
    if (n_steps == 0) return true;
    GafParams p{};
    p.steps = steps;
    p.n_steps = n_steps;
    p.unitig_offsets = in.unitig_offsets;
    p.n_unitigs = in.n_unitigs;
    p.seq_offsets = in.seq_offsets;
    p.n_seqs = in.n_seqs;
    p.read_len = in.seq_offsets ? 0 : in.fixed;
    p.n_bases = in.n_bases;
    p.k = in.k;
    p.read_prefix_len = (uint32_t)head[14];
    p.seg_prefix_len = (uint32_t)head[15];
    for (uint32_t i = 0; i < p.read_prefix_len; ++i) p.read_prefix[i >> 3] |= (uint64_t)(uint8_t)prefixes[i] << (8 * (i & 7));
    for (uint32_t i = 0; i < p.seg_prefix_len; ++i) p.seg_prefix[i >> 3] |= (uint64_t)(uint8_t)prefixes[16 + i] << (8 * (i & 7));
    p.read_first = head[12];
    p.seg_first = head[13];
    const uint64_t n1 = n_steps + 1;
    Exact<uint64_t> measures(4 * n1), sums(4 * n1);
    p.kmers = measures.p;
    p.keys = measures.p + n1;
    p.path = measures.p + 2 * n1;
    p.head = measures.p + 3 * n1;
    uint32_t continued = 0;
    for (uint64_t i = 0; i < (n1 + STPB - 1) / STPB * STPB; ++i) continued |= measure_step(p, i);
    if (continued) return false;
    for (int j = 0; j < 4; ++j) {
        uint64_t total = 0;
        for (uint64_t i = 0; i < n1; ++i) {
            sums.p[j * n1 + i] = total;
            total += measures.p[j * n1 + i];
        }
    }
    p.kmers_sum = sums.p;
    p.keys_sum = sums.p + n1;
    p.path_sum = sums.p + 2 * n1;
    p.head_sum = sums.p + 3 * n1;
    p.n_chains = p.head_sum[n_steps];
    Exact<uint64_t> chain_begin(p.n_chains + 1), line_len(p.n_chains + 1), line_off(p.n_chains + 1);
    p.chain_begin = chain_begin.p;
    p.line_len = line_len.p;
    for (uint64_t i = 0; i < (n1 + STPB - 1) / STPB * STPB; ++i) chain_first(p, i);
    for (uint64_t c = 0; c < (p.n_chains + 1 + STPB - 1) / STPB * STPB; ++c) chain_length(p, c);
    uint64_t total = 0;
    for (uint64_t c = 0; c <= p.n_chains; ++c) {
        line_off.p[c] = total;
        total += line_len.p[c];
    }
    p.line_off = line_off.p;
    p.total = total;
    Exact<uint8_t> out(total);
    std::memset(out.p, 0, total);
    p.out = out.p;
    for (uint64_t i = 0; i < (n_steps + STPB - 1) / STPB * STPB; ++i) write_step(p, i);
    for (uint64_t x = 0; x < total; ++x) CHECK(out.p[x] != 0, "byte %llu of the text was not written", (ull)x);
    text.assign(out.p, out.p + total);
    return true;
}

static bool same_step(const Step& a, const Step& b)
{
    return a.pos == b.pos && a.seq == b.seq && a.end == b.end && a.offset == b.offset && a.n_kmers == b.n_kmers && a.flags == b.flags;
}

int main(int argc, char** argv)
{
    CHECK(argc >= 3, "usage: emu_steps input.bin out.gaf");
    FILE* f = std::fopen(argv[1], "rb");
    CHECK(f, "cannot open %s", argv[1]);
    uint64_t head[16];
    char prefixes[32];
    CHECK(std::fread(head, 8, 16, f) == 16 && std::fread(prefixes, 1, 32, f) == 32, "short file");
    const uint32_t kw = (uint32_t)head[0], key_bits = (uint32_t)head[1], n = (uint32_t)head[2], k = (uint32_t)head[3];
    int why = blgr::refuse(k, kw, key_bits, head[2]);
    if (!why) why = refuse(k, head[2], head[5]);
    if (!why && refuse_rule(0, k, (int)head[14], (int)head[15], 0)) why = 8;
    if (why) {
        std::printf("refused %d\n", why);
        return 0;
    }
    Input in;
    in.k = k;
    in.n_unitigs = head[5];
    in.n_bases = head[6];
    in.n_seqs = head[7];
    in.fixed = head[8];
    in.n_links = head[9];
    const uint64_t n_ranges = head[10], mode = head[11];
    Exact<uint64_t> keys((size_t)n * kw), unitig_offsets(in.n_unitigs + 1), seq_offsets(in.n_seqs + 1), link_offsets(2 * in.n_unitigs + 1);
    Exact<Node> nodes(n);
    Exact<uint8_t> bases(in.n_bases);
    Exact<LinkWords> links(in.n_links);
    std::vector<uint64_t> ranges(2 * n_ranges);
    CHECK(std::fread(keys.p, 8, keys.n, f) == keys.n && std::fread(nodes.p, 8, n, f) == n, "short file");
    CHECK(std::fread(unitig_offsets.p, 8, unitig_offsets.n, f) == unitig_offsets.n && std::fread(seq_offsets.p, 8, seq_offsets.n, f) == seq_offsets.n, "short file");
    CHECK(std::fread(bases.p, 1, bases.n, f) == bases.n && std::fread(link_offsets.p, 8, link_offsets.n, f) == link_offsets.n, "short file");
    CHECK(std::fread(links.p, 8, links.n, f) == links.n && std::fread(ranges.data(), 8, ranges.size(), f) == ranges.size(), "short file");
    std::fclose(f);
    in.t.keys = n ? keys.p : nullptr;
    in.t.counts = nullptr;
    in.t.n = n;
    in.t.key_words = kw;
    in.t.key_bits = key_bits;
    in.t.prefix_bits = bllk::choose_prefix_bits((int)(int64_t)head[4], n, key_bits);
    Exact<uint32_t> index(((size_t)1 << in.t.prefix_bits) + 1);
    in.t.index = index.p;
    for (uint64_t j = 0; j <= (1ull << in.t.prefix_bits); ++j) index.p[j] = bllk::index_entry(in.t, (uint32_t)j);
    in.nodes = n ? nodes.p : nullptr;
    in.unitig_offsets = unitig_offsets.p;
    in.bases = bases.p;
    in.link_offsets = link_offsets.p;
    in.links = links.p;
    Exact<uint32_t> start_bits((size_t)((in.n_bases + 31) / 32 + 4));
    if (in.n_seqs > 1) {  // as the library builds them
        std::memset(start_bits.p, 0, start_bits.n * 4);
        for (uint64_t q = 0; q < in.n_seqs; ++q)
            if (seq_offsets.p[q] < in.n_bases) start_bits.p[seq_offsets.p[q] >> 5] |= 1u << (seq_offsets.p[q] & 31);
        in.start_bits = start_bits.p;
        if (!in.fixed) in.seq_offsets = seq_offsets.p;
    }

    if (mode == 2) {  // unitig numbers at, above and far above n_unitigs, any rank and flip, offsets in any order
        uint64_t x = 0x9E3779B97F4A7C15ull ^ head[2];
        auto next = [&x]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return x >> 24; };
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t r = next();
            nodes.p[i].unitig = (r & 7) == 0 ? 0xFFFFFFFFu : (uint32_t)(next() % (in.n_unitigs + 3));
            nodes.p[i].rank_flip = (r & 8) ? (uint32_t)next() : (uint32_t)(next() & 7);
        }
        for (uint64_t u = 0; u <= in.n_unitigs; ++u) unitig_offsets.p[u] = (next() & 3) == 0 ? ~0ull - next() % 5 : next() % (in.n_bases + 5);
        for (uint64_t e = 0; e <= 2 * in.n_unitigs; ++e) link_offsets.p[e] = (next() & 3) == 0 ? ~0ull - next() % 5 : next() % (in.n_links + 5);
        for (uint64_t r = 0; r < in.n_links; ++r) links.p[r] = LinkWords{(uint32_t)next(), (next() & 1) ? (uint32_t)next() : (uint32_t)(next() % (2 * in.n_unitigs + 2))};
        Result whole;
        run_steps(in, 0, 0, whole);
        std::vector<Step> steps = whole.steps;
        for (size_t j = 0; j < steps.size(); j += 3) {  // and any record
            Step& s = steps[j];
            s.pos = next();
            s.seq = (next() & 1) ? next() : next() % (in.n_seqs + 2);
            s.end = (next() & 1) ? (uint32_t)next() : (uint32_t)(next() % (2 * in.n_unitigs + 2));
            s.offset = (uint32_t)next();
            s.n_kmers = (uint32_t)next();
            s.flags = (uint32_t)(next() & 1);
        }
        Exact<Step> exact(steps.size());
        std::copy(steps.begin(), steps.end(), exact.p);
        std::vector<uint32_t> support;
        ull sstats[2];
        run_support(in, exact.p, steps.size(), support, sstats);
        std::vector<uint8_t> text;
        run_gaf(in, exact.p, steps.size(), head, prefixes, text);
        std::printf("garbage ok\n");
        return 0;
    }

    for (uint64_t r = 0; r < n_ranges; ++r) {
        Result res;
        CHECK(ranges[2 * r] <= in.n_bases, "range starts beyond the batch");
        run_steps(in, ranges[2 * r], ranges[2 * r + 1], res);
        std::printf("range %llu %llu\n", (ull)ranges[2 * r], (ull)ranges[2 * r + 1]);
        print_result(res);
    }
    Result whole;
    run_steps(in, 0, 0, whole);
    if (mode == 1) {
        for (uint64_t c = 1; c < in.n_bases; ++c) {
            Result a, b;
            run_steps(in, 0, c, a);
            run_steps(in, c, 0, b);
            std::vector<Step> folded = a.steps;
            for (const Step& s : b.steps) {
                if (s.flags & CONTINUED) {
                    CHECK(!folded.empty() && &s == &b.steps[0] && s.pos == c, "cut %llu: a CONTINUED record that is not the range's first", (ull)c);
                    folded.back().n_kmers += s.n_kmers;
                } else {
                    folded.push_back(s);
                }
            }
            CHECK(folded.size() == whole.steps.size(), "cut %llu: %zu folded records, %zu whole", (ull)c, folded.size(), whole.steps.size());
            for (size_t j = 0; j < folded.size(); ++j) CHECK(same_step(folded[j], whole.steps[j]), "cut %llu: record %zu differs", (ull)c, j);
            CHECK(a.stats[0] + b.stats[0] == whole.stats[0] && a.stats[1] + b.stats[1] == whole.stats[1], "cut %llu: n_valid or n_found do not add up", (ull)c);
            const ull cont = !b.steps.empty() && (b.steps[0].flags & CONTINUED) ? 1 : 0;
            CHECK(a.stats[2] + b.stats[2] == whole.stats[2] + cont && a.stats[3] + b.stats[3] == whole.stats[3] && a.stats[4] + b.stats[4] == whole.stats[4],
                  "cut %llu: n_steps, n_chains or n_linked do not add up", (ull)c);
        }
        std::printf("cuts %llu\n", (ull)(in.n_bases ? in.n_bases - 1 : 0));
    }
    Exact<Step> exact(whole.steps.size());
    std::copy(whole.steps.begin(), whole.steps.end(), exact.p);
    std::vector<uint32_t> support;
    ull sstats[2];
    run_support(in, exact.p, whole.steps.size(), support, sstats);
    std::printf("support");
    for (uint32_t v : support) std::printf(" %u", v);
    std::printf("\nsstats %llu %llu\n", sstats[0], sstats[1]);
    std::vector<uint8_t> text;
    CHECK(run_gaf(in, exact.p, whole.steps.size(), head, prefixes, text), "a whole-batch call set CONTINUED");
    FILE* g = std::fopen(argv[2], "wb");
    CHECK(g && std::fwrite(text.data(), 1, text.size(), g) == text.size() && std::fclose(g) == 0, "cannot write %s", argv[2]);
    return 0;
}
