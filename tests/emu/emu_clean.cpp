// CPU emulation of graph cleaning (biolib_amd/csrc/bl_clean_core.hpp), built with -DBL_CPU_EMU under AddressSanitizer / UBSan by
// tests/test_emu_clean.py.  bl_unitigs_mark runs lane by lane over every unitig; bl_table_remove_unitigs runs as the driver of bl_clean.hip
// launches it — the count pass tile by tile with its ballots, the sum of the tile totals, the write pass — at tiles of 1, 2 and ROWS rows,
// so that kept and dropped runs straddle every seam, and each result is checked against the plain sequential filter.  Every input,
// intermediate and result array is a heap array of EXACTLY the needed length, so that an access one element outside is a sanitizer report.
// usage: emu_clean input.bin [normal | all | none | garbage]
//   all / none: the removal with every unitig marked / no unitig marked; garbage: link offsets, link words, nodes and the removal's marks
//   are overwritten with anything first (trusted for content, not for safety) and printed, so that the model can be asked about them
//   input.bin: uint64 key_words, key_bits, n, k, flags, max_tip_keys, max_isolated_keys, max_isolated_mean, max_bubble_keys,
//   max_bubble_diff, n_unitigs, n_links and four words of 0; then n_unitigs + 1 offsets, n_unitigs sums, 2 n_unitigs + 1 link offsets,
//   n_links records; then, where n > 0, the sorted keys, n counts and n nodes
//   prints "refused <reason>", else the lines  marks / stats / used (the marks the removal took) / keys (hex words) / counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../biolib_amd/csrc/bl_clean_core.hpp"

typedef unsigned long long ull;

#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            std::printf("FAILED: ");  \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            return false;             \
        }                             \
    } while (0)

struct Table {
    const uint64_t* keys;       // [n * W]
    const uint32_t* counts;     // [n]
    const bllnk::Node* nodes;   // [n]
    uint64_t n, n_unitigs;
};

// bl_table_remove_unitigs as the driver runs it, tiles of 64 * R keys
template <int W, int R>
static bool run_remove(const Table& t, const uint8_t* marks, std::vector<uint64_t>& keys_out, std::vector<uint32_t>& counts_out)
{
    using namespace blcl;
    const uint64_t n_tiles = tiles_of<R>(t.n);
    std::unique_ptr<uint64_t[]> totals(new uint64_t[n_tiles + 1]), bases(new uint64_t[n_tiles + 1]);
    auto row_ballot = [&](uint64_t tile, int row) {
        uint64_t ballot = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const uint64_t i = tile_slot<R>(tile, row, lane);
            if (i < t.n && keeps(t.nodes, marks, t.n_unitigs, i)) ballot |= (uint64_t)1 << lane;
        }
        return ballot;
    };
    for (uint64_t tile = 0; tile < n_tiles; ++tile) {
        uint64_t total = 0;
        for (int row = 0; row < R; ++row) total += (uint64_t)__builtin_popcountll(row_ballot(tile, row));
        totals[tile] = total;
    }
    totals[n_tiles] = 0;
    uint64_t n_out = 0;
    for (uint64_t tile = 0; tile <= n_tiles; ++tile) {
        bases[tile] = n_out;
        n_out += totals[tile];
    }
    CHECK(n_out <= t.n, "%llu keys kept of %llu", (ull)n_out, (ull)t.n);
    std::unique_ptr<uint64_t[]> ok(new uint64_t[n_out * W]);
    std::unique_ptr<uint32_t[]> oc(new uint32_t[n_out]);
    std::memset(ok.get(), 0xA5, n_out * W * sizeof(uint64_t));
    std::memset(oc.get(), 0xA5, n_out * sizeof(uint32_t));
    std::vector<uint8_t> written(n_out, 0);
    for (uint64_t tile = 0; tile < n_tiles; ++tile) {
        uint64_t base = bases[tile];
        for (int row = 0; row < R; ++row) {
            const uint64_t ballot = row_ballot(tile, row);
            for (int lane = 0; lane < 64; ++lane) {
                if (!((ballot >> lane) & 1)) continue;
                const uint64_t to = base + rank_in_row(ballot, lane);
                CHECK(to < n_out && !written[to], "rows %d tile %llu: place %llu of %llu", R, (ull)tile, (ull)to, (ull)n_out);
                written[to] = 1;
                move_key<W>(t.keys, t.counts, tile_slot<R>(tile, row, lane), ok.get(), oc.get(), to);
            }
            base += (uint64_t)__builtin_popcountll(ballot);
        }
        CHECK(base == bases[tile + 1], "rows %d tile %llu ends at %llu", R, (ull)tile, (ull)base);
    }
    uint64_t j = 0;  // the plain filter
    for (uint64_t i = 0; i < t.n; ++i) {
        const uint32_t u = t.nodes[i].unitig;
        if (u < t.n_unitigs && marks[u]) continue;
        CHECK(j < n_out && std::memcmp(&ok[j * W], &t.keys[i * W], W * 8) == 0 && oc[j] == t.counts[i], "rows %d: kept key %llu", R, (ull)j);
        ++j;
    }
    CHECK(j == n_out, "rows %d: %llu keys, the filter keeps %llu", R, (ull)n_out, (ull)j);
    keys_out.assign(ok.get(), ok.get() + n_out * W);
    counts_out.assign(oc.get(), oc.get() + n_out);
    return true;
}

template <int W>
static bool run_removes(const Table& t, const uint8_t* marks)
{
    std::vector<uint64_t> k1, k2, k8;
    std::vector<uint32_t> c1, c2, c8;
    if (!run_remove<W, 1>(t, marks, k1, c1) || !run_remove<W, 2>(t, marks, k2, c2) || !run_remove<W, blcl::ROWS>(t, marks, k8, c8)) return false;
    CHECK(k1 == k2 && k1 == k8 && c1 == c2 && c1 == c8, "the tile sizes disagree");
    std::printf("keys");
    for (uint64_t w : k8) std::printf(" %llx", (ull)w);
    std::printf("\ncounts");
    for (uint32_t c : c8) std::printf(" %u", c);
    std::printf("\n");
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s input.bin [normal | all | none | garbage]\n", argv[0]); return 2; }
    const char* mode = argc > 2 ? argv[2] : "normal";
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[16];
    if (std::fread(head, 8, 16, f) != 16) return 2;
    const uint32_t kw = (uint32_t)head[0];
    const uint64_t n = head[2], nu = head[10], nl = head[11];
    blcl::Rule r{(uint32_t)head[4], (uint32_t)head[3], head[5], head[6], head[7], head[8], head[9], head[12]};
    const int why = blcl::refuse(r.flags, r.k, r.reserved, nu);
    if (why) { std::printf("refused %d\n", why); return 0; }
    std::unique_ptr<uint64_t[]> offsets(new uint64_t[nu + 1]), sums(new uint64_t[nu]), link_offsets(new uint64_t[2 * nu + 1]);
    std::unique_ptr<bllnk::Link[]> links(new bllnk::Link[nl]);
    std::unique_ptr<uint64_t[]> keys(new uint64_t[n * kw]);
    std::unique_ptr<uint32_t[]> counts(new uint32_t[n]);
    std::unique_ptr<bllnk::Node[]> nodes(new bllnk::Node[n]);
    if (std::fread(offsets.get(), 8, nu + 1, f) != nu + 1 || std::fread(sums.get(), 8, nu, f) != nu) return 2;
    if (std::fread(link_offsets.get(), 8, 2 * nu + 1, f) != 2 * nu + 1 || std::fread(static_cast<void*>(links.get()), 8, nl, f) != nl) return 2;
    if (n && (std::fread(keys.get(), 8 * kw, n, f) != n || std::fread(counts.get(), 4, n, f) != n || std::fread(static_cast<void*>(nodes.get()), 8, n, f) != n)) return 2;
    std::fclose(f);

    std::unique_ptr<uint8_t[]> marks(new uint8_t[nu]), used(new uint8_t[nu]);
    const bool garbage = std::strcmp(mode, "garbage") == 0;
    if (garbage) {  // offsets beyond the records and out of order, `to` words at and beyond the ends, unitig numbers at and above n_unitigs
        uint64_t x = 0x9E3779B97F4A7C15ull ^ (n * 31 + nu);
        auto next = [&x]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return x >> 24; };
        for (uint64_t e = 0; e <= 2 * nu; ++e) link_offsets[e] = (next() & 7) == 0 ? ~0ull - next() % 3 : next() % (nl + 3);
        for (uint64_t j = 0; j < nl; ++j) {
            links[j].from = (uint32_t)next();
            links[j].to = (next() & 7) == 0 ? 0xFFFFFFFFu - (uint32_t)(next() % 3) : (uint32_t)(next() % (2 * nu + 2));
        }
        for (uint64_t i = 0; i < n; ++i) {
            nodes[i].unitig = (next() & 7) == 0 ? 0xFFFFFFFFu : (uint32_t)(next() % (nu + 3));
            nodes[i].rank_flip = (uint32_t)next();
        }
        for (uint64_t u = 0; u < nu; ++u) used[u] = (next() & 1) ? (uint8_t)next() : 0;
        std::printf("g_link_offsets");
        for (uint64_t e = 0; e <= 2 * nu; ++e) std::printf(" %llu", (ull)link_offsets[e]);
        std::printf("\ng_links");
        for (uint64_t j = 0; j < nl; ++j) std::printf(" %u %u", links[j].from, links[j].to);
        std::printf("\ng_nodes");
        for (uint64_t i = 0; i < n; ++i) std::printf(" %u", nodes[i].unitig);
        std::printf("\n");
    }
    blcl::Graph g{offsets.get(), sums.get(), link_offsets.get(), links.get(), nu, nl};
    ull st[5] = {0, 0, 0, 0, 0};
    for (uint64_t u = 0; u < nu; ++u) {
        uint64_t L = 0, S = 0;
        const uint8_t m = blcl::mark_thread(g, r, u, L, S);
        marks[u] = m;
        st[0] += m == blcl::TIP;
        st[1] += m == blcl::ISLAND;
        st[2] += m == blcl::BUBBLE;
        if (m != blcl::KEEP) {
            st[3] += L;
            st[4] += S;
        }
    }
    std::printf("marks");
    for (uint64_t u = 0; u < nu; ++u) std::printf(" %u", marks[u]);
    std::printf("\nstats %llu %llu %llu %llu %llu %llu\n", (ull)nu, st[0], st[1], st[2], st[3], st[4]);
    if (!garbage)
        for (uint64_t u = 0; u < nu; ++u) used[u] = std::strcmp(mode, "all") == 0 ? 1 : std::strcmp(mode, "none") == 0 ? 0 : marks[u];
    std::printf("used");
    for (uint64_t u = 0; u < nu; ++u) std::printf(" %u", used[u]);
    std::printf("\n");
    Table t{keys.get(), counts.get(), nodes.get(), n, nu};
    const bool ok = kw == 2 ? run_removes<2>(t, used.get()) : run_removes<1>(t, used.get());
    return ok ? 0 : 1;
}
