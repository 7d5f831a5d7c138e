// CPU emulation of the table graph (biolib_amd/csrc/bl_graph_core.hpp), built with -DBL_CPU_EMU under AddressSanitizer / UBSan by
// tests/test_emu_graph.py.  Every pass of bl_table_adjacency and bl_table_unitigs runs lane by lane in the order the host driver of
// bl_graph.hip launches them: the key check, the mask pass, the link pass, the statistics, pointer doubling over ping-pong records with
// the cycle cut and the second labelling, placement, numbering, lengths, offsets, emission.  The table, its prefix index and every
// intermediate and result array are heap arrays of EXACTLY the needed lengths — n keys, 2^P + 1 index words, 2n links and records,
// n_unitigs + 1 offsets, n_bases bytes — so that an access one element outside is a sanitizer report.
// usage: emu_graph input.bin
//   input.bin: uint64 key_words, key_bits, n, k, option ("table_prefix_bits": 0 .. 24 forced), then the sorted keys (key_words words
//   each: low, high) and n uint32 counts
//   prints "refused <reason>" or "bad <slot>", else the lines  mask / links / stats / rounds / nodes / offsets / sums / bases
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../biolib_amd/csrc/bl_graph_core.hpp"

using namespace blgr;
typedef unsigned long long ull;

template <int W>
static int run(const TableView& t, const uint32_t* counts, uint32_t k)
{
    const uint32_t n = t.n;
    for (uint32_t i = 0; i < n; ++i)
        if (bad_key<W>(t, k, i)) { std::printf("bad %u\n", i); return 0; }
    // mask and link passes
    std::unique_ptr<uint8_t[]> mask(new uint8_t[n]);
    std::unique_ptr<uint32_t[]> nbr(new uint32_t[2 * (size_t)n]), links(new uint32_t[2 * (size_t)n]);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t l, r;
        mask[i] = (uint8_t)mask_thread<W>(t, k, i, l, r);
        nbr[2 * (size_t)i] = l;
        nbr[2 * (size_t)i + 1] = r;
    }
    for (uint32_t s = 0; s < 2 * n; ++s) links[s] = link_thread(mask.get(), nbr.get(), s);
    ull stats[9] = {n, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        const KeyStats st = key_stats(mask.get(), links.get(), i);
        stats[1] += st.arcs;
        stats[2] += st.isolated;
        stats[3] += st.dead_end_sides;
        stats[4] += st.branch_sides;
        stats[5] += st.linked_sides;
    }
    std::printf("mask");
    for (uint32_t i = 0; i < n; ++i) std::printf(" %02x", mask[i]);
    std::printf("\nlinks");
    for (uint32_t s = 0; s < 2 * n; ++s) std::printf(" %x", links[s]);
    std::printf("\n");

    // labelling: ping-pong records; the links are a copy the cut may change
    std::unique_ptr<uint32_t[]> work(new uint32_t[2 * (size_t)n]);
    std::memcpy(work.get(), links.get(), 2 * (size_t)n * sizeof(uint32_t));
    std::unique_ptr<Rec[]> ra(new Rec[2 * (size_t)n]), rb(new Rec[2 * (size_t)n]);
    Rec* cur = ra.get();
    Rec* nxt = rb.get();
    const uint32_t bound = max_rounds(n);
    ull rounds_total = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        for (uint32_t s = 0; s < 2 * n; ++s) cur[s] = label_init(work.get(), s);
        bool settled = false;
        for (uint32_t round = 0; round < bound + (uint32_t)attempt && !settled; ++round) {
            bool any = false;
            for (uint32_t s = 0; s < 2 * n; ++s) {
                bool live;
                nxt[s] = label_step(cur, s, live);
                any = any || live;
            }
            Rec* swap = cur;
            cur = nxt;
            nxt = swap;
            ++rounds_total;
            settled = !any;
        }
        if (settled) break;
        if (attempt == 1) { std::printf("internal: states unfinished after the cut\n"); return 1; }
        ull cuts = 0;
        for (uint32_t i = 0; i < n; ++i) cuts += cut_cycle_thread(cur, work.get(), i);
        stats[7] = cuts;
        if (!cuts) break;  // (every chain ended in the last round allowed)
    }
    // placement, numbering, lengths, offsets
    std::unique_ptr<Placed[]> placed(new Placed[n]);
    std::unique_ptr<ull[]> number(new ull[(size_t)n + 1]);
    ull n_unitigs = 0;
    for (uint32_t i = 0; i < n; ++i) {
        placed[i] = place_thread(cur, i);
        number[i] = n_unitigs;
        n_unitigs += (placed[i].rank_flip >> 1) == 0;
    }
    number[n] = n_unitigs;
    std::unique_ptr<uint64_t[]> offsets(new uint64_t[n_unitigs + 1]);
    std::unique_ptr<ull[]> sums(new ull[n_unitigs]);
    std::vector<ull> nodes(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        nodes[2 * (size_t)i] = number[placed[i].start];
        nodes[2 * (size_t)i + 1] = placed[i].rank_flip;
        if ((placed[i].rank_flip >> 1) == 0) {
            offsets[number[i]] = (ull)placed[i].length + k - 1;  // the length; summed below
            if (placed[i].length > stats[8]) stats[8] = placed[i].length;
        }
    }
    ull total = 0;
    for (ull u = 0; u < n_unitigs; ++u) {
        const ull len = offsets[u];
        offsets[u] = total;
        total += len;
        sums[u] = 0;
    }
    offsets[n_unitigs] = total;
    stats[6] = n_unitigs;
    std::unique_ptr<uint8_t[]> bases(new uint8_t[total]);
    std::memset(bases.get(), '?', total);
    for (uint32_t i = 0; i < n; ++i) {
        const ull u = nodes[2 * (size_t)i];
        emit_thread<W>(t, k, i, (uint32_t)nodes[2 * (size_t)i + 1], offsets[u], bases.get());
        sums[u] += counts[i];
    }
    bool ragged = false;
    const ull fixed = n_unitigs > 1 && total % n_unitigs == 0 ? total / n_unitigs : 0;
    for (ull u = 0; fixed && u < n_unitigs; ++u) ragged = ragged || breaks_uniform(offsets.get(), n_unitigs, fixed, u);
    std::printf("stats");
    for (int j = 0; j < 9; ++j) std::printf(" %llu", stats[j]);
    std::printf("\nrounds %llu fixed %llu\nnodes", rounds_total, ragged ? 0ull : fixed);
    for (size_t j = 0; j < nodes.size(); ++j) std::printf(" %llu", nodes[j]);
    std::printf("\noffsets");
    for (ull u = 0; u <= n_unitigs; ++u) std::printf(" %llu", (ull)offsets[u]);
    std::printf("\nsums");
    for (ull u = 0; u < n_unitigs; ++u) std::printf(" %llu", sums[u]);
    std::printf("\nbases ");
    std::fwrite(bases.get(), 1, total, stdout);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s input.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[5];
    if (std::fread(head, 8, 5, f) != 5) return 2;
    const uint32_t kw = (uint32_t)head[0], key_bits = (uint32_t)head[1], n = (uint32_t)head[2], k = (uint32_t)head[3];
    const int why = refuse(k, kw, key_bits, head[2]);  // (before anything is allocated: the test of n >= 2^31 sends no keys)
    if (why) { std::printf("refused %d\n", why); return 0; }
    if (argc > 2) { std::printf("accepted\n"); return 0; }  // (any second argument: the argument check alone)
    std::unique_ptr<uint64_t[]> keys(new uint64_t[(size_t)n * kw]);
    std::unique_ptr<uint32_t[]> counts(new uint32_t[n]);
    if (n && (std::fread(keys.get(), 8 * kw, n, f) != n || std::fread(counts.get(), 4, n, f) != n)) return 2;
    std::fclose(f);
    TableView t{};
    t.keys = keys.get();
    t.counts = counts.get();
    t.n = n;
    t.key_words = kw;
    t.key_bits = key_bits;
    t.prefix_bits = bllk::choose_prefix_bits((int)head[4], n, key_bits);
    std::unique_ptr<uint32_t[]> index(new uint32_t[((size_t)1 << t.prefix_bits) + 1]);
    t.index = index.get();
    for (uint32_t j = 0; j <= (1u << t.prefix_bits); ++j) index[j] = bllk::index_entry(t, j);
    return kw == 2 ? run<2>(t, counts.get(), k) : run<1>(t, counts.get(), k);
}
