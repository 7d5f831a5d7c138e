// CPU emulation of the count-table algebra (biolib_amd/csrc/bl_table_ops_core.hpp), built with -DBL_CPU_EMU under AddressSanitizer /
// UBSan by tests/test_emu_table_ops.py.  The four stages of bl_table_combine run lane by lane: the partition (one thread per tile
// boundary), the count pass (staging, walk, statistics, tile totals), the exclusive scan of the tile totals and the write pass (staging,
// walk, workgroup prefix, replay).  The tables, what stands for LDS and the result are heap arrays of EXACTLY the needed lengths — na
// and nb keys and counts, laf + la + lbx staged keys, la + lbx staged counts, n_out result entries — so that an access one element
// outside a range is a sanitizer report.
// usage: emu_table_ops input.bin
//   input.bin: uint32 key_words, uint32 n_rules, uint64 na, uint64 nb, uint64 limit (the host-side capacity check's; 0: the library's
//   2^32 — the test hook for the BL_ERR_CAPACITY branch), A keys (key_words words each: low, high), A counts (uint32), B keys, B counts,
//   then n_rules rules of four uint32: op, mode, count_lo, count_hi
//   prints per rule  "stats <n_a_only> <n_b_only> <n_both> <n_out> <sum_min> <sum_max> <sum_out> <written> <status>"  (status: ok,
//   capacity — nothing written — or invalid — the rule is refused, nothing run), "keys <hex>..." and "counts <dec>..."
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../biolib_amd/csrc/bl_table_ops_core.hpp"

using namespace bltop;
typedef unsigned long long ull;

static void print_key(const Key1& k) { std::printf(" %llx", (ull)k.lo); }
static void print_key(const Key2& k)
{
    if (k.hi) std::printf(" %llx%016llx", (ull)k.hi, (ull)k.lo);
    else std::printf(" %llx", (ull)k.lo);
}

template <typename K>
struct Staged {
    std::unique_ptr<K[]> keys;
    std::unique_ptr<uint32_t[]> counts;
    const K* sa;
    const K* sb;
    const uint32_t* ca;
    const uint32_t* cb;
};

template <typename K>
static bool stage(const TileRange& r, const K* a, const uint32_t* ca, const K* b, const uint32_t* cb, Staged<K>& s)
{
    if (r.laf + r.la + r.lbx > (uint32_t)lds_keys<K>() || r.la + r.lbx > (uint32_t)lds_counts<K>()) return false;
    s.keys.reset(new K[r.laf + r.la + r.lbx]);
    s.counts.reset(new uint32_t[r.la + r.lbx]);
    for (uint32_t tid = 0; tid < (uint32_t)TPB; ++tid) tile_stage_thread<K>(r, a, ca, b, cb, s.keys.get(), s.counts.get(), tid);
    s.sa = s.keys.get() + r.laf;
    s.sb = s.keys.get() + r.laf + r.la;
    s.ca = s.counts.get();
    s.cb = s.counts.get() + r.la;
    return true;
}

template <typename K>
static int run(FILE* f, uint32_t n_rules, ull na, ull nb, ull limit)
{
    constexpr uint32_t W = sizeof(K) / 8;
    std::unique_ptr<K[]> a(new K[na]), b(new K[nb]);
    std::unique_ptr<uint32_t[]> ca(new uint32_t[na]), cb(new uint32_t[nb]);
    if ((na && std::fread(a.get(), 8 * W, na, f) != na) || (na && std::fread(ca.get(), 4, na, f) != na)) return 2;
    if ((nb && std::fread(b.get(), 8 * W, nb, f) != nb) || (nb && std::fread(cb.get(), 4, nb, f) != nb)) return 2;
    std::vector<uint32_t> rules(4 * (size_t)n_rules);
    if (n_rules && std::fread(rules.data(), 16, n_rules, f) != n_rules) return 2;

    const ull total = na + nb;
    const ull TILE = (ull)Geo<K>::TILE;
    const ull n_tiles = (total + TILE - 1) / TILE;
    // stage 1 — the partition: one thread per tile boundary
    std::unique_ptr<ull[]> splits(new ull[n_tiles + 1]);
    for (ull t = 0; t <= n_tiles; ++t) {
        const ull d = t * TILE < total ? t * TILE : total;
        splits[t] = diag_split<K, ull>(a.get(), na, b.get(), nb, d);
    }
    for (uint32_t q = 0; q < n_rules; ++q) {
        if (!rule_ok(rules[4 * q], rules[4 * q + 1]) || rules[4 * q + 2] > rules[4 * q + 3]) {
            std::printf("stats 0 0 0 0 0 0 0 0 invalid\nkeys\ncounts\n");
            continue;
        }
        const Rule rule{rules[4 * q], rules[4 * q + 1], rules[4 * q + 2], rules[4 * q + 3]};
        // stage 2 — the count pass: one workgroup per tile
        ull stats[7] = {0, 0, 0, 0, 0, 0, 0};
        std::unique_ptr<ull[]> totals(new ull[n_tiles]), bases(new ull[n_tiles]);
        for (ull t = 0; t < n_tiles; ++t) {
            const TileRange r = tile_range<K>(splits.get(), t, na, nb);
            Staged<K> s;
            if (!stage<K>(r, a.get(), ca.get(), b.get(), cb.get(), s)) { std::printf("tile %llu stages too much\n", t); return 1; }
            ull tile_out = 0;
            for (uint32_t tid = 0; tid < (uint32_t)TPB; ++tid) {
                ThreadStats st{0, 0, 0, 0, 0, 0, 0};
                Walk<K> w;
                tile_thread_walk<K>(rule, s.sa, s.ca, r.la, r.laf, s.sb, s.cb, r.lb, r.lbx, tid, st, w);
                stats[0] += st.n_a_only;
                stats[1] += st.n_b_only;
                stats[2] += st.n_both;
                stats[3] += st.n_out;
                stats[4] += st.sum_min;
                stats[5] += st.sum_max;
                stats[6] += st.sum_out;
                tile_out += st.n_out;
            }
            totals[t] = tile_out;
        }
        const ull n_out = stats[3];
        // the host's check between the passes
        if (!fits_table(n_out, limit ? limit : MAX_OUT)) {
            std::printf("stats %llu %llu %llu %llu %llu %llu %llu 0 capacity\nkeys\ncounts\n", stats[0], stats[1], stats[2], stats[3], stats[4], stats[5], stats[6]);
            continue;
        }
        // stage 3 — the exclusive scan of the tile totals
        ull run_sum = 0;
        for (ull t = 0; t < n_tiles; ++t) {
            bases[t] = run_sum;
            run_sum += totals[t];
        }
        // stage 4 — the write pass
        std::unique_ptr<K[]> out_keys(new K[n_out]);
        std::unique_ptr<uint32_t[]> out_counts(new uint32_t[n_out]);
        ull written = 0;
        for (ull t = 0; t < n_tiles; ++t) {
            const TileRange r = tile_range<K>(splits.get(), t, na, nb);
            Staged<K> s;
            if (!stage<K>(r, a.get(), ca.get(), b.get(), cb.get(), s)) return 1;
            std::vector<Walk<K>> walks(TPB);
            for (uint32_t tid = 0; tid < (uint32_t)TPB; ++tid) {
                ThreadStats st{0, 0, 0, 0, 0, 0, 0};
                tile_thread_walk<K>(rule, s.sa, s.ca, r.la, r.laf, s.sb, s.cb, r.lb, r.lbx, tid, st, walks[tid]);
            }
            uint32_t rank = 0;  // the workgroup's exclusive prefix of the emit counts
            for (uint32_t tid = 0; tid < (uint32_t)TPB; ++tid) {
                const uint32_t mine = (uint32_t)__builtin_popcount(walks[tid].emit);
                const ull first = bases[t] + rank;
                if (first + mine <= n_out) written += tile_thread_write<K>(walks[tid], s.sa, s.sb, out_keys.get() + first, out_counts.get() + first);
                rank += mine;
            }
        }
        std::printf("stats %llu %llu %llu %llu %llu %llu %llu %llu ok\nkeys", stats[0], stats[1], stats[2], stats[3], stats[4], stats[5], stats[6], written);
        for (ull x = 0; x < n_out; ++x) print_key(out_keys[x]);
        std::printf("\ncounts");
        for (ull x = 0; x < n_out; ++x) std::printf(" %u", out_counts[x]);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s input.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t head[2];
    uint64_t n[3];
    if (std::fread(head, 4, 2, f) != 2 || std::fread(n, 8, 3, f) != 3) return 2;
    const int rc = head[0] == 2 ? run<Key2>(f, head[1], n[0], n[1], n[2]) : run<Key1>(f, head[1], n[0], n[1], n[2]);
    std::fclose(f);
    return rc;
}
