// TEST INFRASTRUCTURE: the read-tiled pass 1 on a tile it does not stage (frl_tile_clean: lanes read their dwords from the batch's packed
// copy) against the same tile staged in LDS, thread by thread on the host.  A stand-alone program: tests/test_emu_direct.py builds it with
// -fsanitize=address,undefined and runs it.
//
// Three things are checked, for reads of 100, 150 and 151 bases, windows of 11 and 5, batches without and with N:
//   1. on every tile the predicate calls clean, phase_hash_frl leaves the same lane_base, jlane and h[] in every lane whether its four
//      dwords come from sh.codes or from codes_packed, and phase_window_frl_a the same vmask and occurrence bits whether it is told that
//      the tile is clean (over an LDS block full of garbage) or reads wave_bad;
//   2. the predicate is never true for a tile that stages a bad chunk, and true for every tile whose covering words of chunk_bad are zero;
//   3. the packed arrays are allocated at exactly packed_total: a read outside them, by the predicate or by a lane, is an
//      AddressSanitizer report (the batch's last tile and ranges that start at chunk 0 are among the cases).
#define BL_CPU_EMU 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../biolib_amd/csrc/bl_scan_frl.hpp"

using namespace bl;

static int g_fail = 0, g_tiles = 0, g_clean = 0, g_staged = 0, g_neighbour = 0;

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

static std::vector<uint8_t> random_text(size_t n)
{
    std::vector<uint8_t> t(n ? n : 1);
    for (size_t i = 0; i < n; ++i) t[i] = (uint8_t)"ACGT"[rnd() & 3];
    return t;
}

static void expect(bool ok, const std::string& what)
{
    if (ok) return;
    if (++g_fail <= 20) std::fprintf(stderr, "MISMATCH %s\n", what.c_str());
}

// what make_packed_codes leaves on the device, in two heap blocks of exactly packed_total chunks and packed_total / 32 words
struct Packed {
    std::unique_ptr<uint32_t[]> words, bits;
    const uint32_t* codes() const { return words.get() + PACK_LEAD; }
    const uint32_t* bad() const { return bits.get() + PACK_LEAD / 32; }
};

static Packed pack(const std::vector<uint8_t>& t, int64_t n_bases)
{
    Packed k;
    const int64_t total = packed_total(n_bases);
    k.words.reset(new uint32_t[(size_t)total]);
    k.bits.reset(new uint32_t[(size_t)(total / 32)]());
    for (int64_t i = 0; i < total; ++i) {  // thread i of pack_codes_kernel
        uint32_t code;
        if (pack_chunk(t.data(), n_bases, i - PACK_LEAD, code)) k.bits[(size_t)(i >> 5)] |= 1u << (i & 31);
        k.words[(size_t)i] = code;
    }
    return k;
}

// every tile of the plan in p (packed pointers set), NS units per lane
template <int W, int NS>
static void compare_tiles(const ScanParams& p, const std::string& name)
{
    constexpr int MODE = MODE_MINIMIZER;
    auto sh = std::make_unique<TileShared<MODE, W>>(), junk = std::make_unique<TileShared<MODE, W>>();
    std::vector<ThreadState> sa(TPB), sb(TPB), ea(TPB), eb(TPB);
    for (int tile = 0; tile < p.n_tiles; ++tile) {
        const int64_t q0 = tile_q0(p, (uint32_t)tile);
        const std::string at = name + " tile " + std::to_string(tile);
        // the predicate against what it stands for, worked out chunk by chunk
        bool staged_bad = false, words_zero = true;
        for (int c = 0; c < p.slot_chunks; ++c) {
            uint32_t code;
            const int64_t ci = (q0 >> 4) + c;
            if (packed_chunk(p, 16 * ci, code)) staged_bad = true;
            if (p.chunk_bad[ci >> 5] != 0) words_zero = false;
        }
        const bool clean = frl_tile_clean(p, q0);
        expect(!(clean && staged_bad), at + ": called clean with a bad staged chunk");
        expect(clean == words_zero, at + ": the predicate is not the OR of the covering words");
        ++g_tiles;
        if (!staged_bad && !words_zero) ++g_neighbour;  // staged for a neighbour's bad chunk: allowed
        if (!clean) {
            ++g_staged;
            continue;
        }
        ++g_clean;
        std::memset(sh.get(), 0xA5, sizeof(*sh));
        std::memset(junk.get(), 0xA5, sizeof(*junk));
        for (int tid = 0; tid < TPB; ++tid) phase_load_frl<MODE, W, true>(p, *sh, tid, q0);
        for (int approx = 0; approx < 2; ++approx) {
            for (int tid = 0; tid < TPB; ++tid) {
                sa[tid] = ThreadState{};
                sb[tid] = ThreadState{};
                if (approx) {
                    phase_hash_frl<MODE, W, NS, false, true>(p, *sh, tid, q0, (uint32_t)tile, sa[tid]);
                    phase_hash_frl<MODE, W, NS, false, true>(p, *junk, tid, q0, (uint32_t)tile, sb[tid], p.codes_packed + (q0 >> 4));
                } else {
                    phase_hash_frl<MODE, W, NS>(p, *sh, tid, q0, (uint32_t)tile, sa[tid]);
                    phase_hash_frl<MODE, W, NS>(p, *junk, tid, q0, (uint32_t)tile, sb[tid], p.codes_packed + (q0 >> 4));
                }
                const std::string who = at + (approx ? " approx" : "") + " thread " + std::to_string(tid);
                expect(sa[tid].lane_base == sb[tid].lane_base, who + " lane_base");
                expect(sa[tid].jlane == sb[tid].jlane, who + " jlane");
                for (int s = 0; s < NS; ++s) expect(sa[tid].h[s] == sb[tid].h[s], who + " h[" + std::to_string(s) + "]");
            }
            if (approx) continue;  // the window phase on the hashes themselves: its exact form needs no second run
            ea = sa;
            eb = sb;
            for (int tid = 0; tid < TPB; ++tid) {
                phase_window_frl_a<MODE, W, NS>(p, *sh, tid, ea[tid], sa.data());
                phase_window_frl_a<MODE, W, NS>(p, *junk, tid, eb[tid], sb.data(), nullptr, true);
                const std::string who = at + " thread " + std::to_string(tid);
                expect(ea[tid].vmask == eb[tid].vmask, who + " vmask");
                if (frl_occ_form<MODE, W, NS>()) {
                    expect(ea[tid].occ == eb[tid].occ, who + " occ");
                } else {
                    expect(ea[tid].apk0 == eb[tid].apk0 && ea[tid].apk1 == eb[tid].apk1, who + " apk");
                    expect(ea[tid].a_first == eb[tid].a_first && ea[tid].a_last == eb[tid].a_last, who + " a_first / a_last");
                }
            }
        }
    }
}

// canonical 31-mers, window w, over reads [first_read, end_read) of a batch of n_bases bases
static void frl_case(const std::vector<uint8_t>& t, int64_t n_bases, int read_len, int w, int64_t first_read, int64_t end_read, const std::string& name)
{
    const Packed k = pack(t, n_bases);
    ScanParams p{};
    p.bases = t.data();
    p.n_bases = n_bases;
    const int64_t first = first_read * read_len, end = end_read * read_len;
    plan_scan(MODE_MINIMIZER, first, end, w, p);
    if (!plan_scan_frl_for(MODE_MINIMIZER, first, end, n_bases, read_len, 31, w, true, p)) {
        expect(false, name + ": the read-tiled plan does not apply");
        return;
    }
    p.unit = 31;
    p.w = w;
    p.canonical = 1;
    p.seed = 42;
    p.direct_codes = 1;
    expect(packed_covers(p), name + ": the plan leaves the packed copy");
    p.codes_packed = k.codes();
    p.chunk_bad = k.bad();
    if (w == 11 && p.ns == 14) compare_tiles<11, 14>(p, name);
    else if (w == 11 && p.ns == 15) compare_tiles<11, 15>(p, name);
    else if (w == 11 && p.ns == 16) compare_tiles<11, 16>(p, name);
    else if (w == 5 && p.ns == 16) compare_tiles<5, 16>(p, name);
    else expect(false, name + ": no instantiation for ns = " + std::to_string(p.ns));
}

int main()
{
    for (int read_len : {100, 150, 151}) {
        for (int w : {11, 5}) {
            ScanParams g{};
            const int64_t probe = 4096 * (int64_t)read_len;
            if (!plan_scan_frl_for(MODE_MINIMIZER, 0, probe, probe, read_len, 31, w, true, g)) {
                expect(false, "no read-tiled plan for L = " + std::to_string(read_len));
                continue;
            }
            const int64_t rpt = NWAVE * g.rpw;            // reads per tile
            const int64_t n_reads = 5 * rpt + 3, n = n_reads * read_len;  // five full tiles and three reads
            const std::string L = "L=" + std::to_string(read_len) + " w=" + std::to_string(w);
            const std::vector<uint8_t> clean = random_text((size_t)n);
            frl_case(clean, n, read_len, w, 0, n_reads, L + " no N");  // starts at chunk 0, ends with the batch's last tile
            for (int64_t r0 : {1, 3, 8}) frl_case(clean, n, read_len, w, r0, n_reads, L + " no N, from read " + std::to_string(r0));
            frl_case(clean, n, read_len, w, 0, 2 * rpt, L + " no N, two tiles that end inside the batch");
            frl_case(clean, n, read_len, w, rpt + 5, 3 * rpt + 6, L + " no N, inner reads");
            // N: in tile 2 only; as the last base of tile 0 and the first of tile 1; behind tile 1's last read where tile 1 still stages it
            std::vector<uint8_t> one = clean;
            one[(size_t)(2 * g.stride + g.stride / 2)] = 'N';
            frl_case(one, n, read_len, w, 0, n_reads, L + " N in tile 2");
            frl_case(one, n, read_len, w, 3, n_reads, L + " N in tile 2, from read 3");
            std::vector<uint8_t> edge = clean;
            edge[(size_t)(g.stride - 1)] = 'N';
            edge[(size_t)g.stride] = 'n';
            frl_case(edge, n, read_len, w, 0, n_reads, L + " N on the border of tiles 0 and 1");
            std::vector<uint8_t> behind = clean;
            behind[(size_t)(2 * g.stride + 20)] = 'N';  // tile 2's second chunk or so: inside tile 1's staged span
            frl_case(behind, n, read_len, w, 0, n_reads, L + " N just behind tile 1");
            std::vector<uint8_t> far = clean;
            far[(size_t)(2 * g.stride + 16 * 40)] = 'N';  // outside tile 1's staged chunks, perhaps inside its last covering word
            frl_case(far, n, read_len, w, 0, n_reads, L + " N 40 chunks behind tile 1");
            std::vector<uint8_t> many = clean;
            for (int i = 0; i < 6; ++i) many[rnd() % many.size()] = (uint8_t)"NnRY-*. "[rnd() & 7];
            frl_case(many, n, read_len, w, 0, n_reads, L + " six random bad bases");
            frl_case(many, n, read_len, w, 8, n_reads - 1, L + " six random bad bases, reads 8 .. last but one");
        }
    }
    std::printf("emu_direct: %d tiles, %d clean, %d staged (%d of them for a neighbour's chunk), %d mismatches\n", g_tiles, g_clean, g_staged, g_neighbour, g_fail);
    if (g_clean == 0 || g_staged == 0) {
        std::fprintf(stderr, "one of the two paths never ran\n");
        return 1;
    }
    return g_fail ? 1 : 0;
}
