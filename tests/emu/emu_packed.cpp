// TEST INFRASTRUCTURE: staging a tile from a batch's packed copy (ScanParams::codes_packed, chunk_bad) against staging it from
// the ASCII bases, thread by thread on the host.  A stand-alone program: tests/test_emu_packed.py builds it with
// -fsanitize=address,undefined and runs it.
//
// The packed copy is made with pack_chunk, the function pack_codes_kernel calls for every chunk.  phase_load_frl and phase_load then
// stage every tile of a scan twice, with and without the two pointers, and the staged codes, flags and (read-tiled) wave_bad must be
// identical.  The base buffers hold exactly n_bases bytes, so a load past the batch's end is an AddressSanitizer report.
#define BL_CPU_EMU 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../biolib_amd/csrc/bl_scan_frl.hpp"

using namespace bl;

static int g_fail = 0, g_tiles = 0, g_fast = 0, g_slow = 0;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
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

// what make_packed_codes / pack_codes_kernel leave on the device: packed_total chunks, the guard chunks on either side included
struct Packed {
    std::vector<uint32_t> words, bits;
    const uint32_t* codes() const { return words.data() + PACK_LEAD; }
    const uint32_t* bad() const { return bits.data() + PACK_LEAD / 32; }
};

static Packed pack(const std::vector<uint8_t>& t, int64_t n_bases)
{
    Packed k;
    const int64_t total = packed_total(n_bases);
    k.words.assign((size_t)total, 0xA5A5A5A5u);
    k.bits.assign((size_t)(total / 32), 0);
    for (int64_t i = 0; i < total; ++i) {  // thread i of pack_codes_kernel
        uint32_t code;
        if (pack_chunk(t.data(), n_bases, i - PACK_LEAD, code)) k.bits[(size_t)(i >> 5)] |= 1u << (i & 31);
        k.words[(size_t)i] = code;
    }
    return k;
}

static void expect(bool ok, const std::string& what)
{
    if (ok) return;
    if (++g_fail <= 20) std::fprintf(stderr, "MISMATCH %s\n", what.c_str());
}

// both stagings of every tile of the plan in p (p.bases, p.n_bases, p.start_bits set; the packed pointers not)
template <int MODE, int W>
static void compare_tiles(const ScanParams& p, const Packed& k, const std::string& name)
{
    ScanParams pp = p;
    pp.codes_packed = k.codes();
    pp.chunk_bad = k.bad();
    expect(packed_covers(p), name + ": the plan leaves the packed copy");
    auto* a = new TileShared<MODE, W>();
    auto* b = new TileShared<MODE, W>();
    for (int tile = 0; tile < p.n_tiles; ++tile) {
        std::memset(a, 0xA5, sizeof(*a));
        std::memset(b, 0xA5, sizeof(*b));
        const int64_t q0 = p.frl ? tile_q0(p, (uint32_t)tile) : p.origin + (int64_t)tile * p.stride;
        for (int tid = 0; tid < TPB; ++tid) {
            if (p.frl) {
                phase_load_frl<MODE, W>(p, *a, tid, q0);
                phase_load_frl<MODE, W, true>(pp, *b, tid, q0);  // what the PACKED twin of the kernel runs
            } else {
                phase_load<MODE, W>(p, *a, tid, q0);
                phase_load<MODE, W, true>(pp, *b, tid, q0);
            }
        }
        const int needed = staged_chunks(p);
        const std::string at = name + " tile " + std::to_string(tile);
        for (int c = 0; c < needed; ++c) {
            expect(a->codes[c] == b->codes[c], at + " codes[" + std::to_string(c) + "]");
            expect(a->flags[c] == b->flags[c], at + " flags[" + std::to_string(c) + "]");
            // which path the packed staging took.  wave_any is the thread's own predicate in the emulation; on the device a good chunk also
            // takes the ASCII path when another lane of its wave met a bad one, which stages what `a` holds for it: any mix of the two
            // paths over a wave's chunks is covered by comparing every chunk of the two stagings
            uint32_t code;
            if (packed_chunk(pp, q0 + 16 * (int64_t)c, code)) ++g_slow;
            else ++g_fast;
        }
        if (p.frl)
            for (int wv = 0; wv < NWAVE; ++wv) expect(a->wave_bad[wv] == b->wave_bad[wv], at + " wave_bad[" + std::to_string(wv) + "]");
        ++g_tiles;
    }
    delete a;
    delete b;
}

// read-tiled: reads of one length, the headline scan (canonical 31-mers, window 11), over reads [first_read, end_read)
static void frl_case(const std::vector<uint8_t>& t, int64_t n_bases, int read_len, int64_t first_read, int64_t end_read, const std::string& name)
{
    const Packed k = pack(t, n_bases);
    ScanParams p{};
    p.bases = t.data();
    p.n_bases = n_bases;
    const int64_t first = first_read * read_len, end = end_read * read_len;
    plan_scan(MODE_MINIMIZER, first, end, 11, p);
    if (!plan_scan_frl_for(MODE_MINIMIZER, first, end, n_bases, read_len, 31, 11, true, p)) {
        expect(false, name + ": the read-tiled plan does not apply");
        return;
    }
    p.unit = 31;
    p.w = 11;
    p.canonical = 1;
    compare_tiles<MODE_MINIMIZER, 11>(p, k, name);
}

// position-tiled: the whole batch, minimizers (31, 11); starts: the batch's sequence starts (empty: one sequence)
static void pos_case(const std::vector<uint8_t>& t, int64_t n_bases, const std::vector<int64_t>& starts, const std::string& name)
{
    const Packed k = pack(t, n_bases);
    std::vector<uint32_t> bits((size_t)((n_bases + 31) / 32 + 4), 0);
    for (int64_t s : starts) bits[(size_t)(s >> 5)] |= 1u << (s & 31);
    ScanParams p{};
    p.bases = t.data();
    p.n_bases = n_bases;
    p.start_bits = starts.empty() ? nullptr : bits.data();
    plan_scan(MODE_MINIMIZER, 0, n_bases, 11, p);
    p.unit = 31;
    p.w = 11;
    p.canonical = 1;
    compare_tiles<MODE_MINIMIZER, 11>(p, k, name);
    // the syncmer plan starts its first tile at the range's first base, not one chunk before it
    ScanParams q = p;
    plan_scan(MODE_SYNCMER, 0, n_bases, 21, q);
    q.unit = 11;
    q.w = 21;
    compare_tiles<MODE_SYNCMER, 21>(q, k, name + " (syncmer plan)");
}

// N as the first and as the last base of a chunk, in the chunk that straddles the border between tiles 0 and 1 of the range that starts at
// `first` (stride bases per tile), and in the last read
static void place_ns(std::vector<uint8_t>& t, int64_t n_bases, int64_t first, int64_t stride, int read_len)
{
    auto put = [&](int64_t q) { if (q >= 0 && q < n_bases) t[(size_t)q] = 'N'; };
    put(first + 16 * 20);            // first base of a chunk
    put(first + 16 * 40 + 15);       // last base of a chunk
    put(((first + 700) | 15));       // ... whatever the range's alignment
    put(((first + 900) & ~15LL));
    put(first + stride - 1);         // the chunk that holds the tile border
    put(first + 2 * stride);
    put(n_bases - 1 - read_len / 2); // the last read
    put(n_bases - 1);
}

int main()
{
    // ---- read-tiled, 150 bp: 100 reads = three tiles of 32 reads and four reads
    for (int read_len : {150, 151}) {
        const int64_t n_reads = read_len == 150 ? 100 : 67, n = n_reads * read_len;
        const int64_t stride = 4 * 8 * read_len;
        const std::string L = "frl L=" + std::to_string(read_len);
        std::vector<uint8_t> clean = random_text((size_t)n);
        frl_case(clean, n, read_len, 0, n_reads, L + " clean");
        frl_case(clean, n, read_len, 1, n_reads, L + " clean, from read 1");  // 151: the range starts inside a chunk
        frl_case(clean, n, read_len, 33, 35, L + " clean, two reads");
        std::vector<uint8_t> dirty = clean;
        place_ns(dirty, n, 0, stride, read_len);
        frl_case(dirty, n, read_len, 0, n_reads, L + " N");
        dirty = clean;
        place_ns(dirty, n, read_len, stride, read_len);
        frl_case(dirty, n, read_len, 1, n_reads, L + " N, from read 1");
        std::vector<uint8_t> mixed = clean;
        for (size_t i = 0; i < mixed.size(); ++i) {
            const uint32_t r = rnd() % 8;
            if (r == 0) mixed[i] = (uint8_t)(mixed[i] | 0x20);                      // lower case
            else if (r == 1 && mixed[i] == 'T') mixed[i] = (rnd() & 1) ? 'U' : 'u';
        }
        frl_case(mixed, n, read_len, 0, n_reads, L + " lower case and U");
        for (int i = 0; i < 40; ++i) mixed[rnd() % mixed.size()] = (uint8_t)"NnRY-*. "[rnd() & 7];
        frl_case(mixed, n, read_len, 0, n_reads, L + " lower case, U and others");
        frl_case(random_text((size_t)read_len), read_len, read_len, 0, 1, L + " one read");
    }
    // ---- position-tiled
    for (int64_t n : {(int64_t)1, (int64_t)10, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)(16 * 750), (int64_t)(16 * 750 + 7)}) {
        const std::string name = "pos n=" + std::to_string(n);
        std::vector<uint8_t> t = random_text((size_t)n);
        pos_case(t, n, {}, name + " clean");
        std::vector<int64_t> starts;  // ragged reads of 100 .. 151 bases
        for (int64_t q = 0; q < n; q += 100 + (int64_t)(rnd() % 52)) starts.push_back(q);
        pos_case(t, n, starts, name + " ragged reads");
        const int64_t stride = 4 * (64 * 16 - 16);
        place_ns(t, n, 0, stride, 120);
        for (int64_t q = stride - 20; q < stride + 20 && q < n; ++q) t[(size_t)q] = 'N';  // N's across the border of tiles 0 and 1
        pos_case(t, n, {}, name + " N");
        pos_case(t, n, starts, name + " N, ragged reads");
        for (size_t i = 0; i < t.size(); i += 3) t[i] = t[i] == 'T' ? 'u' : (uint8_t)(t[i] | 0x20);
        pos_case(t, n, starts, name + " lower case and U");
    }
    std::printf("emu_packed: %d tiles, %d chunks staged from the packed copy, %d through the ASCII path, %d mismatches\n", g_tiles, g_fast, g_slow, g_fail);
    if (g_fast == 0 || g_slow == 0) {
        std::fprintf(stderr, "one of the two staging paths never ran\n");
        return 1;
    }
    return g_fail ? 1 : 0;
}
