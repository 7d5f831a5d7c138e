// CPU emulation of the unitig links and the GFA writer (biolib_amd/csrc/bl_links_core.hpp, bl_gfa_core.hpp), built with -DBL_CPU_EMU under
// AddressSanitizer / UBSan by tests/test_emu_links.py.  Every pass of bl_unitig_links and bl_unitigs_format_gfa runs lane by lane in the
// order the host driver of bl_links.hip launches them, for both flag values: the end keys, the end search with its parked words, the sum
// of the degrees, the emission at capacities n_links, n_links - 1 and 0, then the line lengths, their sum and the write, wave by wave as
// the kernel's ballots and shuffles see it.  The table, its prefix index, the nodes, the offsets, the bases and every intermediate and
// result array are heap arrays of EXACTLY the needed lengths, so that an access one element outside is a sanitizer report.  Every byte
// the write produced is checked against gfa_byte(position).
// usage: emu_links input.bin out_prefix [sweep | garbage]   (sweep: the text again with every prefix length 0 .. 15; garbage: nodes, offsets
//   and link words are overwritten with anything first — trusted for content, not for safety)
//   input.bin: uint64 key_words, key_bits, n, k, option ("table_prefix_bits" forced), n_unitigs, n_bases, first_number, header, prefix_len,
//   16 bytes of prefix, then the sorted keys, n nodes (8 bytes), n_unitigs + 1 offsets, n_unitigs count sums and the bases
//   prints "refused <reason>", else for flags f = 0, 1 the lines  links<f> / offsets<f> / stats<f> / chunks<f>  and "residues <mask>";
//   writes the text of flags f to <out_prefix><f>.gfa
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../biolib_amd/csrc/bl_gfa_core.hpp"
#include "../../biolib_amd/csrc/bl_links_core.hpp"

typedef unsigned long long ull;

#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            std::printf("FAILED: ");       \
            std::printf(__VA_ARGS__);      \
            std::printf("\n");             \
            return false;                  \
        }                                  \
    } while (0)

struct Input {
    blgr::TableView t;
    uint32_t k;
    const bllnk::Node* nodes;     // [n]
    const uint64_t* offsets;      // [n_unitigs + 1]
    const uint64_t* sums;         // [n_unitigs]
    const uint8_t* bases;         // [n_bases]
    uint64_t n_unitigs, n_bases, first_number;
    uint32_t header;
    std::string prefix;
    bool garbage;                 // nodes, offsets and link words hold anything: only the sanitizers and gfa_byte judge
};

struct Links {
    std::vector<uint64_t> offsets;  // 2 * n_unitigs + 1
    std::unique_ptr<bllnk::Link[]> records;
    uint64_t n_links = 0;
    ull stats[5] = {0, 0, 0, 0, 0};
};

// bl_unitig_links as the driver runs it
template <int W>
static bool run_links(const Input& in, uint32_t flags, Links& out)
{
    using namespace bllnk;
    const uint64_t n_ends = 2 * in.n_unitigs;
    std::unique_ptr<uint32_t[]> end_key(new uint32_t[n_ends]);
    std::memset(end_key.get(), 0xFF, n_ends * sizeof(uint32_t));
    for (uint32_t i = 0; i < in.t.n; ++i) end_key_thread(in.nodes, in.offsets, in.n_unitigs, in.k, i, end_key.get());
    std::unique_ptr<uint64_t[]> degree(new uint64_t[n_ends + 1]);
    std::unique_ptr<Parked[]> parked(new Parked[n_ends]);
    out.stats[0] = n_ends;
    for (uint64_t e = 0; e < n_ends; ++e) {
        CHECK(in.garbage || end_key[e] != END_NONE, "end %llu has no key", (ull)e);
        const EndStats st = end_search<W>(in.t, in.k, in.nodes, in.n_unitigs, end_key.get(), flags, (uint32_t)e, parked[e]);
        CHECK(st.kept <= st.degree && st.degree <= 4, "end %llu: degree %u kept %u", (ull)e, st.degree, st.kept);
        degree[e] = st.kept;
        out.stats[2] += st.self_reverse;
        out.stats[3] += st.degree == 0;
        out.stats[4] += st.degree >= 2;
    }
    degree[n_ends] = 0;
    out.offsets.assign(n_ends + 1, 0);
    uint64_t total = 0;
    for (uint64_t e = 0; e <= n_ends; ++e) {
        out.offsets[e] = total;
        total += degree[e];
    }
    out.n_links = out.stats[1] = total;
    // capacities n_links - 1 and 0: the driver answers BL_ERR_CAPACITY in front of the emission and the array keeps its fill;
    // capacity n_links: an array of exactly that length takes every record
    for (uint64_t capacity : {total ? total - 1 : 0, (uint64_t)0, total}) {
        std::unique_ptr<Link[]> records(new Link[capacity]);
        std::memset(static_cast<void*>(records.get()), 0xA5, capacity * sizeof(Link));
        if (capacity < total) {
            for (uint64_t r = 0; r < capacity; ++r) CHECK(records[r].from == 0xA5A5A5A5u, "capacity %llu: record %llu written", (ull)capacity, (ull)r);
            continue;
        }
        for (uint64_t e = 0; e < n_ends; ++e) emit_thread(out.offsets.data(), parked.get(), total, (uint32_t)e, records.get());
        for (uint64_t r = 0; r < total; ++r) CHECK(records[r].from != 0xA5A5A5A5u, "record %llu not written", (ull)r);
        if (in.garbage)  // (the text takes any link words)
            for (uint64_t r = 0; r < total; r += 3) records[r].from = records[r].to = 0xFFFFFFFFu - (uint32_t)r;
        out.records = std::move(records);
    }
    return true;
}

// bl_unitigs_format_gfa as the driver and the kernel run it; text: exactly `total` bytes
static bool run_gfa(const Input& in, const Links& lk, const std::string& prefix, std::vector<uint8_t>& text, ull* chunks, uint64_t* boundary)
{
    using namespace blgfa;
    GfaParams p{};
    p.bases = in.bases;
    p.n_bases = in.n_bases;
    p.offsets = in.offsets;
    p.n_unitigs = in.n_unitigs;
    p.sums = in.sums;
    p.links = reinterpret_cast<const LinkWords*>(lk.records.get());
    p.n_links = lk.n_links;
    p.n_head = in.header ? 1u : 0u;
    p.overlap = in.k - 1;
    p.overlap_digits = p.overlap >= 10 ? 2u : 1u;
    for (size_t i = 0; i < prefix.size(); ++i) p.prefix[i >> 3] |= (uint64_t)(uint8_t)prefix[i] << (8 * (i & 7));
    p.prefix_len = (uint32_t)prefix.size();
    p.first_number = in.first_number;
    p.n_lines = p.n_head + p.n_unitigs + p.n_links;
    text.clear();
    *boundary = 0;
    if (p.n_lines == 0) return true;
    std::unique_ptr<uint64_t[]> line_len(new uint64_t[p.n_lines + 1]), line_off(new uint64_t[p.n_lines + 1]);
    p.line_len = line_len.get();
    for (uint64_t i = 0; i <= p.n_lines; ++i) line_length(p, i);
    uint64_t total = 0;
    for (uint64_t i = 0; i <= p.n_lines; ++i) {
        CHECK(i == p.n_lines || line_len[i] > 0, "line %llu is empty", (ull)i);
        line_off[i] = total;
        total += line_len[i];
    }
    p.line_off = line_off.get();
    p.total = total;
    *boundary = line_off[p.n_head + p.n_unitigs];
    std::unique_ptr<uint8_t[]> out(new uint8_t[total]);
    std::memset(out.get(), '?', total);
    p.out = out.get();
    const uint64_t waves = (total + WAVE_BYTES - 1) / WAVE_BYTES;
    for (uint64_t wave = 0; wave < waves; ++wave) {
        const uint64_t x_first = blsel::wave_first_byte(wave);
        uint64_t lo = 0, e = p.n_lines;
        while (e - lo > 1) {
            uint64_t below = 0;
            bool open = true;
            for (int lane = 0; lane < 64; ++lane) {
                const bool pred = blsel::kary_probe(p.line_off, lo, e, lane, x_first);
                CHECK(open || !pred, "wave %llu: the probes at or below the byte are no prefix of the lanes", (ull)wave);
                open = pred;
                below += pred ? 1 : 0;
            }
            blsel::kary_narrow(lo, e, below);
        }
        CHECK(lo == blsel::seq_of(p.line_off, x_first, 0, p.n_lines - 1), "wave %llu: the 64-ary search differs from the bisection", (ull)wave);
        const uint64_t x_last = wave_last_byte(p, wave);
        uint64_t o[64];  // the lanes' registers
        int inside = 0;
        for (int lane = 0; lane < 64; ++lane) {
            o[lane] = lane_offset(p, lo, lane);
            inside += o[lane] <= x_last ? 1 : 0;
        }
        const uint64_t o_lo = p.line_off[lo];
        const bool in_registers = inside < 64;
        const uint64_t hi = in_registers ? lo + (uint64_t)inside : blsel::seq_of(p.line_off, x_last, lo + 64, p.n_lines - 1);
        for (int u = 0; u < CHUNKS_PER_LANE; ++u)
            for (int lane = 0; lane < 64; ++lane) {
                const uint64_t x0 = blsel::chunk_first_byte(wave, u, lane);
                if (x0 >= total) continue;
                LineAt s;
                if (in_registers) {
                    uint32_t cnt = 0;
                    for (uint32_t step = 32; step >= 1; step >>= 1) blsel::count_step(cnt, step, o[(cnt + step - 1) & 63], x0);  // (a shuffle's index wraps)
                    CHECK(cnt <= (uint32_t)inside, "wave %llu: line %u of the wave's %d", (ull)wave, cnt, inside);
                    s.j = lo + cnt;
                    s.begin = cnt ? o[cnt - 1] : o_lo;
                    s.end = o[cnt & 63];
                } else {
                    s = line_from_memory(p, x0, lo, hi);
                }
                CHECK(s.j == blsel::seq_of(p.line_off, x0, 0, p.n_lines - 1) && s.begin == p.line_off[s.j] && s.end == p.line_off[s.j + 1],
                      "chunk at %llu: line %llu", (ull)x0, (ull)s.j);
                uint32_t w[4];
                uint64_t vsrc = 0;
                bool whole = false;
                if (x0 + CHUNK <= s.end) whole = chunk_window(p, s.j, x0 - s.begin, vsrc);
                if (whole) {
                    uint32_t v[5];
                    blsel::window_load(p.bases, vsrc, v);
                    blsel::window_shift(v, vsrc, w);
                    ++chunks[0];
                } else {
                    gfa_pieces(p, x0, s, w);
                    ++chunks[1];
                }
                blfmt::store_chunk(p.out, total, x0, w);
            }
    }
    for (uint64_t x = 0; x < total; ++x) CHECK(out[x] == gfa_byte(p, x), "byte %llu is %02x, gfa_byte says %02x", (ull)x, out[x], gfa_byte(p, x));
    text.assign(out.get(), out.get() + total);
    return true;
}

template <int W>
static int run(const Input& in, const char* out_prefix, bool sweep)
{
    uint32_t residues = 0;
    for (uint32_t flags = 0; flags < 2; ++flags) {
        Links lk;
        if (!run_links<W>(in, flags, lk)) return 1;
        std::printf("links%u", flags);
        for (uint64_t r = 0; r < lk.n_links; ++r) std::printf(" %u %u", lk.records[r].from, lk.records[r].to);
        std::printf("\noffsets%u", flags);
        for (uint64_t v : lk.offsets) std::printf(" %llu", (ull)v);
        std::printf("\nstats%u", flags);
        for (int j = 0; j < 5; ++j) std::printf(" %llu", lk.stats[j]);
        std::vector<uint8_t> text;
        ull chunks[2] = {0, 0};
        uint64_t boundary = 0;
        if (!run_gfa(in, lk, in.prefix, text, chunks, &boundary)) return 1;
        std::printf("\nchunks%u %llu %llu\n", flags, chunks[0], chunks[1]);
        FILE* f = std::fopen((std::string(out_prefix) + std::to_string(flags) + ".gfa").c_str(), "wb");
        if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size() || std::fclose(f) != 0) return 2;
        // every prefix length moves the place where the segment lines end and the link lines begin, and the text's end
        if (sweep)
            for (size_t len = 0; len < 16; ++len) {
                std::vector<uint8_t> other;
                ull ignored[2] = {0, 0};
                if (!run_gfa(in, lk, std::string("abcdefghijklmno").substr(0, len), other, ignored, &boundary)) return 1;
                if (lk.n_links) residues |= 1u << (boundary & 15);
            }
    }
    std::printf("residues %u\n", residues);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s input.bin out_prefix\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[10];
    char prefix[16];
    if (std::fread(head, 8, 10, f) != 10 || std::fread(prefix, 1, 16, f) != 16) return 2;
    const uint32_t kw = (uint32_t)head[0], key_bits = (uint32_t)head[1], n = (uint32_t)head[2], k = (uint32_t)head[3];
    int why = blgr::refuse(k, kw, key_bits, head[2]);
    if (!why) why = bllnk::refuse(k, 0, head[2], head[5]);
    if (!why && blgfa::refuse(0, k, (int)head[9], 0)) why = 8;
    if (why) { std::printf("refused %d\n", why); return 0; }
    const uint64_t n_unitigs = head[5], n_bases = head[6];
    std::unique_ptr<uint64_t[]> keys(new uint64_t[(size_t)n * kw]);
    std::unique_ptr<bllnk::Node[]> nodes(new bllnk::Node[n]);
    std::unique_ptr<uint64_t[]> offsets(new uint64_t[n_unitigs + 1]), sums(new uint64_t[n_unitigs]);
    // (blsel::window_load reads aligned dwords: the bases start 16-byte aligned as a batch's do)
    void* aligned = nullptr;
    if (n_bases && posix_memalign(&aligned, 16, n_bases) != 0) return 2;  // (ASan keeps the exact length)
    uint8_t* bases = static_cast<uint8_t*>(aligned);
    if (n && (std::fread(keys.get(), 8 * kw, n, f) != n || std::fread(nodes.get(), 8, n, f) != n)) return 2;
    if (std::fread(offsets.get(), 8, n_unitigs + 1, f) != n_unitigs + 1) return 2;
    if (n_unitigs && std::fread(sums.get(), 8, n_unitigs, f) != n_unitigs) return 2;
    if (n_bases && std::fread(bases, 1, n_bases, f) != n_bases) return 2;
    std::fclose(f);
    Input in{};
    in.t.keys = keys.get();
    in.t.counts = nullptr;
    in.t.n = n;
    in.t.key_words = kw;
    in.t.key_bits = key_bits;
    in.t.prefix_bits = bllk::choose_prefix_bits((int)head[4], n, key_bits);
    std::unique_ptr<uint32_t[]> index(new uint32_t[((size_t)1 << in.t.prefix_bits) + 1]);
    in.t.index = index.get();
    for (uint32_t j = 0; j <= (1u << in.t.prefix_bits); ++j) index[j] = bllk::index_entry(in.t, j);
    in.k = k;
    in.nodes = nodes.get();
    in.offsets = offsets.get();
    in.sums = sums.get();
    in.bases = bases;
    in.n_unitigs = n_unitigs;
    in.n_bases = n_bases;
    in.first_number = head[7];
    in.header = (uint32_t)head[8];
    in.prefix.assign(prefix, (size_t)head[9]);
    in.garbage = argc > 3 && std::strcmp(argv[3], "garbage") == 0;
    if (in.garbage) {  // unitig numbers at, above and far above n_unitigs, any rank and flip, offsets in any order and beyond the bases
        uint64_t x = 0x9E3779B97F4A7C15ull ^ head[2];
        auto next = [&x]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return x >> 24; };
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t r = next();
            nodes[i].unitig = (r & 7) == 0 ? 0xFFFFFFFFu : (uint32_t)(next() % (n_unitigs + 3));
            nodes[i].rank_flip = (r & 8) ? (uint32_t)next() : (uint32_t)(next() & 7);
        }
        for (uint64_t u = 0; u <= n_unitigs; ++u) offsets[u] = (next() & 3) == 0 ? ~0ull - next() % 5 : next() % (n_bases + 5);
    }
    const bool sweep = argc > 3 && !in.garbage;
    const int rc = kw == 2 ? run<2>(in, argv[2], sweep) : run<1>(in, argv[2], sweep);
    std::free(bases);
    return rc;
}
