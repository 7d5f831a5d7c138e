// CPU emulation of the two intersection kernels for 16-byte keys (biolib_amd/csrc/bl_setops128_core.hpp), built with -DBL_CPU_EMU under
// AddressSanitizer / UBSan by tests/test_emu_setops128.py.  The partition step and the tile body run lane by lane for every tile; what
// stands for LDS is a heap array of EXACTLY the staged length (la + lbx keys), and the global arrays are exactly na and nb keys long, so
// that any index outside a range is a sanitizer report.  The count is compared with a plain two-finger walk in this program.
// usage: emu_setops128 input.bin [nocheck]
//   input.bin: uint64 na, uint64 nb, then na + nb keys of two uint64 words (low, high): A, then B
//   prints "merge <count> search <count> walk <count>"; exit status 1 when the three differ (never with nocheck: inputs with duplicates,
//   run for the sanitizers only)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../biolib_amd/csrc/bl_setops128_core.hpp"

using bl128s::Key;
typedef unsigned long long ull;

static ull walk(const std::vector<Key>& a, const std::vector<Key>& b)
{
    size_t i = 0, j = 0;
    ull both = 0;
    while (i < a.size() && j < b.size()) {
        const unsigned __int128 x = ((unsigned __int128)a[i].hi << 64) | a[i].lo, y = ((unsigned __int128)b[j].hi << 64) | b[j].lo;
        if (x < y) ++i;
        else if (y < x) ++j;
        else { ++i; ++j; ++both; }
    }
    return both;
}

static ull merge_kernels(const std::vector<Key>& a, const std::vector<Key>& b)
{
    const ull na = a.size(), nb = b.size(), total = na + nb;
    const ull n_tiles = (total + bl128s::TILE - 1) / bl128s::TILE;
    // merge_partition_kernel: one thread per tile boundary
    std::vector<ull> splits(n_tiles + 1);
    for (ull t = 0; t <= n_tiles; ++t) {
        const ull d = t * (ull)bl128s::TILE < total ? t * (ull)bl128s::TILE : total;
        splits[t] = bl128s::diag_split<ull>(a.data(), na, b.data(), nb, d);
    }
    // merge_tile_kernel: one workgroup per tile
    ull sum = 0;
    for (ull t = 0; t < n_tiles; ++t) {
        const bl128s::TileRange r = bl128s::tile_range(splits.data(), t, na, nb);
        if (r.la + r.lbx > (uint32_t)bl128s::LDS_KEYS) { std::printf("tile %llu stages %u keys\n", t, r.la + r.lbx); return ~0ull; }
        std::vector<Key> lds(r.la + r.lbx);
        for (int tid = 0; tid < bl128s::TPB; ++tid) {
            for (uint32_t x = tid; x < r.la; x += bl128s::TPB) lds[x] = a.at(r.a0 + x);
            for (uint32_t x = tid; x < r.lbx; x += bl128s::TPB) lds[r.la + x] = b.at(r.b0 + x);
        }
        for (int tid = 0; tid < bl128s::TPB; ++tid) sum += bl128s::tile_thread_count(lds.data(), r.la, lds.data() + r.la, r.lb, r.lbx, (uint32_t)tid);
    }
    return sum;
}

static ull search_kernel(const std::vector<Key>& a, const std::vector<Key>& b)
{
    const std::vector<Key>& x = a.size() <= b.size() ? a : b;
    const std::vector<Key>& y = a.size() <= b.size() ? b : a;
    ull sum = 0;
    if (x.empty() || y.empty()) return 0;
    for (size_t i = 0; i < x.size(); ++i) sum += bl128s::search_count(x[i], y.data(), y.size());
    return sum;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s input.bin [nocheck]\n", argv[0]); return 2; }
    const bool check = !(argc > 2 && std::strcmp(argv[2], "nocheck") == 0);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n[2];
    if (std::fread(n, 8, 2, f) != 2) return 2;
    std::vector<Key> a(n[0]), b(n[1]);
    if ((n[0] && std::fread(a.data(), 16, n[0], f) != n[0]) || (n[1] && std::fread(b.data(), 16, n[1], f) != n[1])) return 2;
    std::fclose(f);
    const ull m = merge_kernels(a, b), s = search_kernel(a, b), w = walk(a, b);
    std::printf("merge %llu search %llu walk %llu\n", m, s, w);
    return check && (m != w || s != w) ? 1 : 0;
}
