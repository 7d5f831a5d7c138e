// TEST INFRASTRUCTURE: the per-thread bodies of bl_scan_syncmers128 (biolib_amd/csrc/bl_syncmers128_core.hpp) run on the host — a
// workgroup's phases lane by lane, a host array standing in for LDS — under AddressSanitizer / UBSan, against a plain
// `unsigned __int128` evaluation of the rule written here.  Built and run by tests/test_emu_syncmers128.py, which compares the
// digests printed below with its own Python model.
//
//   emu_syncmers128 <batch file> <k> <s> <first> <n> <start_offset> <end_offset>
// batch file: u64 n_bases, u64 n_seqs, u64 offsets[n_seqs + 1], bases.  For canonical x drop_last it prints
//   sync <canonical> <drop_last> count xor_pos
// and exits non-zero on the first disagreement with the plain evaluation.
#define EMU_NAME "emu_syncmers128"
#include "emu128_common.hpp"
#include "../../biolib_amd/csrc/bl_syncmers128_core.hpp"

// per position: 1 + the extractor's offset of the (canonical) k-mer that starts there, 0 where none does
static std::vector<int> plain_offsets(const std::vector<uint8_t>& seq, const std::vector<uint64_t>& offs, int k, int s, uint32_t seed, bool canonical, bool drop_last)
{
    std::vector<int> r(seq.size(), 0);
    const u128 mask = k == 64 ? ~(u128)0 : (((u128)1 << (2 * k)) - 1);
    const u128 smask = ((u128)1 << (2 * s)) - 1;
    for (size_t q = 0; q + 1 < offs.size(); ++q) {
        u128 fwd = 0, rc = 0;
        int run = 0;
        for (uint64_t i = offs[q]; i < offs[q + 1]; ++i) {
            const int c = nt4(seq[i]);
            if (c > 3) { run = 0; continue; }
            fwd = ((fwd << 2) | (u128)c) & mask;
            rc = (rc >> 2) | ((u128)(3 ^ c) << (2 * (k - 1)));
            if (++run < k) continue;
            if (drop_last && i + 1 == offs[q + 1]) continue;
            const u128 v = canonical && rc < fwd ? rc : fwd;
            int best = 0;
            uint64_t best_hash = 0;
            for (int j = 0; j <= k - s; ++j) {  // x_j from the first base on; a strict '<' keeps the leftmost minimum
                const uint64_t h = plain_hash((v >> (2 * (k - s - j))) & smask, seed);
                if (j == 0 || h < best_hash) {
                    best_hash = h;
                    best = j;
                }
            }
            r[i + 1 - k] = 1 + best;
        }
    }
    return r;
}

static int scan_one(int argc, char** argv)
{
    CHECK(argc == 8, "usage: emu_syncmers128 <batch file> <k> <s> <first> <n> <start_offset> <end_offset>");
    const EmuBatch batch(argv[1]);
    const uint64_t n_bases = batch.n_bases;
    const std::vector<uint64_t>& offs = batch.offs;
    const std::vector<uint8_t>& seq = batch.seq;
    const int k = std::atoi(argv[2]), s = std::atoi(argv[3]);
    const uint64_t first = std::strtoull(argv[4], nullptr, 10), n_arg = std::strtoull(argv[5], nullptr, 10);
    const uint32_t soff = (uint32_t)std::strtoul(argv[6], nullptr, 10), eoff = (uint32_t)std::strtoul(argv[7], nullptr, 10);
    const uint64_t end = (n_arg == 0 || first + n_arg > n_bases) ? n_bases : first + n_arg;
    const uint32_t seed = 0x9e3779b9u;
    const uint64_t origin = 1000000007ull;
    CHECK(s >= 1 && s <= bl::MAX_SMER128 && k >= s && k <= bl::MAX_UNIT128 && first < end, "bad arguments");

    // the six-multiply form of the hash is bit-identical to the general one with a zero high word, and to the plain one
    uint64_t x = 0x243f6a8885a308d3ULL;
    static bool hash_checked;  // (once per run, not once per range of a list)
    for (int i = 0; i < 20000 && !hash_checked; ++i) {
        x = x * 6364136223846793005ULL + 1442695040888963407ULL;
        const uint64_t key = i < 70 ? (i < 64 ? 1ULL << i : (i == 64 ? 0 : ~0ULL >> (i - 65))) : x >> (x & 31);
        const uint32_t sd = i % 5 == 0 ? 0u : (i % 5 == 1 ? ~0u : (uint32_t)(x >> 17));
        const uint64_t got = bl::murmur64_u128_lo(key, sd);
        CHECK(got == bl::murmur64_u128(key, 0, sd) && got == plain_hash(key, sd), "murmur64_u128_lo(%llx, %x)", (unsigned long long)key, sd);
    }
    hash_checked = true;

    for (int canonical = 0; canonical < 2; ++canonical) {
        for (int drop_last = 0; drop_last < 2; ++drop_last) {
            static std::vector<int> plain[4];  // (a list of ranges: the batch, k and s stay, the plain evaluation runs once per strand and drop_last)
            static bool have[4];
            std::vector<int>& want = plain[2 * canonical + drop_last];
            if (!have[2 * canonical + drop_last]) want = plain_offsets(seq, offs, k, s, seed, canonical, drop_last);
            have[2 * canonical + drop_last] = true;
            bl::Sync128Params p{};
            batch.describe(p.km);
            p.km.pos_base = (int64_t)origin;
            bl::plan_kmers128((int64_t)first, (int64_t)end, p.km);
            p.km.seed = seed;
            p.km.canonical = canonical;
            p.km.drop_last = drop_last;
            bl::plan_syncmers128(k, s, soff, eoff, p);
            std::vector<uint32_t> codes(bl::NCHUNK_POS), flags(bl::NCHUNK_POS);
            std::vector<uint64_t> lds(bl::SYNC128_SLOTS);  // exact size: a read or write outside it is a finding
            std::vector<uint16_t> masks((size_t)p.km.n_tiles * bl::TPB);
            std::vector<unsigned long long> tile_counts(p.km.n_tiles), tile_base(p.km.n_tiles);
            std::vector<uint32_t> ok(bl::TPB), strand(bl::TPB), hit_fwd(bl::TPB), hit_rev(bl::TPB);
            unsigned long long xor_pos = 0;
            for (int tile = 0; tile < p.km.n_tiles; ++tile) {
                const int64_t q0 = p.km.origin + (int64_t)tile * bl::H;
                stage_all(p.km, codes, flags, q0);
                // every phase between two barriers runs for all lanes before the next one starts.  The array is zeroed first: a
                // window that read a word phase A did not write would find a minimum there
                std::fill(lds.begin(), lds.end(), 0);
                for (int tid = 0; tid < bl::TPB; ++tid) {
                    bl::sync128_hash_thread(p, codes.data(), lds.data(), tid, false);
                    ok[tid] = bl::sync128_ok_strand(p.km, codes.data(), flags.data(), tid, q0, strand[tid]);
                }
                for (int tid = 0; tid < bl::TPB; ++tid) hit_fwd[tid] = bl::sync128_window_thread<true>(lds.data(), tid, p.w, p.fwd_a, p.fwd_b);
                std::fill(hit_rev.begin(), hit_rev.end(), 0);
                if (canonical) {
                    std::fill(lds.begin(), lds.end(), 0);
                    for (int tid = 0; tid < bl::TPB; ++tid) bl::sync128_hash_thread(p, codes.data(), lds.data(), tid, true);
                    for (int tid = 0; tid < bl::TPB; ++tid) hit_rev[tid] = bl::sync128_window_thread<false>(lds.data(), tid, p.w, p.rev_a, p.rev_b);
                }
                unsigned long long cnt = 0;
                for (int tid = 0; tid < bl::TPB; ++tid) {
                    const uint32_t sel = bl::sync128_select(p.km, tid, q0, ok[tid], strand[tid], hit_fwd[tid], hit_rev[tid], xor_pos);
                    masks[(size_t)tile * bl::TPB + tid] = (uint16_t)sel;
                    cnt += (unsigned)__builtin_popcount(sel);
                    for (int t = 0; t < bl::S; ++t) {
                        const int64_t q = q0 + 16 * tid + t;
                        const bool in = q >= (int64_t)first && q < (int64_t)end && want[q] != 0;
                        const bool rec = in && ((uint32_t)(want[q] - 1) == soff || (uint32_t)(want[q] - 1) == eoff);
                        CHECK(((sel >> t) & 1u) == (rec ? 1u : 0u), "k=%d s=%d canonical=%d drop_last=%d position %lld: lane says %u, offset+1 = %d", k, s, canonical,
                              drop_last, (long long)q, (sel >> t) & 1u, q >= 0 && q < (int64_t)n_bases ? want[q] : -1);
                    }
                }
                tile_counts[tile] = cnt;
            }
            std::vector<uint64_t> w_pos;
            unsigned long long w_xor = 0;
            for (uint64_t q = first; q < end; ++q)
                if (want[q] && ((uint32_t)(want[q] - 1) == soff || (uint32_t)(want[q] - 1) == eoff)) {
                    w_pos.push_back(q + origin);
                    w_xor ^= q + origin;
                }
            unsigned long long total = 0;
            for (int tile = 0; tile < p.km.n_tiles; ++tile) {
                tile_base[tile] = total;
                total += tile_counts[tile];
            }
            CHECK(total == w_pos.size() && xor_pos == w_xor, "count / xor_pos k=%d s=%d: %llu, want %zu", k, s, total, w_pos.size());
            // the record pass: once with room for everything, once one record short
            for (int pass = 0; pass < 2; ++pass) {
                const uint64_t cap = pass == 0 ? total : (total ? total - 1 : 0);
                std::vector<uint64_t> rp(cap);  // exact size
                p.km.rec_pos = rp.data();
                p.km.capacity = cap;
                for (int tile = 0; tile < p.km.n_tiles; ++tile) {
                    const int64_t q0 = p.km.origin + (int64_t)tile * bl::H;
                    uint64_t at = tile_base[tile];
                    for (int tid = 0; tid < bl::TPB; ++tid) {
                        const uint32_t sel = masks[(size_t)tile * bl::TPB + tid];
                        bl::sync128_emit_thread(p.km, tid, q0, sel, at);
                        at += (unsigned)__builtin_popcount(sel);
                    }
                }
                for (uint64_t r = 0; r < cap; ++r) CHECK(rp[r] == w_pos[r], "record %llu k=%d s=%d", (unsigned long long)r, k, s);
            }
            std::printf("sync %d %d %llu %llu\n", canonical, drop_last, total, xor_pos);
        }
    }
    return 0;
}

// <first> = @FILE: every range of FILE in one run (emu128_common.hpp: run_ranges)
int main(int argc, char** argv) { return run_ranges(argc, argv, 4, scan_one); }
