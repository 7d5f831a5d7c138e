// TEST INFRASTRUCTURE: the per-thread bodies of the 128-bit k-mer scans (biolib_amd/csrc/bl_kmers128_core.hpp) run on the host, lane by
// lane and tile by tile, under AddressSanitizer / UBSan, against a plain `unsigned __int128` loop written here.  Built and run by
// tests/test_emu_kmers128.py, which compares the digests printed below with its own Python model.
//
//   emu_kmers128 <batch file> <k> <first> <n> <threshold>
// batch file: u64 n_bases, u64 n_seqs, u64 offsets[n_seqs + 1], bases.  For canonical x drop_last it prints
//   dense  <canonical> <drop_last> count xor_lo xor_hi xor_hash sum_hash
//   sample <canonical> <drop_last> count xor_lo xor_hi xor_hash xor_pos
// and exits non-zero on the first disagreement with the plain loop.
#define EMU_NAME "emu_kmers128"
#include "emu128_common.hpp"
#include "../../biolib_amd/csrc/bl_kmers128_core.hpp"

struct Plain {
    std::vector<uint64_t> lo, hi, hash;
    std::vector<uint8_t> valid;
};

static Plain plain_scan(const std::vector<uint8_t>& seq, const std::vector<uint64_t>& offs, int k, uint32_t seed, bool canonical, bool drop_last)
{
    const size_t n = seq.size();
    Plain r{std::vector<uint64_t>(n, 0), std::vector<uint64_t>(n, 0), std::vector<uint64_t>(n, 0), std::vector<uint8_t>(n, 0)};
    const u128 mask = k == 64 ? ~(u128)0 : (((u128)1 << (2 * k)) - 1);
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
            const uint64_t p = i + 1 - k;
            r.lo[p] = (uint64_t)v;
            r.hi[p] = (uint64_t)(v >> 64);
            r.hash[p] = plain_hash(v, seed);
            r.valid[p] = 1;
        }
    }
    return r;
}

static int scan_one(int argc, char** argv)
{
    CHECK(argc == 6, "usage: emu_kmers128 <batch file> <k> <first> <n> <threshold>");
    const EmuBatch batch(argv[1]);
    const uint64_t n_bases = batch.n_bases;
    const std::vector<uint64_t>& offs = batch.offs;
    const std::vector<uint8_t>& seq = batch.seq;
    const int k = std::atoi(argv[2]);
    const uint64_t first = std::strtoull(argv[3], nullptr, 10), n_arg = std::strtoull(argv[4], nullptr, 10);
    const uint64_t threshold = std::strtoull(argv[5], nullptr, 10);
    const uint64_t end = (n_arg == 0 || first + n_arg > n_bases) ? n_bases : first + n_arg;
    const uint32_t seed = 0x9e3779b9u;
    const uint64_t origin = 1000000007ull;
    CHECK(k >= 1 && k <= bl::MAX_UNIT128 && first < end, "bad arguments");

    for (int canonical = 0; canonical < 2; ++canonical) {
        for (int drop_last = 0; drop_last < 2; ++drop_last) {
            static Plain plain[4];  // (a list of ranges: the batch and k stay, the plain loop runs once per strand and drop_last)
            static bool have[4];
            Plain& want = plain[2 * canonical + drop_last];
            if (!have[2 * canonical + drop_last]) want = plain_scan(seq, offs, k, seed, canonical, drop_last);
            have[2 * canonical + drop_last] = true;
            bl::Kmer128Params p{};
            batch.describe(p);
            p.pos_base = (int64_t)origin;
            bl::plan_kmers128((int64_t)first, (int64_t)end, p);
            p.unit = k;
            p.seed = seed;
            p.canonical = canonical;
            p.drop_last = drop_last;
            p.hash_below = threshold;
            const size_t span = end - first;
            // exact-size outputs: a store outside [0, span) is a finding
            std::vector<bl::U64x2> out_value(span);
            std::vector<uint64_t> out_hash(span);
            std::vector<uint8_t> out_valid(span);
            std::vector<uint32_t> codes(bl::NCHUNK_POS), flags(bl::NCHUNK_POS);
            std::vector<uint16_t> masks((size_t)p.n_tiles * bl::TPB);
            std::vector<unsigned long long> tile_counts(p.n_tiles), tile_base(p.n_tiles);
            bl::Kmer128Acc dense{0, 0, 0, 0, 0}, digest_only{0, 0, 0, 0, 0}, samp{0, 0, 0, 0, 0};
            for (int tile = 0; tile < p.n_tiles; ++tile) {
                const int64_t q0 = p.origin + (int64_t)tile * bl::H;
                stage_all(p, codes, flags, q0);
                unsigned long long cnt = 0;
                for (int tid = 0; tid < bl::TPB; ++tid) {
                    p.out_value = reinterpret_cast<uint64_t*>(out_value.data());
                    p.out_hash = out_hash.data();
                    p.out_valid = out_valid.data();
                    bl::kmer128_dense_thread(p, codes.data(), flags.data(), tid, q0, dense);
                    p.out_value = nullptr;
                    p.out_hash = nullptr;
                    p.out_valid = nullptr;
                    bl::kmer128_dense_thread(p, codes.data(), flags.data(), tid, q0, digest_only);  // the path that stores nothing
                    const uint32_t sel = bl::kmer128_count_thread(p, codes.data(), flags.data(), tid, q0, samp);
                    masks[(size_t)tile * bl::TPB + tid] = (uint16_t)sel;
                    cnt += (unsigned)__builtin_popcount(sel);
                }
                tile_counts[tile] = cnt;
            }
            // dense: arrays and digest against the plain loop
            unsigned long long w_cnt = 0, w_lo = 0, w_hi = 0, w_h = 0, w_sum = 0;
            for (uint64_t q = first; q < end; ++q) {
                const size_t o = q - first;
                CHECK(out_valid[o] == want.valid[q] && out_value[o].lo == want.lo[q] && out_value[o].hi == want.hi[q] && out_hash[o] == want.hash[q],
                      "dense k=%d canonical=%d drop_last=%d position %llu", k, canonical, drop_last, (unsigned long long)q);
                w_cnt += want.valid[q];
                w_lo ^= want.lo[q];
                w_hi ^= want.hi[q];
                w_h ^= want.hash[q];
                w_sum += want.hash[q];
            }
            CHECK(dense.cnt == w_cnt && dense.xlo == w_lo && dense.xhi == w_hi && dense.xh == w_h && dense.sx == w_sum, "dense digest k=%d", k);
            CHECK(std::memcmp(&dense, &digest_only, sizeof(dense)) == 0, "digest-only path differs k=%d", k);
            std::printf("dense %d %d %llu %llu %llu %llu %llu\n", canonical, drop_last, dense.cnt, dense.xlo, dense.xhi, dense.xh, dense.sx);

            // sampler: prefix over tiles, then the record pass — once with room for everything, once one record short
            std::vector<uint64_t> w_pos;
            for (uint64_t q = first; q < end; ++q)
                if (want.valid[q] && want.hash[q] < threshold) w_pos.push_back(q);
            unsigned long long total = 0;
            for (int tile = 0; tile < p.n_tiles; ++tile) {
                tile_base[tile] = total;
                total += tile_counts[tile];
            }
            CHECK(total == w_pos.size() && samp.cnt == total, "sampler count k=%d: %llu, want %zu", k, total, w_pos.size());
            for (int pass = 0; pass < 2; ++pass) {
                const uint64_t cap = pass == 0 ? total : (total ? total - 1 : 0);
                const uint64_t guard = 0xfeedfacecafebeefULL;
                std::vector<bl::U64x2> rv(cap);            // exact size again
                std::vector<uint64_t> rp(cap), rh(cap + 1, guard);
                p.rec_value = reinterpret_cast<uint64_t*>(rv.data());
                p.rec_pos = rp.data();
                p.rec_hash = rh.data();
                p.capacity = cap;
                for (int tile = 0; tile < p.n_tiles; ++tile) {
                    const int64_t q0 = p.origin + (int64_t)tile * bl::H;
                    stage_all(p, codes, flags, q0);
                    uint64_t at = tile_base[tile];
                    for (int tid = 0; tid < bl::TPB; ++tid) {
                        const uint32_t sel = masks[(size_t)tile * bl::TPB + tid];
                        bl::kmer128_emit_thread(p, codes.data(), tid, q0, sel, at);
                        at += (unsigned)__builtin_popcount(sel);
                    }
                }
                CHECK(rh[cap] == guard, "sampler wrote at capacity k=%d", k);
                for (uint64_t r = 0; r < cap; ++r) {
                    const uint64_t q = w_pos[r];
                    CHECK(rp[r] == q + origin && rv[r].lo == want.lo[q] && rv[r].hi == want.hi[q] && rh[r] == want.hash[q],
                          "sampler k=%d canonical=%d drop_last=%d record %llu", k, canonical, drop_last, (unsigned long long)r);
                }
            }
            unsigned long long s_lo = 0, s_hi = 0, s_h = 0, s_pos = 0;
            for (uint64_t q : w_pos) {
                s_lo ^= want.lo[q];
                s_hi ^= want.hi[q];
                s_h ^= want.hash[q];
                s_pos ^= q + origin;
            }
            CHECK(samp.xlo == s_lo && samp.xhi == s_hi && samp.xh == s_h && samp.sx == s_pos, "sampler digest k=%d", k);
            std::printf("sample %d %d %llu %llu %llu %llu %llu\n", canonical, drop_last, samp.cnt, samp.xlo, samp.xhi, samp.xh, samp.sx);
        }
    }
    return 0;
}

// <first> = @FILE: every range of FILE in one run (emu128_common.hpp: run_ranges)
int main(int argc, char** argv) { return run_ranges(argc, argv, 3, scan_one); }
