// TEST INFRASTRUCTURE: the per-thread bodies of bl_scan_minimizers128 (biolib_amd/csrc/bl_minimizers128_core.hpp) run on the host — a
// workgroup's phases lane by lane, host arrays standing in for LDS — under AddressSanitizer / UBSan, against a plain
// `unsigned __int128` evaluation of the rule written here.  Built and run by tests/test_emu_minimizers128.py, which compares the
// digests printed below with its own Python model.
//
//   emu_minimizers128 <batch file> <unit> <w> <first> <n>
// batch file: u64 n_bases, u64 n_seqs, u64 offsets[n_seqs + 1], bases.  For canonical x drop_last it prints
//   min <canonical> <drop_last> count xor_value aux xor_hash xor_pos
// and exits non-zero on the first disagreement with the plain evaluation.
#define EMU_NAME "emu_minimizers128"
#include "emu128_common.hpp"
#include "../../biolib_amd/csrc/bl_minimizers128_core.hpp"

struct Plain {
    std::vector<uint8_t> valid;
    std::vector<u128> value;
    std::vector<uint64_t> hash;
    std::vector<int64_t> occ;  // per window start: the occurrence's position, -1 where no window
};

static Plain plain_scan(const std::vector<uint8_t>& seq, const std::vector<uint64_t>& offs, int k, int w, uint32_t seed, bool canonical, bool drop_last)
{
    const size_t n = seq.size();
    Plain r{std::vector<uint8_t>(n, 0), std::vector<u128>(n, 0), std::vector<uint64_t>(n, 0), std::vector<int64_t>(n, -1)};
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
            r.valid[i + 1 - k] = 1;
            r.value[i + 1 - k] = v;
            r.hash[i + 1 - k] = plain_hash(v, seed);
        }
    }
    for (size_t p = 0; p + w <= n; ++p) {
        int64_t arg = (int64_t)p;
        bool all = true;
        for (size_t j = p; j < p + w; ++j) {
            all = all && r.valid[j];
            if (r.hash[j] < r.hash[arg]) arg = (int64_t)j;  // strict: the leftmost minimum stays
        }
        if (all) r.occ[p] = arg;
    }
    return r;
}

static int scan_one(int argc, char** argv)
{
    CHECK(argc == 6, "usage: emu_minimizers128 <batch file> <unit> <w> <first> <n>");
    const EmuBatch batch(argv[1]);
    const uint64_t n_bases = batch.n_bases;
    const std::vector<uint64_t>& offs = batch.offs;
    const std::vector<uint8_t>& seq = batch.seq;
    const int k = std::atoi(argv[2]), w = std::atoi(argv[3]);
    const uint64_t first = std::strtoull(argv[4], nullptr, 10), n_arg = std::strtoull(argv[5], nullptr, 10);
    const uint64_t end = (n_arg == 0 || first + n_arg > n_bases) ? n_bases : first + n_arg;
    const uint32_t seed = 0x9e3779b9u;
    const uint64_t origin = 1000000007ull;
    CHECK(k >= 1 && k <= bl::MAX_UNIT128 && w >= 1 && w <= bl::MAX_W && first < end, "bad arguments");

    for (int canonical = 0; canonical < 2; ++canonical) {
        for (int drop_last = 0; drop_last < 2; ++drop_last) {
            static Plain plain[4];  // (a list of ranges: the batch, unit and w stay, the plain evaluation runs once per strand and drop_last)
            static bool have[4];
            Plain& want = plain[2 * canonical + drop_last];
            if (!have[2 * canonical + drop_last]) want = plain_scan(seq, offs, k, w, seed, canonical, drop_last);
            have[2 * canonical + drop_last] = true;
            auto is_record = [&](int64_t q) {
                if (q < (int64_t)first || q >= (int64_t)end || want.occ[q] < 0) return false;
                return q == 0 || want.occ[q - 1] != want.occ[q];
            };
            bl::Min128Params p{};
            batch.describe(p.km);
            p.km.pos_base = (int64_t)origin;
            bl::plan_kmers128((int64_t)first, (int64_t)end, p.km);
            p.km.unit = k;
            p.km.seed = seed;
            p.km.canonical = canonical;
            p.km.drop_last = drop_last;
            p.w = w;
            // exact sizes: a read or write outside them is a finding
            std::vector<uint32_t> codes(bl::MIN128_NCHUNK), flags(bl::MIN128_NCHUNK);
            std::vector<uint64_t> lds(bl::MIN128_SLOTS);
            std::vector<uint16_t> valid(bl::MIN128_NVALID);
            std::vector<uint16_t> masks((size_t)p.km.n_tiles * bl::TPB);
            std::vector<uint32_t> lane_offs((size_t)p.km.n_tiles * 3 * bl::TPB);  // as pass 1 leaves them for pass 2
            std::vector<unsigned long long> tile_counts(p.km.n_tiles), tile_base(p.km.n_tiles);
            bl::Kmer128Acc acc{0, 0, 0, 0, 0};
            for (int tile = 0; tile < p.km.n_tiles; ++tile) {
                const int64_t r0 = p.km.origin + (int64_t)tile * bl::H - 16;
                stage_all(p.km, codes, flags, r0);
                // every phase between two barriers runs for all lanes before the next one starts.  The arrays are zeroed first: a
                // window that read a word phase A did not write would find a minimum (or an invalid unit) there
                std::fill(lds.begin(), lds.end(), 0);
                std::fill(valid.begin(), valid.end(), 0);
                for (int tid = 0; tid < bl::TPB; ++tid) bl::min128_hash_thread(p, codes.data(), flags.data(), lds.data(), valid.data(), tid, r0);
                unsigned long long cnt = 0;
                for (int tid = 0; tid < bl::TPB; ++tid) {
                    bl::Min128Offs o;
                    const uint32_t sel = bl::min128_window_thread(p, lds.data(), valid.data(), tid, r0, o);
                    bl::min128_digest_thread(p.km, codes.data(), lds.data(), tid, r0, sel, o, acc);
                    masks[(size_t)tile * bl::TPB + tid] = (uint16_t)sel;
                    bl::min128_offs_store(lane_offs.data(), tile, tid, o);
                    cnt += (unsigned)__builtin_popcount(sel);
                    for (int t = 0; t < bl::S; ++t) {
                        const int64_t q = r0 + 16 * (tid + 1) + t;
                        const bool rec = q >= 0 && q < (int64_t)n_bases && is_record(q);
                        CHECK(((sel >> t) & 1u) == (rec ? 1u : 0u), "unit=%d w=%d canonical=%d drop_last=%d window %lld: lane says %u", k, w, canonical, drop_last,
                              (long long)q, (sel >> t) & 1u);
                        if (rec) CHECK(q + bl::min128_off(o, t) == want.occ[q], "unit=%d w=%d window %lld: offset %d, occurrence %lld", k, w, (long long)q, bl::min128_off(o, t), (long long)want.occ[q]);
                    }
                }
                tile_counts[tile] = cnt;
            }
            std::vector<uint64_t> w_pos, w_hash;
            std::vector<u128> w_val;
            unsigned long long x_lo = 0, x_hi = 0, x_h = 0, x_pos = 0;
            for (uint64_t q = first; q < end; ++q)
                if (is_record((int64_t)q)) {
                    const int64_t o = want.occ[q];
                    w_pos.push_back((uint64_t)o + origin);
                    w_val.push_back(want.value[o]);
                    w_hash.push_back(want.hash[o]);
                    x_lo ^= (uint64_t)want.value[o];
                    x_hi ^= (uint64_t)(want.value[o] >> 64);
                    x_h ^= want.hash[o];
                    x_pos ^= (uint64_t)o + origin;
                }
            unsigned long long total = 0;
            for (int tile = 0; tile < p.km.n_tiles; ++tile) {
                tile_base[tile] = total;
                total += tile_counts[tile];
            }
            CHECK(total == w_pos.size() && acc.xlo == x_lo && acc.xhi == x_hi && acc.xh == x_h && acc.sx == x_pos, "count / digest unit=%d w=%d: %llu, want %zu", k, w,
                  total, w_pos.size());
            // the record pass: once with room for everything, once one record short
            for (int pass = 0; pass < 2; ++pass) {
                const uint64_t cap = pass == 0 ? total : (total ? total - 1 : 0);
                std::vector<bl::U64x2> rv(cap);  // exact sizes
                std::vector<uint64_t> rp(cap), rh(cap);
                p.km.rec_value = reinterpret_cast<uint64_t*>(rv.data());
                p.km.rec_pos = rp.data();
                p.km.rec_hash = rh.data();
                p.km.capacity = cap;
                for (int tile = 0; tile < p.km.n_tiles; ++tile) {
                    const int64_t r0 = p.km.origin + (int64_t)tile * bl::H - 16;
                    stage_all(p.km, codes, flags, r0);
                    uint64_t at = tile_base[tile];
                    for (int tid = 0; tid < bl::TPB; ++tid) {
                        const uint32_t sel = masks[(size_t)tile * bl::TPB + tid];
                        bl::min128_emit_thread(p.km, codes.data(), tid, r0, sel, bl::min128_offs_load(lane_offs.data(), tile, tid), at);
                        at += (unsigned)__builtin_popcount(sel);
                    }
                }
                for (uint64_t r = 0; r < cap; ++r)
                    CHECK(rp[r] == w_pos[r] && rh[r] == w_hash[r] && rv[r].lo == (uint64_t)w_val[r] && rv[r].hi == (uint64_t)(w_val[r] >> 64), "record %llu unit=%d w=%d",
                          (unsigned long long)r, k, w);
            }
            std::printf("min %d %d %llu %llu %llu %llu %llu\n", canonical, drop_last, total, acc.xlo, acc.xhi, acc.xh, acc.sx);
        }
    }
    return 0;
}

// <first> = @FILE: every range of FILE in one run (emu128_common.hpp: run_ranges)
int main(int argc, char** argv) { return run_ranges(argc, argv, 4, scan_one); }
