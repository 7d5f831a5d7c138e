// TEST INFRASTRUCTURE: the per-thread bodies of the 32-byte super-k-mer record and of the counter's table
// (biolib_amd/csrc/bl_superkmer128_core.hpp) run on the host under AddressSanitizer / UBSan — lane by lane, a host WaveTable128 standing
// in for LDS — against a plain `unsigned __int128` evaluation written here.  Built and run by tests/test_emu_superkmer128.py, which
// compares what is printed / written below with tests/superkmer128_model.py.
//
//   emu_superkmer128 pack <in> <out>
//       in:  u64 n_bases, origin, n_groups, k; u64 first_pos[n_groups]; u8 sizes[n_groups]; u8 mm_pos[n_groups]; u8 bases[n_bases]
//       out: u64 records[4 n_groups] (sk128_pack of every group; the bases live in an exact-size heap block: an over-read is an ASan report)
//   emu_superkmer128 count <in> <k> <m> <canonical>
//       in:  u64 n; u64 records[4 n] — treated as ONE bucket in this order
//       prints  expand <n_kmers> <xor lo> <xor hi>     sk128_expand of every record == the plain evaluation (exit 1 otherwise)
//               minhash <xor of the records' minimizer hashes>   sk128_minimizer_hash == the plain evaluation
//               path table|fallback, rounds <records per round ...>
//               kmer <lo> <hi> <count>                 the table's contents, slot order (table path only)
#define EMU_NAME "emu_superkmer128"
#include "emu128_common.hpp"  // u128, rotl, fmix
#include "../../biolib_amd/csrc/bl_superkmer128_core.hpp"

// MurmurHash3_x64_128 of the 8 bytes of v, first word (written out here: no code shared with the header under test)
static uint64_t plain_hash8(uint64_t v, uint32_t seed)
{
    const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
    uint64_t h1 = seed, h2 = seed, k1 = v;
    k1 *= c1; k1 = rotl(k1, 31); k1 *= c2; h1 ^= k1;
    h1 ^= 8; h2 ^= 8;
    h1 += h2; h2 += h1;
    h1 = fmix(h1); h2 = fmix(h2);
    return h1 + h2;
}

// base i of a record, 0 <= i < 128 (the twelve low bits of word 3 are no bases)
static int plain_base(const uint64_t* r, int i)
{
    if (i >= 122) return 0;
    return (int)((r[i >> 5] >> (62 - 2 * (i & 31))) & 3u);
}
// the (canonical) t-mer at base pos
static u128 plain_mer(const uint64_t* r, int pos, int t, bool canonical)
{
    u128 fwd = 0, rc = 0;
    for (int i = 0; i < t; ++i) {
        const int c = plain_base(r, pos + i);
        fwd = (fwd << 2) | (u128)c;
        rc |= (u128)(3 ^ c) << (2 * i);
    }
    return canonical && rc < fwd ? rc : fwd;
}

static std::vector<uint8_t> read_file(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> out((size_t)n);
    if (n && fread(out.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
    fclose(f);
    return out;
}

static int run_pack(const char* in, const char* outp)
{
    const std::vector<uint8_t> raw = read_file(in);
    uint64_t hdr[4];
    memcpy(hdr, raw.data(), 32);
    const uint64_t n_bases = hdr[0], origin = hdr[1], n = hdr[2];
    const int k = (int)hdr[3];
    std::vector<uint64_t> fp(n);
    memcpy(fp.data(), raw.data() + 32, 8 * n);
    const uint8_t* sizes = raw.data() + 32 + 8 * n;
    const uint8_t* mm = sizes + n;
    uint8_t* bases = (uint8_t*)malloc(n_bases ? n_bases : 1);  // exact size: nothing behind n_bases may be read
    memcpy(bases, mm + n, n_bases);
    std::vector<uint64_t> recs(4 * n);
    for (uint64_t g = 0; g < n; ++g) bl::sk128_pack(bases, n_bases, fp[g] - origin, (int)sizes[g], (int)mm[g], k, &recs[4 * g]);
    free(bases);
    FILE* f = fopen(outp, "wb");
    if (!f) { perror(outp); return 2; }
    fwrite(recs.data(), 8, recs.size(), f);
    fclose(f);
    return 0;
}

// the wave of count_one_bucket128, its lanes one after the other; false: the bucket is the fallback's
static bool emu_bucket(bl::WaveTable128& t, const std::vector<uint64_t>& recs, int k, bool canonical, std::vector<int>& round_sizes)
{
    const size_t n = recs.size() / 4;
    if (n > (size_t)bl::CT128_MAXREC) return false;
    memset(t.owner, 0, sizeof(t.owner));
    memset(t.cnt, 0, sizeof(t.cnt));
    unsigned held = 0;
    for (size_t at = 0; at < n;) {
        unsigned incl[64], size[64];
        int n_take = 0;
        unsigned run = 0, total = 0;
        for (int lane = 0; lane < 64; ++lane) {
            size[lane] = at + lane < n ? (unsigned)bl::sk128_size(recs[4 * (at + lane) + 3]) : 0u;
            run += size[lane];
            incl[lane] = run;
            if (size[lane] != 0 && incl[lane] <= (unsigned)bl::CT128_CAP) { ++n_take; total = incl[lane]; }
        }
        if (held + total > (unsigned)bl::CT128_FULL) return false;
        round_sizes.push_back(n_take);
        for (int lane = 0; lane < n_take; ++lane) {
            const uint64_t* r = &recs[4 * (at + lane)];
            bl::table128_stage(t, lane, r[0], r[1], r[2], r[3]);
            for (unsigned q = 0; q < size[lane]; ++q) t.work[incl[lane] - size[lane] + q] = (uint16_t)((lane << 6) | q);
        }
        unsigned fresh = 0;
        for (unsigned base = 0; base < total; base += 64) {
            bool pending[64], won[64];
            uint64_t klo[64] = {0}, khi[64] = {0};
            uint32_t h[64];
            for (int lane = 0; lane < 64; ++lane) {
                pending[lane] = base + lane < total;
                if (pending[lane]) bl::table128_work_key(t, t.work[base + lane], k, canonical, klo[lane], khi[lane]);
                h[lane] = bl::table128_slot(klo[lane], khi[lane]);
            }
            int step = 0;
            for (; step < bl::CT128_SLOTS; ++step) {
                for (int lane = 0; lane < 64; ++lane) won[lane] = pending[lane] && bl::table128_claim(t, h[lane], klo[lane], khi[lane]);
                bool any = false;
                for (int lane = 0; lane < 64; ++lane) {
                    if (pending[lane] && bl::table128_settle(t, h[lane], klo[lane], khi[lane])) {
                        pending[lane] = false;
                        fresh += won[lane] ? 1u : 0u;
                    }
                    any |= pending[lane];
                }
                if (!any) break;
            }
            if (step == bl::CT128_SLOTS) { fprintf(stderr, "a lane is still pending after CT128_SLOTS steps\n"); exit(1); }
        }
        at += (size_t)n_take;
        held += fresh;
    }
    return true;
}

static int run_count(const char* in, int k, int m, bool canonical)
{
    const std::vector<uint8_t> raw = read_file(in);
    uint64_t n;
    memcpy(&n, raw.data(), 8);
    std::vector<uint64_t> recs(4 * n);
    memcpy(recs.data(), raw.data() + 8, 32 * n);
    const uint32_t seed = 0x9E3779B9u;
    uint64_t n_kmers = 0, xlo = 0, xhi = 0, xmin = 0;
    for (uint64_t g = 0; g < n; ++g) {
        const uint64_t* r = &recs[4 * g];
        const int size = bl::sk128_size(r[3]);
        std::vector<uint64_t> out(2 * size);  // exact size: a write behind the record's k-mers is an ASan report
        bl::sk128_expand(r[0], r[1], r[2], r[3], k, canonical, out.data());
        for (int q = 0; q < size; ++q) {
            const u128 want = plain_mer(r, q, k, canonical);
            if (out[2 * q] != (uint64_t)want || out[2 * q + 1] != (uint64_t)(want >> 64)) {
                fprintf(stderr, "record %llu k-mer %d: expand differs from the plain evaluation\n", (unsigned long long)g, q);
                return 1;
            }
            // the single extraction the counter uses
            uint32_t c[8], five[5];
            uint64_t lo, hi;
            bl::sk128_chunks(r[0], r[1], r[2], r[3], c);
            bl::sk128_pick5(c, q >> 4, five);
            bl::sk128_mer_at(five, q, k, canonical, lo, hi);
            if (lo != (uint64_t)want || hi != (uint64_t)(want >> 64)) {
                fprintf(stderr, "record %llu k-mer %d: extraction differs from the plain evaluation\n", (unsigned long long)g, q);
                return 1;
            }
            xlo ^= lo;
            xhi ^= hi;
        }
        n_kmers += (uint64_t)size;
        const uint64_t mh = bl::sk128_minimizer_hash(r[0], r[1], r[2], r[3], m, canonical, seed);
        if (mh != plain_hash8((uint64_t)plain_mer(r, bl::sk128_mm_pos(r[3]), m, canonical), seed)) {
            fprintf(stderr, "record %llu: minimizer hash differs from the plain evaluation\n", (unsigned long long)g);
            return 1;
        }
        xmin ^= mh;
    }
    printf("expand %llu %llu %llu\n", (unsigned long long)n_kmers, (unsigned long long)xlo, (unsigned long long)xhi);
    printf("minhash %llu\n", (unsigned long long)xmin);
    bl::WaveTable128* t = new bl::WaveTable128;
    std::vector<int> round_sizes;
    const bool kept = emu_bucket(*t, recs, k, canonical, round_sizes);
    printf("path %s\n", kept ? "table" : "fallback");
    printf("rounds");
    for (int r : round_sizes) printf(" %d", r);
    printf("\n");
    if (kept)
        for (uint32_t h = 0; h < (uint32_t)bl::CT128_SLOTS; ++h)
            if (t->owner[h]) printf("kmer %llu %llu %u\n", (unsigned long long)t->klo[h], (unsigned long long)t->khi[h], bl::table128_count(*t, h));
    delete t;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "pack")) return run_pack(argv[2], argv[3]);
    if (argc == 6 && !strcmp(argv[1], "count")) return run_count(argv[2], atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) != 0);
    fprintf(stderr, "usage: emu_superkmer128 pack <in> <out> | count <in> <k> <m> <canonical>\n");
    return 2;
}
