// TEST INFRASTRUCTURE: what the host emulators of the 128-bit scans share (emu_kmers128.cpp, emu_syncmers128.cpp, emu_minimizers128.cpp;
// emu_superkmer128.cpp takes the hash pieces): the plain 2-bit code and MurmurHash3 written out here, the CHECK macro, the batch file
// with its exact-size copy of the bases and its start bits, and the staging of a whole tile.  The including file defines EMU_NAME, the
// program's name in front of its messages.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../biolib_amd/csrc/bl_kmers128_core.hpp"

typedef unsigned __int128 u128;

static int nt4(uint8_t c)
{
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
        default: return 4;
    }
}

static uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
static uint64_t fmix(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
    return k;
}
// MurmurHash3_x64_128 of the 16 bytes of v, first word (written out here: no code shared with the headers under test)
static uint64_t plain_hash(u128 v, uint32_t seed)
{
    const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
    uint64_t k1 = (uint64_t)v, k2 = (uint64_t)(v >> 64), h1 = seed, h2 = seed;
    k1 *= c1; k1 = rotl(k1, 31); k1 *= c2; h1 ^= k1;
    h1 = rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
    k2 *= c2; k2 = rotl(k2, 33); k2 *= c1; h2 ^= k2;
    h2 = rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    h1 ^= 16; h2 ^= 16;
    h1 += h2; h2 += h1;
    h1 = fmix(h1); h2 = fmix(h2);
    return h1 + h2;
}

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::fprintf(stderr, EMU_NAME ": " __VA_ARGS__); \
            std::fprintf(stderr, "\n");           \
            std::exit(1);                         \
        }                                         \
    } while (0)

// batch file: u64 n_bases, u64 n_seqs, u64 offsets[n_seqs + 1], bases
struct EmuBatch {
    uint64_t n_bases = 0, n_seqs = 0;
    std::vector<uint64_t> offs;
    std::vector<uint8_t> seq;
    uint8_t* exact = nullptr;          // an exact-size heap copy of the bases (16-byte aligned as the device buffer is; the sanitizer
                                       // sees every byte past n_bases)
    std::vector<uint32_t> start_bits;  // as the library builds them: one bit per first base of a sequence, four words of slack

    explicit EmuBatch(const char* path)
    {
        FILE* f = std::fopen(path, "rb");
        CHECK(f, "cannot open %s", path);
        uint64_t hdr[2];
        CHECK(std::fread(hdr, 8, 2, f) == 2, "short file");
        n_bases = hdr[0];
        n_seqs = hdr[1];
        offs.resize(n_seqs + 1);
        CHECK(std::fread(offs.data(), 8, n_seqs + 1, f) == n_seqs + 1, "short file");
        seq.resize(n_bases);
        CHECK(n_bases == 0 || std::fread(seq.data(), 1, n_bases, f) == n_bases, "short file");
        std::fclose(f);
        exact = static_cast<uint8_t*>(std::malloc(n_bases ? n_bases : 1));
        std::memcpy(exact, seq.data(), n_bases);
        start_bits.assign((n_bases + 31) / 32 + 4, 0);
        for (uint64_t q = 0; q < n_seqs; ++q)
            if (offs[q] < n_bases) start_bits[offs[q] >> 5] |= 1u << (offs[q] & 31);
    }
    ~EmuBatch() { std::free(exact); }
    EmuBatch(const EmuBatch&) = delete;
    EmuBatch& operator=(const EmuBatch&) = delete;

    // the batch's fields of the scan parameters
    void describe(bl::Kmer128Params& km) const
    {
        km.bases = exact;
        km.n_bases = (int64_t)n_bases;
        km.start_bits = start_bits.data();
    }
};

// all of a tile's chunks from position r0 on, as the workgroup stages them
static void stage_all(const bl::Kmer128Params& km, std::vector<uint32_t>& codes, std::vector<uint32_t>& flags, int64_t r0)
{
    const bl::ScanParams lp = bl::kmer128_staging_params(km);
    for (int c = 0; c < (int)codes.size(); ++c) bl::stage_chunk(lp, codes.data(), flags.data(), c, r0);
}

// A list of ranges in one run: where the program takes <first> <n>, "@FILE 0" names a text file of "first n" pairs, one range per line.
// `one` is the program's single-range body; before each range's lines a line "range <first> <n>" is printed.  at: index of <first> in argv.
static int run_ranges(int argc, char** argv, int at, int (*one)(int, char**))
{
    if (argc <= at + 1 || argv[at][0] != '@') return one(argc, argv);
    FILE* f = std::fopen(argv[at] + 1, "r");
    CHECK(f, "cannot open %s", argv[at] + 1);
    std::vector<char*> args(argv, argv + argc);
    unsigned long long first, n;
    char a[32], b[32];
    while (std::fscanf(f, "%llu %llu", &first, &n) == 2) {
        std::snprintf(a, sizeof a, "%llu", first);
        std::snprintf(b, sizeof b, "%llu", n);
        args[at] = a;
        args[at + 1] = b;
        std::printf("range %llu %llu\n", first, n);
        const int rc = one(argc, args.data());
        if (rc != 0) return rc;
    }
    std::fclose(f);
    return 0;
}
