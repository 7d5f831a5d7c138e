// TEST INFRASTRUCTURE — the super-k-mer scan with 32-byte records (bl_scan_super_kmer_records128) on the host: the whole
// count -> prefix scan -> emit pipeline of emu_scan.cpp, thread by thread, with ScanParams::records128 set, so that pass 1 spills and
// pass 2 stages what staged_chunks gives for wide records and phase_emit packs them with emit_record128 / pack_group128.  Built by
// tests/test_emu_records128.py with -fsanitize=address,undefined: the code arrays are poisoned per tile and the output arrays have
// exactly the size of the need, so a chunk read that was never staged or a record written behind the capacity is a report here, not a
// GPU fault.  Not a product path.
//
//   emu_records128 run <in> <out>     in : u64 n_bases, n_offsets, read_len, k, m, seed, flags, n_jobs; n_jobs x (first, n);
//                                          n_offsets x u64 offsets (n_offsets = 0: one sequence, or fixed-length reads); the bases
//                                     out: per job u64 count, group ends, then count x 4 record words, then count hashes
//   emu_records128 plan <first> <n> <n_bases> <read_len> <unit> <w> <flags>     the tile plan: emu_plan's nine values
#include "emu_scan.cpp"

#include <cstdio>

namespace {

std::vector<uint8_t> read_file(const char* path)
{
    std::vector<uint8_t> out;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return out;
}

// one call of the C ABI's shape: both outputs NULL counts only
void scan(const EmuBatch* b, uint64_t first, uint64_t n, unsigned k, unsigned m, uint64_t seed, unsigned flags, uint64_t* records, uint64_t* hashes,
          uint64_t capacity, unsigned long long* result)
{
    ScanParams p{};
    fill_common(p, b->bases, b->n_bases, b->single ? nullptr : b->bits.data(), MODE_SUPERKMER, first, n, m, k - m + 1, seed, flags, b->read_len);
    p.out_records = records;
    p.out_hash = hashes;
    p.records128 = 1;
    p.capacity = (records || hashes) ? capacity : 0;
    std::memset(result, 0, 8 * sizeof(unsigned long long));
    if (p.n_tiles > 0) run_mode<MODE_SUPERKMER>(p, result);
}

int run(const char* in, const char* out)
{
    const std::vector<uint8_t> raw = read_file(in);
    uint64_t h[8];
    if (raw.size() < sizeof(h)) return 2;
    memcpy(h, raw.data(), sizeof(h));
    const uint64_t n_bases = h[0], n_offs = h[1], read_len = h[2], n_jobs = h[7];
    const unsigned k = (unsigned)h[3], m = (unsigned)h[4], flags = (unsigned)h[6];
    if (raw.size() != sizeof(h) + 16 * n_jobs + 8 * n_offs + n_bases) { fprintf(stderr, "bad input size\n"); return 2; }
    std::vector<uint64_t> jobs(2 * n_jobs + 1), offs(n_offs + 1);
    memcpy(jobs.data(), raw.data() + sizeof(h), 16 * n_jobs);
    memcpy(offs.data(), raw.data() + sizeof(h) + 16 * n_jobs, 8 * n_offs);
    EmuBatch* b = emu_batch(raw.data() + sizeof(h) + 16 * n_jobs + 8 * n_offs, n_bases, n_offs ? offs.data() : nullptr, n_offs ? n_offs - 1 : 0, read_len);
    FILE* f = fopen(out, "wb");
    if (!b || !f) return 2;
    for (uint64_t j = 0; j < n_jobs; ++j) {
        const uint64_t first = jobs[2 * j], n = jobs[2 * j + 1];
        unsigned long long r0[8], r1[8];
        scan(b, first, n, k, m, h[5], flags, nullptr, nullptr, 0, r0);
        const uint64_t need = r0[0];
        uint64_t* recs = new uint64_t[4 * need];  // exact: one record more is a report
        uint64_t* hs = new uint64_t[need];
        scan(b, first, n, k, m, h[5], flags, recs, hs, need, r1);
        if (r1[0] != need || r1[4] != r0[4]) { fprintf(stderr, "job %llu: the count-only run and the run with records disagree\n", (unsigned long long)j); return 1; }
        const uint64_t head[2] = {need, r1[4]};
        fwrite(head, 8, 2, f);
        fwrite(recs, 8, 4 * need, f);
        fwrite(hs, 8, need, f);
        delete[] recs;
        delete[] hs;
    }
    fclose(f);
    emu_batch_free(b);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 9 && !strcmp(argv[1], "plan")) {
        long long v[9];
        emu_plan(MODE_SUPERKMER, strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10),
                 (unsigned)atoi(argv[6]), (unsigned)atoi(argv[7]), (unsigned)atoi(argv[8]), v);
        for (int i = 0; i < 9; ++i) printf("%lld%c", v[i], i == 8 ? '\n' : ' ');
        return 0;
    }
    fprintf(stderr, "usage: emu_records128 run <in> <out> | plan <first> <n> <n_bases> <read_len> <unit> <w> <flags>\n");
    return 2;
}
