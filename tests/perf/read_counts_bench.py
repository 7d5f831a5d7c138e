#!/usr/bin/env python3
"""What the per-read reduction of bl_scan_read_counts costs beside the lookups, on ONE GPU.  The batches and tables of lookup_bench.py's
`scan` rows: synthetic reads (150 bp, and 10 kbp) against tables of random distinct 62-bit keys (k = 31) of 2^22 and 2^26 entries.
Three variants per (read length, table):
  read_counts   bl_scan_read_counts: one 48-byte record per read;
  kmer_counts   bl_scan_kmer_counts writing counts and valid (five bytes per base) — the parent's call, unchanged;
  then_torch    kmer_counts followed by the segment reduction a caller writes in torch today.  The reads have one length, so the caller can
                view the arrays as [reads, read_len] and reduce along rows — the cheapest form torch offers; ragged reads would need
                scatter_reduce over sequence ids.  n_found is taken as count > 0 there (the per-position output cannot tell a stored 0
                from an absent key).
Every call is synchronous, so the host clock around it is the call time.  After one warm-up pass over all variants, `rounds` passes are
taken with the variants INTERLEAVED; the median is reported with the spread (min .. max) beside it.  `beats` compares whole spreads: true
only when the slower end of one lies above the faster end of the other; `behind` likewise.  What binds the kernels is not measured here
(no counter run).  Writes one JSON file.
    read_counts_bench.py [--out profiles/read_counts_bench.json] [--log2 22 26] [--read-len 150 10000] [--scan-gbp 1.5] [--rounds 3]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B
from biolib_amd.scan import ReadCounts, _flags

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_counts_bench.json"))
ap.add_argument("--log2", type=int, nargs="*", default=[22, 26])
ap.add_argument("--read-len", type=int, nargs="*", default=[150, 10000])
ap.add_argument("--scan-gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--min-count", type=int, default=1)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(4096)
K, KEY_BITS = 31, 62
U32 = (1 << 32) - 1


def interleaved(variants):
    """{name: callable} -> {name: [seconds per round]}: one warm-up pass, then args.rounds passes over all variants in turn"""
    times = {name: [] for name in variants}
    for rnd in range(args.rounds + 1):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(time.perf_counter() - t0)
    return times


def row(seconds, work, unit):
    rates = sorted(work / s / 1e9 for s in seconds)
    return {"ms_median": round(statistics.median(seconds) * 1e3, 3), unit: round(statistics.median(rates), 3), unit + "_min": round(rates[0], 3),
            unit + "_max": round(rates[-1], 3)}


def beats(new, base, unit):
    return bool(new[unit + "_min"] > base[unit + "_max"])


def torch_reduce(counts, valid, n_reads, read_len, min_count):
    """the eight fields per read from the per-position arrays, along the rows of a [reads, read_len] view"""
    v = valid.view(n_reads, read_len) == 1
    c = counts.view(n_reads, read_len).to(torch.int64) & U32
    solid = (c >= min_count) & v
    weak = v & ~solid
    pos = torch.arange(read_len, device=c.device)
    big = 1 << 62
    return (v.sum(1), ((c > 0) & v).sum(1), solid.sum(1), torch.where(v, c, big).amin(1), c.amax(1), c.sum(1),
            torch.where(weak, pos, big).amin(1), torch.where(weak, pos + 1, 0).amax(1))


def bench(table, lg, read_len):
    n_bases = int(args.scan_gbp * 1e9) // read_len * read_len
    n_reads = n_bases // read_len
    b = ctx.synth(7, n_bases, read_len)
    assert b.n_seqs == n_reads
    counts = torch.empty(n_bases, dtype=torch.int32, device="cuda")
    valid = torch.empty(n_bases, dtype=torch.uint8, device="cuda")
    rc = ReadCounts(ctx, n_reads)
    flags = _flags(False, False, True)
    keep = {}

    def read_counts():
        keep["rc"] = b.read_counts_raw(table, K, flags, args.min_count, rc.records).as_dict()

    def kmer_counts():
        keep["kc"] = b.kmer_counts_raw(table, K, flags, 0, 0, counts, valid).as_dict()

    def then_torch():
        kmer_counts()
        keep["torch"] = torch_reduce(counts, valid, n_reads, read_len, args.min_count)

    st = interleaved({"read_counts": read_counts, "kmer_counts": kmer_counts, "then_torch": then_torch})
    # the three agree
    assert keep["rc"] == keep["kc"]
    fields = (rc.n_kmers, rc.n_found, rc.n_solid, rc.min_count, rc.max_count, rc.sum_counts, rc.weak_begin, rc.weak_end)
    for i, (mine, theirs) in enumerate(zip(fields, keep["torch"])):
        mine = mine.to(torch.int64) & U32 if mine.dtype == torch.int32 else mine
        if i == 3:
            theirs = torch.where(theirs == (1 << 62), U32, theirs)
        if i == 6:
            theirs = torch.where(theirs == (1 << 62), -1, theirs)
        assert torch.equal(mine, theirs), f"field {i} differs from the torch reduction"
    res = {name: row(s, n_bases, "Gbp_s") for name, s in st.items()}
    res.update(bases=n_bases, reads=n_reads, read_len=read_len, table_entries=table.n_distinct, valid_kmers=keep["rc"]["count"], found=keep["rc"]["xor_hash"],
               bytes_out_read_counts=48 * n_reads, bytes_out_kmer_counts=5 * n_bases)
    res["read_counts_beats_then_torch"] = beats(res["read_counts"], res["then_torch"], "Gbp_s")
    res["read_counts_behind_kmer_counts"] = beats(res["kmer_counts"], res["read_counts"], "Gbp_s")
    del counts, valid, rc, keep
    b.close()
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "k": K, "min_count": args.min_count,
       "note": "interleaved rounds after one warm-up pass; median with min .. max beside it; what binds the kernels: not measured", "rows": {}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
for lg in args.log2:
    table = ctx.count_table(torch.randint(0, 1 << KEY_BITS, (1 << lg,), dtype=torch.int64, device="cuda", generator=gen), None, key_bits=KEY_BITS)
    for read_len in args.read_len:
        name = f"reads_{read_len}_table_2^{lg}"
        out["rows"][name] = bench(table, lg, read_len)
        print(json.dumps({name: out["rows"][name]}), flush=True)
        with open(args.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(out, f, indent=1)
            f.write("\n")
    table.close()
