#!/usr/bin/env python3
"""What correcting substitutions costs beside the lookups, on ONE GPU.  Reads (150 bp, and 10 kbp) drawn from a random genome, k = 31, a
canonical table of the genome's error-free k-mers (every count 3 = min_count), substitution rates 0, 0.1 % and 1 %.  Variants per (read
length, rate), all on the same batch and table:
  read_counts   bl_scan_read_counts: the lookup pass no corrector avoids — the yardstick;
  read_edits    bl_scan_read_edits alone (capacity = the number of edits, known from a counting call outside the timing);
  apply_edits   bl_batch_apply_edits alone;
  chain         both (Batch.correct_by_counts, one pass);
  then_torch    the same correction as far as torch can write it on the arrays of bl_scan_kmer_counts: states, run boundaries, shape and
                support of every run — the candidate list.  The test of the three alternatives has no torch form short of building the
                patched k-mers and calling bl_table_lookup; it is NOT included, so this variant does less than read_edits.
Every call is synchronous, so the host clock around it is the call time.  After one warm-up pass over all variants, `rounds` passes are
taken with the variants INTERLEAVED; the median is reported with the spread (min .. max) beside it.  The call's time is reported as a
multiple of read_counts, and the test pass's lookups per second (3 per k-mer of every candidate run; the pass is not timed alone, so
this is lookups over the time read_edits takes beyond read_counts) beside the lookup rates of profiles/lookup_bench.json.  Clocks are not
pinned; rocm-smi's current sclk is noted before and after where the tool is there.  Writes one JSON file.
    correct_bench.py [--out profiles/correct_bench.json] [--read-len 150 10000] [--gbp 1.5] [--rates 0 0.001 0.01] [--rounds 3]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B
from biolib_amd.scan import ReadCounts, _flags

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correct_bench.json"))
ap.add_argument("--read-len", type=int, nargs="*", default=[150, 10000])
ap.add_argument("--gbp", type=float, default=1.5)
ap.add_argument("--genome-log2", type=int, default=24)
ap.add_argument("--rates", type=float, nargs="*", default=[0.0, 0.001, 0.01])
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(31)
K, MIN_COUNT = 31, 3
LETTERS = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout  # (a query, no setting)
        return [line.strip() for line in out.splitlines() if "sclk" in line][:1]
    except Exception:
        return []


def interleaved(variants):
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
    return {"ms_median": round(statistics.median(seconds) * 1e3, 3), "ms_min": round(min(seconds) * 1e3, 3), "ms_max": round(max(seconds) * 1e3, 3),
            unit: round(statistics.median(rates), 3)}


def make_table(genome_codes):
    g = ctx.from_tensor(LETTERS[genome_codes.long()].contiguous())
    n = g.n_bases
    vals = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    g.kmers128_raw(K, 0, _flags(True, False, True), 0, 0, vals, None, ok)
    keys = vals[ok == 1][:, 0].contiguous()
    uniq = keys[: ctx.sort_unique(keys)]
    table = ctx.count_table(uniq, torch.full((uniq.numel(),), MIN_COUNT, dtype=torch.int32, device="cuda"), key_bits=2 * K)
    g.close()
    return table


def make_reads(genome_codes, read_len, rate):
    n_reads = int(args.gbp * 1e9) // read_len
    out = torch.empty(n_reads * read_len, dtype=torch.uint8, device="cuda")
    step = max((1 << 26) // read_len, 1)
    col = torch.arange(read_len, device="cuda")
    for r0 in range(0, n_reads, step):
        m = min(step, n_reads - r0)
        starts = torch.randint(0, genome_codes.numel() - read_len + 1, (m, 1), device="cuda", generator=gen)
        codes = genome_codes[starts + col]
        if rate:
            err = torch.rand(codes.shape, device="cuda", generator=gen) < rate
            codes = torch.where(err, (codes + torch.randint(1, 4, codes.shape, device="cuda", generator=gen, dtype=torch.uint8)) % 4, codes)
        out[r0 * read_len:(r0 + m) * read_len] = LETTERS[codes.long()].reshape(-1)
    return out, n_reads


def torch_candidates(counts, valid, n_reads, read_len):
    """states, runs, shape and support along the rows of a [reads, read_len] view -> number of candidate runs"""
    n = read_len - K + 1
    v = valid.view(n_reads, read_len)[:, :n] == 1
    c = counts.view(n_reads, read_len)[:, :n]
    weak = v & (c < MIN_COUNT)  # (counts below 2^31 here)
    solid = v & ~weak
    pad = torch.zeros((n_reads, 1), dtype=torch.bool, device=weak.device)
    begins = weak & ~torch.cat([pad, weak[:, :-1]], 1)
    ends = weak & ~torch.cat([weak[:, 1:], pad], 1)
    rb, cb = begins.nonzero(as_tuple=True)
    re_, ce = ends.nonzero(as_tuple=True)  # (row-major: the i-th begin and the i-th end are one run)
    length = ce - cb + 1
    left = (cb >= 1) & solid[rb, (cb - 1).clamp(min=0)]
    right = ~left & (ce <= n - 2) & solid[rb, (ce + 1).clamp(max=n - 1)]
    fits = (left & (ce == torch.minimum(cb + K - 1, torch.full_like(cb, n - 1)))) | (right & (cb == (ce - K + 1).clamp(min=0)))
    return int(fits.sum()), int((length[fits] * 3).sum())


def bench(table, genome_codes, read_len, rate):
    bases, n_reads = make_reads(genome_codes, read_len, rate)
    n_bases = bases.numel()
    b = ctx.from_tensor(bases, read_len=read_len)
    rc = ReadCounts(ctx, n_reads)
    flags = _flags(True, False, True)
    _, stats = b.read_edits_raw(table, K, 1, MIN_COUNT, 1, None, 0)
    n_edits = int(stats.n_edits)
    edits = torch.zeros((max(n_edits, 1), 2), dtype=torch.int64, device="cuda")
    counts = torch.empty(n_bases, dtype=torch.int32, device="cuda")
    valid = torch.empty(n_bases, dtype=torch.uint8, device="cuda")
    keep = {}

    def read_counts():
        b.read_counts_raw(table, K, flags, MIN_COUNT, rc.records)

    def read_edits():
        keep["stats"] = b.read_edits_raw(table, K, 1, MIN_COUNT, 1, edits, max(n_edits, 1))[1].as_dict()

    def apply_edits():
        b.apply_edits(edits[:n_edits]).close()

    def chain():
        out, _, _ = b.correct_by_counts(table, K, MIN_COUNT, canonical=True)
        keep["left"] = out
        out.close()

    def then_torch():
        b.kmer_counts_raw(table, K, flags, 0, 0, counts, valid)
        keep["torch"] = torch_candidates(counts, valid, n_reads, read_len)

    before = clocks()
    st = interleaved({"read_counts": read_counts, "read_edits": read_edits, "apply_edits": apply_edits, "chain": chain, "then_torch": then_torch})
    s = keep["stats"]
    n_cand = s["n_edits"] + s["n_ambiguous"] + s["n_no_base"]
    res = {name: row(t, n_bases, "Gbp_s") for name, t in st.items()}
    base = res["read_counts"]["ms_median"]
    extra = max(res["read_edits"]["ms_median"] - base, 1e-6)
    res.update(bases=n_bases, reads=n_reads, read_len=read_len, rate=rate, stats=s, table_entries=table.n_distinct, candidates=n_cand, then_torch_candidates=keep["torch"][0], then_torch_agrees=bool(keep["torch"][0] == n_cand), test_lookups=keep["torch"][1],
               read_edits_over_read_counts=round(res["read_edits"]["ms_median"] / base, 3), chain_over_read_counts=round(res["chain"]["ms_median"] / base, 3),
               then_torch_over_read_edits=round(res["then_torch"]["ms_median"] / res["read_edits"]["ms_median"], 3),
               test_lookups_per_s_over_the_extra_time=round(keep["torch"][1] / (extra * 1e-3), 1), sclk_before=before, sclk_after=clocks())
    b.close()
    del counts, valid, edits, rc, bases
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "k": K, "min_count": MIN_COUNT, "rows": {},
       "note": "interleaved rounds after one warm-up pass; medians with min .. max; clocks not pinned; then_torch stops at the candidate list"}
try:  # the table lookup's own rate at the automatic prefix width, for the comparison
    tables = json.load(open(os.path.join(ROOT, "profiles", "lookup_bench.json")))["tables"]
    out["lookup_bench_Glookups_s"] = {name: t["lookup"]["P_auto"]["Glookups_s"] for name, t in tables.items() if "lookup" in t and "P_auto" in t["lookup"]}
except Exception:
    out["lookup_bench_Glookups_s"] = "profiles/lookup_bench.json not readable"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
genome = torch.randint(0, 4, (1 << args.genome_log2,), dtype=torch.uint8, device="cuda", generator=gen)
table = make_table(genome)
for read_len in args.read_len:
    for rate in args.rates:
        name = f"reads_{read_len}_rate_{rate}"
        out["rows"][name] = bench(table, genome, read_len, rate)
        print(json.dumps({name: out["rows"][name]}), flush=True)
        with open(args.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(out, f, indent=1)
            f.write("\n")
table.close()
