#!/usr/bin/env python3
"""What duplicate removal costs on ONE GPU: bl_scan_read_duplicates (records and spans, no statistics) beside three yardsticks on the
same batch.  About 1.5 Gbp per row, fixed-length reads of random bases; a fraction of the units are copies of earlier ones, shuffled in:
  single150_0     150-bp reads, no duplicates
  single150_25    150-bp reads, 25 % copies
  paired150_25    150-bp interleaved mates, 25 % of the pairs copies
  canonical150_25 150-bp reads, 25 % copies, half of them reverse-complemented, BL_DEDUP_CANONICAL
  single10k_5     10-kbp reads, 5 % copies
  prefix150_25    150-bp reads, 25 % copies, prefix_len 50
Beside each row:
  adapters    (a) bl_scan_read_adapters with one adapter (TruSeq), spans only
  kmers31     (b) bl_scan_kmers at k = 31, canonical, digest only
  torch       (c) torch.unique(dim=0, return_inverse=True) over the base matrix (the key columns; the canonical row first takes the
              smaller of every row and its reverse complement), then a scatter-min for the first index of every class.  Its kept
              mask is asserted equal to the call's before anything is timed.
and the call's phases (hash, sort, resolve, finish) from device events: bl_ctx_kernel_timing makes the call set markers between them.
Timed with the host clock around calls that end in a device synchronise.  After one warm-up pass `rounds` passes are taken with the
variants INTERLEAVED; the median is reported with the whole spread (min .. max) beside it.  Clocks are not pinned: the card runs under its
own power management, as in the other benches of this directory.  No counter run is made here: what binds the kernels is not measured.
    dedup_bench.py [--out profiles/dedup_bench.json] [--gbp 1.5] [--rounds 3] [--rows name,name] [--no-torch]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B
from biolib_amd import capi

ROWS = {  # name: (read length, paired, canonical, copies, prefix_len)
    "single150_25": (150, False, False, 0.25, 0),
    "single150_0": (150, False, False, 0.0, 0),
    "paired150_25": (150, True, False, 0.25, 0),
    "canonical150_25": (150, False, True, 0.25, 0),
    "single10k_5": (10_000, False, False, 0.05, 0),
    "prefix150_25": (150, False, False, 0.25, 50),
}
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_bench.json"))
ap.add_argument("--gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rows", default=",".join(ROWS))
ap.add_argument("--no-torch", action="store_true")
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(2028)
LETTERS = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
a_rule = B.Batch.adapter_rule([B.ADAPTERS["truseq"]])


def interleaved(variants):
    times = {name: [] for name in variants}
    for rnd in range(args.rounds + 1):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(time.perf_counter() - t0)
    return times


def stats(seconds):
    return {"ms_median": round(statistics.median(seconds) * 1e3, 3), "ms_min": round(min(seconds) * 1e3, 3), "ms_max": round(max(seconds) * 1e3, 3)}


def code_matrix(n_units, width, copies, reverse):
    """uint8 codes [n_units, width]: the last `copies` of the rows copy random earlier ones (half of them reverse-complemented where
    `reverse`), then all rows are shuffled"""
    n_new = n_units - int(n_units * copies)
    m = torch.randint(0, 4, (n_units, width), dtype=torch.uint8, device="cuda", generator=gen)
    if n_new < n_units:
        src = torch.randint(0, n_new, (n_units - n_new,), device="cuda", generator=gen)
        m[n_new:] = m[src]
        if reverse:
            half = n_new + (n_units - n_new) // 2
            m[half:] = 3 - m[half:].flip(1)
    return m[torch.randperm(n_units, device="cuda", generator=gen)]


def letters(codes):
    """the ASCII bases of a code matrix, in slices (an index tensor is eight times the codes)"""
    out = torch.empty_like(codes)
    step = max(1, (64 << 20) // codes.shape[1])
    for a in range(0, codes.shape[0], step):
        out[a:a + step] = LETTERS[codes[a:a + step].long()]
    return out


def torch_kept(codes, canonical, prefix_len):
    """the torch composition -> a bool mask [n_units]: the unit is the first of its class"""
    keys = codes[:, :prefix_len] if prefix_len else codes
    if canonical:
        rc = 3 - keys.flip(1)
        differ = keys != rc
        first = differ.to(torch.uint8).argmax(1, keepdim=True)
        take = (rc.gather(1, first) < keys.gather(1, first)) & differ.any(1, keepdim=True)
        keys = torch.where(take, rc, keys)
    n = keys.shape[0]
    uniq, inverse = torch.unique(keys, dim=0, return_inverse=True)
    at = torch.arange(n, device=keys.device)
    first = torch.full((uniq.shape[0],), n, dtype=torch.int64, device=keys.device).scatter_reduce_(0, inverse, at, "amin")
    return first[inverse] == at


read_gbps, copy_gbps = ctx.probe_hbm(4 << 30, 3)
out = {"rounds": args.rounds, "gbp": args.gbp, "probe_hbm": {"read_GB_s": round(read_gbps, 1), "copy_GB_s": round(copy_gbps, 1)},
       "note": "interleaved rounds after one warm-up pass; median with min .. max beside it; host clock around calls that end in a synchronise; clocks not "
               "pinned; the dedup call writes records and spans, no statistics; phases from device events of separate passes; no counter run: what binds "
               "the kernels is not measured",
       "rows": {}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

for name in args.rows.split(","):
    L, paired, canonical, copies, prefix_len = ROWS[name]
    per = 2 if paired else 1
    n_units = int(args.gbp * 1e9) // (L * per)
    codes = code_matrix(n_units, L * per, copies, canonical)
    batch = ctx.upload(letters(codes).reshape(-1).cpu().numpy(), read_len=L)
    n = batch.n_seqs
    assert n == n_units * per and batch.read_len == L
    rule = capi.DedupRule()
    rule.flags = (capi.DEDUP_PAIRED if paired else 0) | (capi.DEDUP_CANONICAL if canonical else 0)
    rule.prefix_len = prefix_len
    records = torch.zeros((n_units, 2), dtype=torch.int64, device="cuda")
    spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    a_spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    st = capi.DedupStats()
    torch.cuda.synchronize()
    batch.read_duplicates_raw(rule, records, spans, st)
    row = {"n_reads": n, "n_units": n_units, "read_len": L, "n_bases": n * L, "stats": st.as_dict()}
    variants = {"dedup": lambda: batch.read_duplicates_raw(rule, records, spans, None),
                "adapters": lambda: batch.read_adapters_raw(a_rule, None, a_spans, None, None, None),
                "kmers31": lambda: batch.kmers(31, 42, canonical=True, arrays=False)}
    if not args.no_torch:
        mine = ((records[:, 1] >> 32) & capi.DUP_DUPLICATE) == 0
        theirs = torch_kept(codes, canonical, prefix_len)
        assert torch.equal(theirs, mine), "the torch composition and the call disagree"
        row["torch_equals_call"] = True
        del theirs, mine
        variants["torch"] = lambda: torch_kept(codes, canonical, prefix_len)
    for vname, seconds in interleaved(variants).items():
        row[vname] = stats(seconds)
        row[vname]["Gbp_s"] = round(n * L / statistics.median(seconds) / 1e9, 1)
    phases = {k: [] for k in ("hash", "sort", "resolve", "finish")}
    ctx.kernel_timing(True)
    for _ in range(args.rounds):
        batch.read_duplicates_raw(rule, records, spans, None)
        t = ctx.mark_times()
        for k, (a, b) in zip(phases, zip(t, t[1:])):
            phases[k].append((b - a) / 1e3)
    ctx.kernel_timing(False)
    row["phases"] = {k: stats(v) for k, v in phases.items()}
    out["rows"][name] = row
    print(name, json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    batch.close()
    del codes, records, spans, a_spans
    torch.cuda.empty_cache()
print("wrote", args.out)
