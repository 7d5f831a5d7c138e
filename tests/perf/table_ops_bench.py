#!/usr/bin/env python3
"""Times of the count-table algebra on ONE GPU against what the same answer cost before it existed.  Rows: two tables of random distinct
62-bit keys at 2^22 and at 2^26 entries each, half of each shared with the other; one row of 102-bit keys; one row with a 16 : 1 size
ratio.  Counts are drawn so that about half the keys are singletons.  For each row:
  union      a.union(b, count="sum")            against  torch.cat of both tables' arrays + ctx.count_table (radix sort + reduce_by_key)
  intersect  a.intersect(b, count="min")        against  b.lookup(a.keys), a torch mask, torch.minimum, ctx.count_table of the survivors
  filter     a.filter(min_count=2)              against  a torch mask + ctx.count_table
  compare    a.compare(b)                       (no table; nothing to compare with for tables with counts)
Every call is synchronous, so the host clock around it is the call time; the result table is closed inside the timed call on both
sides.  After one warm-up pass over all variants, `rounds` passes are taken with the variants INTERLEAVED; the median is reported with
the spread (min .. max) beside it.  `beats` compares whole spreads: true only when the slowest new time lies below the fastest baseline
time.  What binds the kernels is not measured here (no counter run).  Writes one JSON file.
    table_ops_bench.py [--out profiles/table_ops_bench.json] [--log2 22 26] [--wide-log2 24] [--ratio-log2 26 22] [--rounds 3]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_ops_bench.json"))
ap.add_argument("--log2", type=int, nargs="*", default=[22, 26])
ap.add_argument("--wide-log2", type=int, nargs="*", default=[24])
ap.add_argument("--ratio-log2", type=int, nargs="*", default=[26, 22])
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(8192)


def rand_keys(n, key_bits):
    if key_bits <= 64:
        return torch.randint(0, 1 << key_bits, (n,), dtype=torch.int64, device="cuda", generator=gen)
    t = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), dtype=torch.int64, device="cuda", generator=gen)
    t[:, 1] &= (1 << (key_bits - 64)) - 1
    return t


def rand_counts(n):
    """1 for about half the keys, 2 .. 49 for the others"""
    c = torch.randint(2, 50, (n,), dtype=torch.int32, device="cuda", generator=gen)
    c[torch.rand(n, device="cuda", generator=gen) < 0.5] = 1
    return c


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


def row(seconds):
    s = sorted(seconds)
    return {"ms_median": round(statistics.median(s) * 1e3, 3), "ms_min": round(s[0] * 1e3, 3), "ms_max": round(s[-1] * 1e3, 3)}


def bench_row(n_a, n_b, key_bits):
    shared = min(n_a, n_b) // 2
    pool = rand_keys(n_a + n_b - shared, key_bits)  # A: the first n_a, B: the last n_b; the middle is shared
    a = ctx.count_table(pool[:n_a].contiguous(), rand_counts(n_a), key_bits=key_bits)
    b = ctx.count_table(pool[n_a - shared:].contiguous(), rand_counts(n_b), key_bits=key_bits)
    del pool
    kept = {}

    def keep(name, t):
        if name not in kept:  # the first result of every variant stays for the comparison below
            kept[name] = (t.keys.clone(), t.counts.clone())
        t.close()

    def base_union():
        keep("base_union", ctx.count_table(torch.cat([a.keys, b.keys]), torch.cat([a.counts, b.counts]), key_bits=key_bits))

    def base_intersect():
        cb = b.lookup(a.keys)
        hit = cb != 0  # (the stored counts are at least 1)
        keep("base_intersect", ctx.count_table(a.keys[hit].contiguous(), torch.minimum(a.counts[hit], cb[hit]).contiguous(), key_bits=key_bits))

    def base_filter():
        hit = a.counts >= 2  # (counts below 2^31: the int32 view compares like the uint32)
        keep("base_filter", ctx.count_table(a.keys[hit].contiguous(), a.counts[hit].contiguous(), key_bits=key_bits))

    stats = {}
    variants = {
        "union": lambda: keep("union", a.union(b, count="sum")), "base_union": base_union,
        "intersect": lambda: keep("intersect", a.intersect(b, count="min")), "base_intersect": base_intersect,
        "filter": lambda: keep("filter", a.filter(min_count=2)), "base_filter": base_filter,
        "compare": lambda: stats.update(a.compare(b)),
    }
    times = interleaved(variants)
    for name in ("union", "intersect", "filter"):
        assert torch.equal(kept[name][0], kept["base_" + name][0]) and torch.equal(kept[name][1], kept["base_" + name][1]), name + " disagrees with its baseline"
    res = {"entries_a": a.n_distinct, "entries_b": b.n_distinct, "key_bits": key_bits, "n_both": stats["n_both"], "jaccard": round(stats["jaccard"], 4),
           "n_union": int(kept["union"][0].shape[0]), "n_filter": int(kept["filter"][0].shape[0]), "times": {name: row(s) for name, s in times.items()}}
    for name in ("union", "intersect", "filter"):
        new, base = res["times"][name], res["times"]["base_" + name]
        res[name + "_speedup_median"] = round(base["ms_median"] / new["ms_median"], 2)
        res[name + "_beats_baseline"] = bool(new["ms_max"] < base["ms_min"])
    a.close()
    b.close()
    kept.clear()
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "note": "interleaved rounds after one warm-up pass; median with min .. max beside it; what binds the kernels: not measured", "rows": {}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
rows = [(f"u64_2^{lg}", 1 << lg, 1 << lg, 62) for lg in args.log2] + [(f"u128_2^{lg}", 1 << lg, 1 << lg, 102) for lg in args.wide_log2]
if len(args.ratio_log2) == 2:
    rows.append((f"u64_2^{args.ratio_log2[0]}_vs_2^{args.ratio_log2[1]}", 1 << args.ratio_log2[0], 1 << args.ratio_log2[1], 62))
for name, n_a, n_b, key_bits in rows:
    out["rows"][name] = bench_row(n_a, n_b, key_bits)
    print(json.dumps({name: out["rows"][name]}), flush=True)
    with open(args.out, "w") as f:  # after every row: a run cut short keeps what it measured
        json.dump(out, f, indent=1)
        f.write("\n")
