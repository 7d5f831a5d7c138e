#!/usr/bin/env python3
"""Rates of the count table on ONE GPU.  Tables of random distinct keys: 2^16, 2^22, 2^26, 2^28 entries of 62-bit keys (k = 31, one
word) and 2^26 entries of 102-bit keys (k = 51, two words).  For each table:
  lookup   bl_table_lookup_* on 2^26 queries, half of them present, in random order, with the prefix index forced to P = 0, 8, 16, 20, 24
           and automatic;
  torch    the same queries through torch.searchsorted + gather + compare (one-word tables only: the keys are below 2^63, so int64
           order is the key order; torch has no 128-bit form) — what a user could write before this call existed;
  scan     bl_scan_kmer_counts on synthetic 150-bp reads against the same table (automatic P), beside the unfused chain
           bl_scan_kmers128 (values only) followed by bl_table_lookup_*, in Gbp/s.
Every call is synchronous, so the host clock around it is the call time.  After one warm-up pass over all variants, `rounds` passes are
taken with the variants INTERLEAVED (variant after variant inside a pass, not pass after pass of one variant); the median is reported
with the spread (min .. max) beside it.  `beats` compares whole spreads: true only when the slower end of one lies above the faster end
of the other.  What binds the kernels is not measured here (no counter run).  Writes one JSON file.
    lookup_bench.py [--out profiles/lookup_bench.json] [--log2 16 22 26 28] [--wide-log2 26] [--queries-log2 26] [--scan-gbp 1.5] [--rounds 3]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B
from biolib_amd.scan import _flags

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_bench.json"))
ap.add_argument("--log2", type=int, nargs="*", default=[16, 22, 26, 28])
ap.add_argument("--wide-log2", type=int, nargs="*", default=[26])
ap.add_argument("--queries-log2", type=int, default=26)
ap.add_argument("--scan-gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(4096)
FORCED = (0, 8, 16, 20, 24)


def rand_keys(n, key_bits):
    if key_bits <= 64:
        return torch.randint(0, 1 << key_bits, (n,), dtype=torch.int64, device="cuda", generator=gen)
    t = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), dtype=torch.int64, device="cuda", generator=gen)
    t[:, 1] &= (1 << (key_bits - 64)) - 1
    return t


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


def bench_table(lg, key_bits, k):
    n, nq = 1 << lg, 1 << args.queries_log2
    wide = key_bits > 64
    src = rand_keys(n, key_bits)
    tables = {}
    for p in FORCED + (-1,):
        ctx.set_option("table_prefix_bits", p)
        tables[p] = ctx.count_table(src, None, key_bits=key_bits)
    ctx.set_option("table_prefix_bits", -1)
    del src
    auto = tables[-1]
    keys = auto.keys
    pick = torch.randint(0, auto.n_distinct, (nq // 2,), device="cuda", generator=gen)
    # present and absent queries alternate; each is a random draw (of the table's slots, of all keys), so no two neighbours are related
    q = torch.stack([keys.index_select(0, pick), rand_keys(nq // 2, key_bits)], dim=1).reshape((nq, 2) if wide else (nq,)).contiguous()
    del pick
    res = {"entries": auto.n_distinct, "key_bits": key_bits, "queries": nq, "automatic_P": auto.prefix_bits}
    answers = {}
    variants = {}
    for p, t in tables.items():
        name = "P_auto" if p < 0 else f"P_{t.prefix_bits}_forced_{p}"
        variants[name] = (lambda t=t, name=name: answers.__setitem__(name, t.lookup(q)))
    if not wide:
        def torch_chain():
            pos = torch.searchsorted(keys, q).clamp_(max=auto.n_distinct - 1)
            answers["torch"] = torch.where(keys[pos] == q, auto.counts[pos], torch.zeros((), dtype=torch.int32, device="cuda"))
        variants["torch"] = torch_chain
    times = interleaved(variants)
    ref = answers["P_auto"]
    for name, a in answers.items():
        assert torch.equal(a, ref), name + " disagrees"
    res["present_fraction"] = round(float((ref != 0).float().mean()), 4)
    res["lookup"] = {name: row(s, nq, "Glookups_s") for name, s in times.items()}
    forced = {name: r for name, r in res["lookup"].items() if "forced" in name}
    best = max(forced, key=lambda nm: forced[nm]["Glookups_s"])
    res["fastest_forced"] = best
    res["automatic_within_spread_of_fastest"] = bool(res["lookup"]["P_auto"]["Glookups_s_max"] >= forced[best]["Glookups_s_min"])
    if not wide:
        res["lookup_beats_torch"] = beats(res["lookup"]["P_auto"], res["lookup"]["torch"], "Glookups_s")
    answers.clear()
    del q, ref
    for p in FORCED:
        tables[p].close()
    # the scan against the automatic table
    n_bases = int(args.scan_gbp * 1e9) // 150 * 150
    if n_bases:
        b = ctx.synth(7, n_bases, 150)
        counts = torch.empty(n_bases, dtype=torch.int32, device="cuda")
        values = torch.empty((n_bases, 2), dtype=torch.int64, device="cuda")
        chain_counts = torch.empty(n_bases, dtype=torch.int32, device="cuda")
        L = ctx._lib
        import ctypes as C

        def fused():
            b.kmer_counts_raw(auto, k, _flags(False, False, True), 0, 0, counts, None)

        def chain():
            b.kmers128_raw(k, 0, _flags(False, False, True), 0, 0, values, None, None)
            src_q = values if wide else values[:, 0].contiguous()
            call = L.bl_table_lookup_u128 if wide else L.bl_table_lookup_u64
            B.capi.check(call(ctx._h, auto._h, C.c_void_p(src_q.data_ptr()), n_bases, C.c_void_p(chain_counts.data_ptr())))

        st = interleaved({"fused": fused, "unfused_chain": chain})
        res["scan"] = {name: row(s, n_bases, "Gbp_s") for name, s in st.items()}
        res["scan"]["bases"] = n_bases
        res["scan"]["fused_beats_chain"] = beats(res["scan"]["fused"], res["scan"]["unfused_chain"], "Gbp_s")
        del counts, values, chain_counts
        b.close()
    auto.close()
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "note": "interleaved rounds after one warm-up pass; median with min .. max beside it; what binds the kernels: not measured", "tables": {}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
for name, lg, key_bits, k in [(f"u64_2^{lg}", lg, 62, 31) for lg in args.log2] + [(f"u128_2^{lg}", lg, 102, 51) for lg in args.wide_log2]:
    out["tables"][name] = bench_table(lg, key_bits, k)
    print(json.dumps({name: out["tables"][name]}), flush=True)
    with open(args.out, "w") as f:  # after every table: a run cut short keeps what it measured
        json.dump(out, f, indent=1)
        f.write("\n")
