#!/usr/bin/env python3
"""Gbp/s of scan + pack + count for k-mers up to k = 64 on ONE GPU (150-bp reads): bl_scan_super_kmers + bl_pack_super_kmers128 +
bl_count_super_kmers128 at (51, 21) and (64, 32), with the LDS tables (default) and with "count128_tables" = 0 (expand + 128-bit sort
+ run-length for every bucket), and bl_count_super_kmers at (31, 15) in the same process as the yardstick.  One JSON line.
    count128_bench.py [Gbp of synthetic reads, default 0.3]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B

gbp = float(sys.argv[1]) if len(sys.argv) > 1 else 0.3
L = 150
ctx = B.Context(0)
n = int(gbp * 1e9) // L * L
b = ctx.synth(42, n, L)
out = {"bases": n, "read_len": L}


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def chain(tag, records, count, reps=3):
    best = None
    for _ in range(reps):  # the last passes are warm (scratch allocated); the best whole chain is reported with its own stages
        (recs, hashes), t_scan = timed(records)
        (u, c), t_count = timed(lambda: count(recs))
        if best is None or t_scan + t_count < best[0] + best[1]:
            best = (t_scan, t_count, int(recs.shape[0]), int(u.shape[0]), int(c.sum()))
        del recs, hashes, u, c
    out[tag] = {"scan_pack_ms": round(best[0] * 1e3, 2), "count_ms": round(best[1] * 1e3, 2), "Gbp_s": round(n / (best[0] + best[1]) / 1e9, 2),
                "count_only_Gbp_s": round(n / best[1] / 1e9, 2), "super_kmers": best[2], "distinct": best[3], "kmers": best[4]}
    return out[tag]


base = chain("k31_m15_u64", lambda: b.super_kmer_records(31, 15, seed=42, canonical=True), lambda r: ctx.count_super_kmers(r, 31, 15, seed=42, canonical=True))
for k, m in ((51, 21), (64, 32)):
    for tables in (1, 0):
        ctx.set_option("count128_tables", tables)
        tag = f"k{k}_m{m}_" + ("tables" if tables else "sort")
        r = chain(tag, lambda: b.super_kmer_records128(k, m, seed=42, canonical=True), lambda r: ctx.count_super_kmers128(r, k, m, seed=42, canonical=True))
        r["ratio_to_k31_m15_u64"] = round(r["Gbp_s"] / base["Gbp_s"], 3)
    ctx.set_option("count128_tables", 1)
    a, s = out[f"k{k}_m{m}_tables"], out[f"k{k}_m{m}_sort"]
    assert (a["distinct"], a["kmers"]) == (s["distinct"], s["kmers"]), "the two paths disagree"
print(json.dumps(out))
