#!/usr/bin/env python3
"""The super-k-mer record chain for k up to 64 on ONE GPU: bl_scan_super_kmer_records128 (the 32-byte record built inside the scan) against
bl_scan_super_kmers + bl_pack_super_kmers128, at (51, 21) and (64, 32), canonical, on 10-kbp reads and on 150-bp reads, with
bl_scan_super_kmer_records at (31, 15) beside them; then the wide chain's total (records + bl_count_super_kmers128) on a smaller batch.
Buffers are allocated once; every figure is wall time around a synchronised call; the A/B rounds are interleaved (fused, unfused, fused,
..) after one untimed round, and median and best are reported.

    records128_bench.py [--gbp 1.5] [--rounds 3] [--count-gbp 0.3] [--out profiles/records128_bench.json]
                        [--parent-lib PATH [--guard-rounds 3]]

--parent-lib: a libbiolib_amd.so built from the parent commit.  `bench.py --gpus 1 --full` then runs in child processes, this commit's
library and the parent's in turn, and the headline value and other_configs.C4 of every run are recorded with the verdict: the difference
of the medians must lie inside the parent's own spread (max - min) over its rounds."""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SEED = 42


def records_chain(args):
    import torch
    import biolib_amd as B
    from biolib_amd import capi

    ctx = B.Context(0)
    L_ = capi.lib()
    flags = B.FLAG_CANONICAL | B.FLAG_SYNC
    out = {}

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn()
        ctx.sync(); torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def summary(n, times):
        return {"median_ms": round(statistics.median(times) * 1e3, 3), "best_ms": round(min(times) * 1e3, 3), "all_ms": [round(t * 1e3, 3) for t in times],
                "median_Gbp_s": round(n / statistics.median(times) / 1e9, 2), "best_Gbp_s": round(n / min(times) / 1e9, 2)}

    for L in (10_000, 150):
        n = int(args.gbp * 1e9) // L * L
        b = ctx.synth(SEED, n, L)
        row = out[f"reads_{L}bp"] = {"bases": n, "read_len": L}
        for k, m in ((51, 21), (64, 32), (31, 15)):
            cap = int(n * 2.4 / (k - m + 2)) + 65536
            hs, fp, sz, mp = ctx.empty_u64(cap), ctx.empty_u64(cap), ctx.empty_u8(cap), ctx.empty_u8(cap)
            recs = torch.empty((cap, 4), dtype=torch.int64, device=ctx.torch_device)
            p = lambda t: C.c_void_p(t.data_ptr())
            res = capi.Result()

            def fused():
                capi.check(L_.bl_scan_super_kmer_records128(ctx._h, b._h, 0, 0, k, m, SEED, flags, p(recs), p(hs), cap, C.byref(res)))
                return int(res.count)

            def unfused():
                b.super_kmers_raw(k, m, SEED, flags, 0, 0, None, fp, mp, sz, hs, cap, res)
                capi.check(L_.bl_pack_super_kmers128(ctx._h, b._h, p(fp), p(sz), p(mp), int(res.count), k, m, p(recs)))
                return int(res.count)

            def narrow():  # the 16-byte record of the 64-bit path, (31, 15) only
                capi.check(L_.bl_scan_super_kmer_records(ctx._h, b._h, 0, 0, k, m, SEED, flags, p(recs), p(hs), cap, C.byref(res)))
                return int(res.count)

            legs = {"fused": fused, "scan_plus_pack128": unfused}
            if (k, m) == (31, 15):
                legs["records_16_byte"] = narrow
            counts = {name: fn() for name, fn in legs.items()}  # untimed round: scratch allocated, clocks up
            assert len(set(counts.values())) == 1, counts
            times = {name: [] for name in legs}
            for _ in range(args.rounds):
                for name, fn in legs.items():
                    times[name].append(timed(fn)[1])
            cell = row[f"k{k}_m{m}"] = {"super_kmers": counts["fused"], **{name: summary(n, t) for name, t in times.items()}}
            cell["fused_over_scan_plus_pack128"] = round(cell["fused"]["median_Gbp_s"] / cell["scan_plus_pack128"]["median_Gbp_s"], 3)
            cell["fused_not_slower"] = cell["fused"]["median_ms"] <= cell["scan_plus_pack128"]["median_ms"]
            del hs, fp, sz, mp, recs
        b.close()

    # the wide chain's total: records + count (the counter allocates its own outputs: a smaller batch, as tests/perf/count128_bench.py)
    L = 150
    n = int(args.count_gbp * 1e9) // L * L
    b = ctx.synth(SEED, n, L)
    row = out["chain_total_reads_150bp"] = {"bases": n, "read_len": L}
    for k, m in ((51, 21), (64, 32)):
        times = {"fused": [], "scan_plus_pack128": []}
        for r in range(args.rounds + 1):
            for name in times:
                def chain():
                    recs, _ = b.super_kmer_records128(k, m, seed=SEED, canonical=True, fused=name == "fused")
                    u, c = ctx.count_super_kmers128(recs, k, m, seed=SEED, canonical=True)
                    return int(u.shape[0])
                distinct, t = timed(chain)
                if r:  # (the first round is untimed)
                    times[name].append(t)
        row[f"k{k}_m{m}"] = {"distinct": distinct, **{name: summary(n, t) for name, t in times.items()}}
    b.close()
    ctx.close()
    return out


def c4_guard(args):
    """bench.py --full in child processes, this commit's library and the parent's in turn"""
    runs = {"this_commit": [], "parent": []}
    for _ in range(args.guard_rounds):
        for who in ("this_commit", "parent"):
            env = dict(os.environ)
            if who == "parent":
                env["BIOLIB_AMD_LIB"] = os.path.abspath(args.parent_lib)
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-next-rows", "--no-h2d"]
            run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
            if run.returncode != 0:
                raise RuntimeError(f"bench.py ({who}) exit {run.returncode}: {run.stderr[-2000:]}")
            line = [ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1]
            d = json.loads(line)
            runs[who].append({"headline_Gbp_s": d["value"], "C4_Gbp_s": d["other_configs"]["C4_super_kmers_50Gbp_10kbp_reads"]["value"]})
    out = {"command": "bench.py --gpus 1 --steps 5 --warmup 1 --full --no-cpu-baseline --no-next-rows --no-h2d", "rounds": args.guard_rounds, "runs": runs}
    for key in ("headline_Gbp_s", "C4_Gbp_s"):
        a, p = [r[key] for r in runs["this_commit"]], [r[key] for r in runs["parent"]]
        spread = max(p) - min(p)
        diff = statistics.median(a) - statistics.median(p)
        out[key] = {"this_commit_median": statistics.median(a), "parent_median": statistics.median(p), "difference": round(diff, 3), "parent_spread": round(spread, 3),
                    "inside_parent_spread": abs(diff) <= spread}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=1.5)
    ap.add_argument("--count-gbp", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "records128_bench.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--guard-rounds", type=int, default=3)
    ap.add_argument("--skip-chain", action="store_true", help="only the C4 regression guard (keeps the chain figures the output file already holds)")
    args = ap.parse_args()
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    if not args.skip_chain:
        out["records_chain"] = records_chain(args)
        out["records_chain"]["protocol"] = f"{args.rounds} interleaved rounds after one untimed round; wall time around synchronised calls; buffers allocated once"
    if args.parent_lib:
        out["c4_regression_guard"] = c4_guard(args)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
