#!/usr/bin/env python3
"""Rates of the set operations on 16-byte keys on ONE GPU, beside the 8-byte calls at the same element counts (the yardstick):
  sort_unique128 at key_bits 82 (k = 41) and 128, sort_unique (u64);
  jaccard128 with the merge kernel and with the search kernel forced ("jaccard128_path" 1 / 2), jaccard (u64), at size ratios
  |A| / |B| = 1, 4, 16, 64, 256 with |A| = 2^24 and 2^26 keys.
Every call is synchronous, so the host clock around it is the call time (kernels + the count's copy back); the median of `reps` warm
calls is reported, in ms and in millions of keys per second (both sets counted for Jaccard).  Writes one JSON file.
    setops128_bench.py [--out profiles/setops128_bench.json] [--log2 24 26] [--reps 7]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setops128_bench.json"))
ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
ctx = B.Context(0)
RATIOS = (1, 4, 16, 64, 256)
gen = torch.Generator(device="cuda").manual_seed(128)


def rand128(n, key_bits):
    t = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), dtype=torch.int64, device="cuda", generator=gen)
    if key_bits < 128:
        t[:, 1] &= (1 << (key_bits - 64)) - 1
    return t


def rand64(n):
    return torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=gen)


def median_ms(fn, before=None):
    times = []
    for i in range(args.reps + 1):  # the first call is the warm-up (scratch grows, code objects load)
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times[1:])


def rate(n_keys, ms, key_bytes=16):
    return {"ms": round(ms, 3), "Mkeys_s": round(n_keys / ms / 1e3, 1), "key_GB_s": round(n_keys * key_bytes / ms / 1e6, 1)}


def subset(a, na, ratio, fresh):
    """a sorted duplicate-free set of about na / ratio keys: every (2 * ratio)-th key of a, and as many fresh ones"""
    picked = a[:na][:: 2 * ratio]
    keys = torch.cat([picked, fresh(picked.shape[0])]).contiguous()
    return keys


read_gbps, copy_gbps = ctx.probe_hbm(1 << 30, 5)
out = {"reps": args.reps, "note": "median call time of warm synchronous calls; Mkeys_s and key_GB_s (keys x key bytes / call time) count the keys of both "
       "sets for jaccard; hbm_read_GB_s is the streaming-read rate of the same device (bl_probe_hbm)", "hbm_read_GB_s": round(read_gbps, 1), "sizes": {}}
for lg in args.log2:
    n = 1 << lg
    res = {}
    for bits in (82, 128):
        master = rand128(n, bits)
        work = torch.empty_like(master)
        res[f"sort_unique128_bits{bits}"] = rate(n, median_ms(lambda: ctx.sort_unique128(work, key_bits=bits), lambda: work.copy_(master)))
    m64 = rand64(n)
    w64 = torch.empty_like(m64)
    res["sort_unique_u64"] = rate(n, median_ms(lambda: ctx.sort_unique(w64), lambda: w64.copy_(m64)), 8)
    # the sets: A = the distinct keys of the last 128-bit master / the u64 master
    a128 = master
    na128 = ctx.sort_unique128(a128, key_bits=128)
    a64 = m64
    na64 = ctx.sort_unique(a64)
    del work, w64
    res["jaccard"] = {}
    for ratio in RATIOS:
        b128 = subset(a128, na128, ratio, lambda c: rand128(c, 128))
        nb128 = ctx.sort_unique128(b128, key_bits=128)
        b64 = subset(a64, na64, ratio, rand64)
        nb64 = ctx.sort_unique(b64)
        row = {"na": na128, "nb": nb128}
        answers = []
        for path, name in ((1, "merge"), (2, "search")):
            ctx.set_option("jaccard128_path", path)
            answers.append(ctx.jaccard128(a128, na128, b128, nb128))
            row[f"u128_{name}"] = rate(na128 + nb128, median_ms(lambda: ctx.jaccard128(a128, na128, b128, nb128)))
            # and with the small set first: the merge kernel is symmetric, the search kernel searches the larger set either way
            row[f"u128_{name}_swapped"] = rate(na128 + nb128, median_ms(lambda: ctx.jaccard128(b128, nb128, a128, na128)))
        ctx.set_option("jaccard128_path", 0)
        assert answers[0] == answers[1], "the two kernels disagree"
        row["intersection"] = answers[0][0]
        row["u64_search"] = rate(na64 + nb64, median_ms(lambda: ctx.jaccard(a64, na64, b64, nb64)), 8)
        row["faster_u128"] = "merge" if row["u128_merge"]["ms"] <= row["u128_search"]["ms"] else "search"
        res["jaccard"][f"ratio_{ratio}"] = row
        del b128, b64
    out["sizes"][f"2^{lg}"] = res
    del a128, a64, master, m64
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
