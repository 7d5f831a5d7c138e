#!/usr/bin/env python3
"""Rate of the 128-bit window-minimizer scan (bl_scan_minimizers128) beside unchanged yardsticks, measured in ONE process.

Synthetic 150-bp reads, one range of --gbp gigabases (default 1.5), canonical, records materialised.  After a warm-up round, --rounds
rounds (default 7) alternate
  bl_scan_minimizers128   (unit, w) = (33,11), (51,11), (64,11), (64,64), (33,2)
  bl_scan_hash_sample128  k = 51 with a threshold of 2 / (w + 1) of the hash range, w = 11, 64, 2: the same record density, one
                          8-multiply hash and one 128-bit canonical k-mer per position, no windows — THE yardstick of each shape
  bl_scan_kmers128        k = 51, digest only
  bl_scan_minimizers      (31,11) with exact_windows=1 and position_tiled=1: the 64-bit kernel deciding on whole hashes
the time of a scan is the device-event time bl_ctx_last_scan_ms reports.  Writes medians, the spread (min / max over the rounds) and the
ratio of every shape to each yardstick as JSON, stamped with the SHA-256 of the kernel sources.  There is no pass mark.

    python tests/perf/minimizers128_bench.py [--out profiles/minimizers128_rate.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SOURCES = ("bl_minimizers128.hip", "bl_minimizers128_core.hpp", "bl_scan128_launch.hpp", "bl_tile128.hpp", "bl_kmers128.hip", "bl_kmers128_core.hpp", "bl_kernels.hip",
           "bl_scan_core.hpp", "bl_scan_phases.hpp")
SHAPES = ((33, 11), (51, 11), (64, 11), (64, 64), (33, 2))


def sources_digest():
    h = hashlib.sha256()
    for name in SOURCES:
        h.update(name.encode())
        with open(os.path.join(ROOT, "biolib_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=1.5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minimizers128_rate.json"))
    a = ap.parse_args()
    assert a.rounds >= 5 and a.gbp >= 1.5, "at least 5 rounds over at least 1.5 Gbp"
    import torch

    import biolib_amd as B

    ctx = B.Context(0, torch_stream=False)
    n = int(a.gbp * 1e9) // 150 * 150
    batch = ctx.synth(42, n, 150)
    flags = B.FLAG_CANONICAL | B.FLAG_SYNC
    cap = int(n * 0.7)  # w = 2: two of three windows start a record
    values = torch.empty((cap, 2), dtype=torch.int64, device=ctx.torch_device)
    positions, hashes = ctx.empty_u64(cap), ctx.empty_u64(cap)
    torch.cuda.synchronize()

    def narrow():
        ctx.set_option("exact_windows", 1)
        ctx.set_option("position_tiled", 1)
        try:
            return batch.minimizers_raw(31, 11, 42, flags, 0, 0, values, positions, hashes, cap)
        finally:
            ctx.set_option("exact_windows", 0)
            ctx.set_option("position_tiled", 0)

    def sample(w):
        threshold = (2**64 - 1) * 2 // (w + 1)
        return lambda: batch.hash_sample128_raw(51, 42, threshold, flags, 0, 0, values, positions, hashes, cap)

    def wide(unit, w):
        return lambda: batch.minimizers128_raw(unit, w, 42, flags, 0, 0, values, positions, hashes, cap)

    configs = [("minimizers64_u31_w11_exact_position_tiled", narrow, dict(unit=31, w=11)),
               ("kmers128_k51_digest", lambda: batch.kmers128_raw(51, 42, flags, 0, 0, None, None, None), dict(k=51))]
    configs += [(f"hash_sample128_k51_density_w{w}", sample(w), dict(k=51, density=f"2/{w + 1}")) for w in (11, 64, 2)]
    configs += [(f"minimizers128_u{unit}_w{w}", wide(unit, w), dict(unit=unit, w=w)) for unit, w in SHAPES]
    times = {name: [] for name, _, _ in configs}
    digests = {}
    for rnd in range(a.rounds + 1):  # round 0 warms every shape up
        for name, run, _ in configs:
            r = run()
            ms = ctx.last_scan_ms()
            d = (int(r.count), int(r.xor_hash))
            assert digests.setdefault(name, d) == d and 0 < d[0] and (name.startswith("kmers") or d[0] <= cap), "a digest changed between runs, or the capacity is short"
            if rnd:
                times[name].append(ms)
    rows = {}
    for name, _, shape in configs:
        ms = times[name]
        med = statistics.median(ms)
        rows[name] = dict(shape, records=digests[name][0], median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                          Gbp_per_s=round(n / med / 1e6, 1), spread=round((max(ms) - min(ms)) / med, 4))
    for unit, w in SHAPES:
        row = rows[f"minimizers128_u{unit}_w{w}"]
        for key, other in (("ratio_to_hash_sample128_same_density", f"hash_sample128_k51_density_w{w}"), ("ratio_to_kmers128_k51_digest", "kmers128_k51_digest"),
                           ("ratio_to_minimizers64_u31_w11", "minimizers64_u31_w11_exact_position_tiled")):
            row[key] = round(rows[other]["median_ms"] / row["median_ms"], 3)
    out = dict(what="window-minimizer scans, 150-bp synthetic reads, canonical, records materialised, one lane, device-event time per scan; medians of the rounds",
               bases_per_scan=n, rounds=a.rounds, device=torch.cuda.get_device_name(0), kernel_sources=list(SOURCES), kernel_sources_sha256=sources_digest(), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
