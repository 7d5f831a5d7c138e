#!/usr/bin/env python3
"""Rate of the 128-bit syncmer scan (bl_scan_syncmers128) beside unchanged yardsticks, measured in ONE process.

Synthetic 150-bp reads, one range of --gbp gigabases (default 1.5), canonical, positions materialised.  After a warm-up round, --rounds
rounds (default 7) alternate
  bl_scan_syncmers128  (k, s) = (33,11), (51,21), (64,32) with closed offsets {0, W-1}, and (64,1) with {0, 63}
  bl_scan_syncmers     (31,15,{0,16})                       the generic exact form of the 64-bit kernel — THE yardstick of the ratios
  bl_scan_syncmers     (31,11,{0,20}) with exact_windows=1  the 64-bit kernel deciding on whole hashes
  bl_scan_kmers128     k = 51, digest only                  one 8-multiply hash and one 128-bit canonical k-mer per position
the time of a scan is the device-event time bl_ctx_last_scan_ms reports.  Writes medians, the ratio of every row to the (31,15)
yardstick, the spread (min / max over the rounds) and the W-dependence (64,1) : (64,32) as JSON, stamped with the SHA-256 of the
kernel sources.  There is no pass mark.

    python tests/perf/syncmers128_bench.py [--out profiles/syncmers128_rate.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SOURCES = ("bl_syncmers128.hip", "bl_syncmers128_core.hpp", "bl_scan128_launch.hpp", "bl_tile128.hpp", "bl_kmers128.hip", "bl_kmers128_core.hpp", "bl_kernels.hip",
           "bl_scan_core.hpp", "bl_scan_phases.hpp")
YARDSTICK = "syncmers64_k31_s15"


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syncmers128_rate.json"))
    a = ap.parse_args()
    assert a.rounds >= 5 and a.gbp >= 1.5, "at least 5 rounds over at least 1.5 Gbp"
    import torch

    import biolib_amd as B

    ctx = B.Context(0, torch_stream=False)
    n = int(a.gbp * 1e9) // 150 * 150
    batch = ctx.synth(42, n, 150)
    flags = B.FLAG_CANONICAL | B.FLAG_SYNC
    cap = n // 4  # closed syncmers: about 2 / W of the k-mers, W >= 17 here
    positions = ctx.empty_u64(cap)
    torch.cuda.synchronize()

    def wide(k, s, a0, a1):
        return lambda: batch.syncmers128_raw(k, s, a0, a1, 42, flags, 0, 0, positions, cap)

    def narrow(k, s, a0, a1, exact):
        def run():
            ctx.set_exact_windows(exact)
            try:
                return batch.syncmers_raw(k, s, a0, a1, 42, flags, 0, 0, positions, cap)
            finally:
                ctx.set_exact_windows(False)
        return run

    configs = [
        (YARDSTICK, narrow(31, 15, 0, 16, False), dict(k=31, s=15, w=17)),
        ("syncmers64_k31_s11_exact_windows", narrow(31, 11, 0, 20, True), dict(k=31, s=11, w=21)),
        ("kmers128_k51_digest", lambda: batch.kmers128_raw(51, 42, flags, 0, 0, None, None, None), dict(k=51)),
        ("syncmers128_k33_s11", wide(33, 11, 0, 22), dict(k=33, s=11, w=23)),
        ("syncmers128_k51_s21", wide(51, 21, 0, 30), dict(k=51, s=21, w=31)),
        ("syncmers128_k64_s32", wide(64, 32, 0, 32), dict(k=64, s=32, w=33)),
        ("syncmers128_k64_s1", wide(64, 1, 0, 63), dict(k=64, s=1, w=64)),
    ]
    times = {name: [] for name, _, _ in configs}
    digests = {}
    for rnd in range(a.rounds + 1):  # round 0 warms every shape up
        for name, run, _ in configs:
            r = run()
            ms = ctx.last_scan_ms()
            d = (int(r.count), int(r.xor_pos))
            assert digests.setdefault(name, d) == d and 0 < d[0] and (name.startswith("kmers") or d[0] <= cap), "a digest changed between runs, or the capacity is short"
            if rnd:
                times[name].append(ms)
    rows = {}
    for name, _, shape in configs:
        ms = times[name]
        med = statistics.median(ms)
        rows[name] = dict(shape, records=digests[name][0], median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                          Gbp_per_s=round(n / med / 1e6, 1), spread=round((max(ms) - min(ms)) / med, 4))
    for name in rows:
        rows[name]["ratio_to_" + YARDSTICK] = round(rows[YARDSTICK]["median_ms"] / rows[name]["median_ms"], 3)
    out = dict(what="syncmer scans, 150-bp synthetic reads, canonical, positions materialised, one lane, device-event time per scan; medians of the rounds",
               bases_per_scan=n, rounds=a.rounds, device=torch.cuda.get_device_name(0), yardstick=YARDSTICK,
               w_dependence_k64_s1_over_k64_s32=round(rows["syncmers128_k64_s1"]["median_ms"] / rows["syncmers128_k64_s32"]["median_ms"], 3),
               kernel_sources=list(SOURCES), kernel_sources_sha256=sources_digest(), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
