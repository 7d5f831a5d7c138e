#!/usr/bin/env python3
"""Rate of the 128-bit dense k-mer scan (bl_scan_kmers128) beside the unchanged 64-bit one, measured in ONE process.

Synthetic 150-bp reads, one range of --gbp gigabases (default 1.5).  After a warm-up round, --rounds rounds (default 7) alternate
  bl_scan_kmers     k = 31 canonical            (the yardstick: the existing kernel)
  bl_scan_kmers128  k = 33, 51, 64 canonical
each digest-only and with all three arrays; the time of a scan is the device-event time bl_ctx_last_scan_ms reports.  Writes medians,
ratios to the yardstick and the spread (min / max over the rounds) as JSON, stamped with the SHA-256 of the kernel sources.
With arrays the 128-bit scan stores 25 bytes per base (16 value + 8 hash + 1 valid) and the 64-bit one 17: the store rate is reported
against the device's measured copy rate (bl_probe_hbm) and the bound that applies is named.  There is no pass mark.

    python tests/perf/kmers128_bench.py [--out profiles/kmers128_rate.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SOURCES = ("bl_kmers128.hip", "bl_kmers128_core.hpp", "bl_scan128_launch.hpp", "bl_tile128.hpp", "bl_kernels.hip", "bl_scan_core.hpp", "bl_scan_phases.hpp")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmers128_rate.json"))
    a = ap.parse_args()
    assert a.rounds >= 5 and a.gbp >= 1.5, "at least 5 rounds over at least 1.5 Gbp"
    import torch

    import biolib_amd as B

    ctx = B.Context(0, torch_stream=False)
    n = int(a.gbp * 1e9) // 150 * 150
    batch = ctx.synth(42, n, 150)
    flags = B.FLAG_CANONICAL | B.FLAG_SYNC
    values = torch.empty((n, 2), dtype=torch.int64, device=ctx.torch_device)  # the 64-bit scan uses the first n words of it
    hashes, valid = ctx.empty_u64(n), ctx.empty_u8(n)
    torch.cuda.synchronize()
    configs = [("kmers64_k31", 31, False)] + [(f"kmers128_k{k}", k, True) for k in (33, 51, 64)]
    times = {(name, arrays): [] for name, _, _ in configs for arrays in (False, True)}
    digests = {}
    for rnd in range(a.rounds + 1):  # round 0 warms every shape up
        for arrays in (False, True):
            for name, k, wide in configs:
                out = (values, hashes, valid) if arrays else (None, None, None)
                r = (batch.kmers128_raw if wide else batch.kmers_raw)(k, 42, flags, 0, 0, *out)
                ms = ctx.last_scan_ms()
                d = (int(r.count), int(r.xor_value), int(r.aux), int(r.xor_hash), int(r.xor_pos))
                assert digests.setdefault(name, d) == d and d[0] > 0, "a digest changed between runs"
                if rnd:
                    times[(name, arrays)].append(ms)
    read_gbps, copy_gbps = ctx.probe_hbm(4 << 30, 3)
    rows = {}
    for (name, arrays), ms in times.items():
        med = statistics.median(ms)
        row = dict(median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), Gbp_per_s=round(n / med / 1e6, 1),
                   spread=round((max(ms) - min(ms)) / med, 4))
        if arrays:
            per_base = 25 if name.startswith("kmers128") else 17
            row.update(store_bytes_per_base=per_base, store_GB_per_s=round(per_base * n / med / 1e6, 1))
            row["share_of_measured_copy_rate"] = round(row["store_GB_per_s"] / copy_gbps, 3)
        rows[name + ("_arrays" if arrays else "_digest")] = row
    for name, _, wide in configs:
        if wide:
            for kind in ("digest", "arrays"):
                rows[f"{name}_{kind}"]["ratio_to_kmers64_k31"] = round(rows[f"kmers64_k31_{kind}"]["median_ms"] / rows[f"{name}_{kind}"]["median_ms"], 3)
            dg, ar = rows[name + "_digest"], rows[name + "_arrays"]
            # stores cost nothing extra when the scan with arrays runs at the digest-only rate: then the instruction issue of hashing binds
            ar["bound"] = ("HBM stores" if ar["median_ms"] > 1.1 * dg["median_ms"] and ar["share_of_measured_copy_rate"] > 0.5
                           else ("VALU issue (the rate of the digest-only scan)" if ar["median_ms"] <= 1.1 * dg["median_ms"] else "the store pattern: a lane owns 16 consecutive positions, so one store instruction writes 64 pieces 16 positions apart (the 64-bit kernel's "
                                 "layout too) - neither HBM bandwidth nor VALU issue"))
    out = dict(what="dense k-mer scans, 150-bp synthetic reads, canonical, one lane, device-event time per scan; medians of the rounds",
               bases_per_scan=n, rounds=a.rounds, device=torch.cuda.get_device_name(0), hbm_probe_GB_per_s=dict(read=round(read_gbps, 1), copy=round(copy_gbps, 1)),
               kernel_sources=list(SOURCES), kernel_sources_sha256=sources_digest(), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
