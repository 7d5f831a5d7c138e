#!/usr/bin/env python3
"""What quality trimming costs on ONE GPU: bl_scan_read_quality with a fastp-like rule (window 4 at Q20, low_q 15 with 40 % allowed,
min_len 50) beside the two things a caller has without it.  About 1.5 Gbp per row, as 150-bp and as 10-kbp FASTQ whose reads have good
starts and, for a third of them, a degraded tail:
  quality_spans   the call with d_spans alone (asynchronous; the clock stops behind a synchronise)
  quality_full    the call with records, spans and statistics
  format          (a) bl_batch_format as FASTQ on the same batch and index into a buffer that exists: it reads the same bytes and writes them
  torch           (b) 150-bp rows only: a torch composition on the text seen as a matrix — the quality columns, cumulative sums, the first
                  failing window, the trailing walk and the two filters as masks.  Its spans are asserted equal to the call's first.
Timed with the host clock around calls that end in a device synchronise.  After one warm-up pass `rounds` passes are taken with the
variants INTERLEAVED; the median is reported with the spread (min .. max) beside it.  Useful bytes of the call: one quality byte and one
base byte per base, 2 * n_bases; the share is that rate over bl_probe_hbm's READ rate from the same run.
Clocks are not pinned: the card runs under its own power management, as in the other benches of this directory.
    quality_bench.py [--out profiles/quality_bench.json] [--gbp 1.5] [--rounds 3]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import biolib_amd as B
from biolib_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_bench.json"))
ap.add_argument("--gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(2026)
W, WQ, LOW_Q, LOW_NUM, LOW_DEN, MIN_LEN = 4, 20, 15, 2, 5, 50


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


def fastq_matrix(n, L):
    """n records "@r<10 digits>\\n<L bases>\\n+\\n<L qualities>\\n" as a uint8 device matrix [n, 17 + 2 L], made in slices"""
    width = 17 + 2 * L
    rec = torch.empty((n, width), dtype=torch.uint8, device="cuda")
    rec[:, 0], rec[:, 1] = ord("@"), ord("r")
    num = torch.arange(n, dtype=torch.int64, device="cuda")
    for d in range(10):
        rec[:, 11 - d] = (48 + num % 10).to(torch.uint8)
        num = num // 10
    rec[:, 12] = 10
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    pos = torch.arange(L, device="cuda")
    step = max(1, (256 << 20) // width)
    for a in range(0, n, step):
        b = min(n, a + step)
        rec[a:b, 13:13 + L] = letters[torch.randint(0, 4, (b - a, L), device="cuda", generator=gen)]
        q = torch.randint(30, 41, (b - a, L), device="cuda", generator=gen)
        tail = torch.where(torch.rand(b - a, device="cuda", generator=gen) < 1 / 3, torch.randint(L // 4, L, (b - a,), device="cuda", generator=gen), L)
        poor = torch.randint(2, 24, (b - a, L), device="cuda", generator=gen)
        q = torch.where(pos[None, :] >= tail[:, None], poor, q)
        rec[a:b, 16 + L:16 + 2 * L] = (q + 33).to(torch.uint8)
    rec[:, 13 + L], rec[:, 14 + L], rec[:, 15 + L], rec[:, 16 + 2 * L] = 10, ord("+"), 10, 10
    return rec


def torch_spans(rec, L):
    """the fastp-like rule as a torch composition on fixed-length records -> int64 [n, 2]"""
    v = (rec[:, 16 + L:16 + 2 * L].to(torch.int32) - 33).clamp_(0, 93)
    n = v.shape[0]
    c = torch.cumsum(v, dim=1, dtype=torch.int32)
    sums = c[:, W - 1:].clone()
    sums[:, 1:] -= c[:, :L - W]
    fail = sums < W * WQ
    any_fail = fail.any(dim=1)
    j = torch.where(any_fail, fail.to(torch.uint8).argmax(dim=1), L)
    pos = torch.arange(L, device=v.device)
    inside = pos[None, :] < j[:, None]
    keep = inside & (v >= WQ)
    walked = torch.where(keep, pos[None, :] + 1, 0).amax(dim=1)
    e = torch.where(any_fail, walked, L)
    n_low = ((pos[None, :] < e[:, None]) & (v < LOW_Q)).sum(dim=1)
    ok = (e >= MIN_LEN) & (n_low * LOW_DEN <= e * LOW_NUM)
    spans = torch.zeros((n, 2), dtype=torch.int64, device=v.device)
    spans[:, 1] = torch.where(ok, e, 0)
    return spans


rule = B.Batch.quality_rule(window=(W, WQ), low_q=LOW_Q, max_low=(LOW_NUM, LOW_DEN), min_len=MIN_LEN)
read_gbps, copy_gbps = ctx.probe_hbm(4 << 30, 3)
out = {"rounds": args.rounds, "gbp": args.gbp, "probe_hbm": {"read_GB_s": round(read_gbps, 1), "copy_GB_s": round(copy_gbps, 1)},
       "rule": "window 4 at Q20, low_q 15 with 2/5 allowed, min_len 50",
       "note": "interleaved rounds after one warm-up pass; median with min .. max beside it; host clock around calls that end in a synchronise; clocks not "
               "pinned; useful bytes of the call = 2 * n_bases (a quality byte and a base byte per base), share = that rate over probe_hbm's read rate",
       "rows": {}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

for L in (150, 10_000):
    n = int(args.gbp * 1e9) // L
    rec = fastq_matrix(n, L)
    host = rec.reshape(-1).cpu().numpy()
    batch, index = ctx.from_text_indexed(host)
    del host
    assert batch.n_seqs == n and batch.n_bases == n * L
    d_offsets = batch._device_offsets(None)
    records = torch.zeros((n, 6), dtype=torch.int64, device="cuda")
    spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    st = capi.QualityStats()
    frule = B.Batch.format_rule("fastq")
    n_bytes, _ = batch.format_raw(frule, None, 0, index=index, offsets=d_offsets)
    dest = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    batch.read_quality_raw(index, rule, records, spans, st)
    row = {"n_reads": n, "read_len": L, "n_bases": n * L, "text_bytes": int(rec.numel()), "stats": st.as_dict()}
    variants = {"quality_spans": lambda: batch.read_quality_raw(index, rule, None, spans, None),
                "quality_full": lambda: batch.read_quality_raw(index, rule, records, spans, st),
                "format": lambda: batch.format_raw(frule, dest, n_bytes, index=index, offsets=d_offsets)}
    if L == 150:
        theirs = torch_spans(rec, L)
        ctx.sync()
        assert torch.equal(theirs, spans), "the torch composition and the call disagree"
        row["torch_equals_call"] = True
        del theirs
        variants["torch"] = lambda: torch_spans(rec, L)
    times = interleaved(variants)
    for name, seconds in times.items():
        row[name] = stats(seconds)
        if name.startswith("quality"):
            rate = 2 * n * L / statistics.median(seconds) / 1e9
            row[name]["useful_GB_s"] = round(rate, 1)
            row[name]["share_of_read_rate"] = round(rate / read_gbps, 3)
            row[name]["Gbp_s"] = round(n * L / statistics.median(seconds) / 1e9, 1)
    out["rows"]["reads%s" % ("150" if L == 150 else "10k")] = row
    print(json.dumps(row), flush=True)
    index.close()
    batch.close()
    del rec, dest, records, spans
    torch.cuda.empty_cache()

with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
