#!/usr/bin/env python3
"""What adapter trimming costs on ONE GPU: bl_scan_read_adapters, spans only, beside three yardsticks on the same batch.  About 1.5 Gbp per
row, as FASTQ (the quality yardstick needs the index):
  paired150   150-bp interleaved mates; in a quarter of the pairs an insert of 20 .. 149 bases is read through into TruSeq (the other
              pairs are unrelated reads, which makes step 2 try every insert size); TruSeq as the adapter, poly-G after it, min_len 25
  single150   the same reads as single reads with one adapter (TruSeq) ...
  eight150    ... and with eight (the three of biolib_amd.ADAPTERS and five random ones of 20 .. 64 bases)
  single10k   10-kbp reads, TruSeq written at a random place of a quarter of them, one adapter
Beside each row:
  quality     (a) bl_scan_read_quality with a fastp-like rule (window 4 at Q20, min_len 50), spans only
  kmers31     (b) bl_scan_kmers at k = 31, canonical, digest only: a known instruction-bound scan
  torch       (c) single150 only: a torch composition of step 3 on the bases seen as a matrix (mismatch counts by a loop over the
              adapter's bases, the best candidate as a packed key).  Its spans are asserted equal to the call's before anything is timed.
Timed with the host clock around calls that end in a device synchronise.  After one warm-up pass `rounds` passes are taken with the
variants INTERLEAVED; the median is reported with the whole spread (min .. max) beside it.  Clocks are not pinned: the card runs under its
own power management, as in the other benches of this directory.  No counter run is made here: what binds the kernel is not measured.
    adapter_bench.py [--out profiles/adapter_bench.json] [--gbp 1.5] [--rounds 3]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import biolib_amd as B
from biolib_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapter_bench.json"))
ap.add_argument("--gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(2027)
TRUSEQ = B.ADAPTERS["truseq"]
PLANTED = 0.25
LETTERS = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")


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


def fastq_matrix(n, L, paired):
    """n records "@r<10 digits>\\n<L bases>\\n+\\n<L qualities>\\n" as a uint8 device matrix [n, 17 + 2 L], made in slices"""
    width = 17 + 2 * L
    rec = torch.empty((n, width), dtype=torch.uint8, device="cuda")
    rec[:, 0], rec[:, 1] = ord("@"), ord("r")
    num = torch.arange(n, dtype=torch.int64, device="cuda")
    for d in range(10):
        rec[:, 11 - d] = (48 + num % 10).to(torch.uint8)
        num = num // 10
    rec[:, 12] = 10
    pos = torch.arange(L, device="cuda")
    adapter = torch.tensor([b"ACGT".index(c) for c in TRUSEQ.encode()], device="cuda")
    A = len(adapter)
    step = max(2, ((256 << 20) // width) & ~1)
    for a in range(0, n, step):
        b = min(n, a + step)
        m = b - a
        codes = torch.randint(0, 4, (m, L), device="cuda", generator=gen)
        if paired:  # mates 2j, 2j + 1: the first I bases of the second are the reverse complement of the first I of the first, then the adapter
            half = m // 2
            I = torch.where(torch.rand(half, device="cuda", generator=gen) < PLANTED, torch.randint(20, L, (half,), device="cuda", generator=gen), 2 * L)
            r1, r2 = codes[0::2], codes[1::2]
            back = (I[:, None] - 1 - pos[None, :]).clamp(0, L - 1)
            r2[:] = torch.where(pos[None, :] < I[:, None], 3 - r1.gather(1, back), r2)
            in_adapter = (pos[None, :] >= I[:, None]) & (pos[None, :] < I[:, None] + A)
            letter = adapter[(pos[None, :] - I[:, None]).clamp(0, A - 1)]
            r1[:] = torch.where(in_adapter, letter, r1)
            r2[:] = torch.where(in_adapter, letter, r2)
        else:
            at = torch.where(torch.rand(m, device="cuda", generator=gen) < PLANTED, torch.randint(0, L, (m,), device="cuda", generator=gen), 2 * L)
            in_adapter = (pos[None, :] >= at[:, None]) & (pos[None, :] < at[:, None] + A)
            codes = torch.where(in_adapter, adapter[(pos[None, :] - at[:, None]).clamp(0, A - 1)], codes)
        rec[a:b, 13:13 + L] = LETTERS[codes]
        q = torch.randint(30, 41, (m, L), device="cuda", generator=gen)
        tail = torch.where(torch.rand(m, device="cuda", generator=gen) < 1 / 3, torch.randint(L // 4, L, (m,), device="cuda", generator=gen), L)
        q = torch.where(pos[None, :] >= tail[:, None], torch.randint(2, 24, (m, L), device="cuda", generator=gen), q)
        rec[a:b, 16 + L:16 + 2 * L] = (q + 33).to(torch.uint8)
        del codes, q
    rec[:, 13 + L], rec[:, 14 + L], rec[:, 15 + L], rec[:, 16 + 2 * L] = 10, ord("+"), 10, 10
    return rec


def torch_spans(rec, L, adapter, min_overlap, num, den):
    """step 3 for one adapter on fixed-length reads of valid bases, as a torch composition -> int64 [n, 2]"""
    bases = rec[:, 13:13 + L]
    n, A = bases.shape[0], len(adapter)
    m = torch.zeros((n, L), dtype=torch.int16, device=bases.device)
    for j, ch in enumerate(adapter):
        m[:, :L - j] += (bases[:, j:] != ch).to(torch.int16)
    pos = torch.arange(L, device=bases.device)
    o = torch.clamp(L - pos, max=A).to(torch.int16)
    ok = (m.to(torch.int32) * den <= o.to(torch.int32)[None, :] * num) & (pos[None, :] <= L - min(min_overlap, A))
    key = torch.where(ok, (o[None, :] - m + 1).to(torch.int32) * 256 + (L - 1 - pos)[None, :].to(torch.int32), 0).amax(dim=1)
    e = torch.where(key > 0, L - 1 - key % 256, L)
    spans = torch.zeros((n, 2), dtype=torch.int64, device=bases.device)
    spans[:, 1] = e
    return spans


rng = np.random.default_rng(5)
EIGHT = list(B.ADAPTERS.values()) + ["".join(rng.choice(list("ACGT"), int(k))) for k in (20, 33, 64, 47, 25)]
q_rule = B.Batch.quality_rule(window=(4, 20), min_len=50)
read_gbps, copy_gbps = ctx.probe_hbm(4 << 30, 3)
out = {"rounds": args.rounds, "gbp": args.gbp, "probe_hbm": {"read_GB_s": round(read_gbps, 1), "copy_GB_s": round(copy_gbps, 1)},
       "planted_fraction": PLANTED, "eight_adapters": EIGHT,
       "note": "interleaved rounds after one warm-up pass; median with min .. max beside it; host clock around calls that end in a synchronise; clocks not "
               "pinned; every adapter call writes spans only; no counter run: what binds the kernel is not measured",
       "rows": {}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def measure(name, batch, index, rec, L, rule, with_torch=False):
    n = batch.n_seqs
    spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    q_spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    st = capi.AdapterStats()
    d_offsets = batch._device_offsets(None)
    torch.cuda.synchronize()
    batch.read_adapters_raw(rule, None, spans, st, None, d_offsets)
    row = {"n_reads": n, "read_len": L, "n_bases": n * L, "stats": st.as_dict()}
    variants = {"adapters": lambda: batch.read_adapters_raw(rule, None, spans, None, None, d_offsets),
                "quality": lambda: batch.read_quality_raw(index, q_rule, None, q_spans, None),
                "kmers31": lambda: batch.kmers(31, 42, canonical=True, arrays=False)}
    if with_torch:
        theirs = torch_spans(rec, L, TRUSEQ.encode(), rule.min_overlap, rule.error_num, rule.error_den)
        ctx.sync()
        assert torch.equal(theirs, spans), "the torch composition and the call disagree"
        row["torch_equals_call"] = True
        del theirs
        variants["torch"] = lambda: torch_spans(rec, L, TRUSEQ.encode(), rule.min_overlap, rule.error_num, rule.error_den)
    for vname, seconds in interleaved(variants).items():
        row[vname] = stats(seconds)
        row[vname]["Gbp_s"] = round(n * L / statistics.median(seconds) / 1e9, 1)
    out["rows"][name] = row
    print(name, json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


for L in (150, 10_000):
    n = (int(args.gbp * 1e9) // L) & ~1
    rec = fastq_matrix(n, L, paired=L == 150)
    host = rec.reshape(-1).cpu().numpy()
    batch, index = ctx.from_text_indexed(host)
    del host
    assert batch.n_seqs == n and batch.n_bases == n * L
    if L == 150:
        measure("paired150", batch, index, rec, L, B.Batch.adapter_rule([TRUSEQ], paired=True, poly_after="G", min_len=25))
        measure("single150", batch, index, rec, L, B.Batch.adapter_rule([TRUSEQ]), with_torch=True)
        measure("eight150", batch, index, rec, L, B.Batch.adapter_rule(EIGHT))
    else:
        measure("single10k", batch, index, rec, L, B.Batch.adapter_rule([TRUSEQ]))
    index.close()
    batch.close()
    del rec
    torch.cuda.empty_cache()
print("wrote", args.out)
