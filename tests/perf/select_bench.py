#!/usr/bin/env python3
"""What bl_batch_select costs on ONE GPU, against what a caller writes in torch without it, and how far its gather kernel is from the
card's copy rate.  About 1.5 Gbp of synthetic reads per row, the spans made on the device beforehand:
  reads150_half_whole    150-bp fixed-length reads, a random half kept whole (the result is a fixed-length batch again)
  reads150_prefix_trim   the same reads, every one cut to a random prefix of 0 .. 150 bases (seams every 75 bytes of the result)
  reads10k_trimmed       ragged reads of 5 .. 15 kbp, each cut to a random prefix of at least half its length
  reads150_keep_empty    the first row with BL_SELECT_KEEP_EMPTY (the result carries the dropped reads as empty sequences)
Variants per row, timed with the host clock around calls that end in a device synchronise:
  select        Batch.select: the call, the download of the new offsets and the new Batch
  select_raw    bl_batch_select alone (Batch.select_raw)
  torch         the composition a caller has today: an index tensor from repeat_interleave and arange (eight bytes per base), a gather with
                it, and Context.from_tensor on the gathered bases (with the host offsets, or read_len for the first row)
The results of select and torch are compared byte for byte inside the script.  After one warm-up pass over all variants, `rounds` passes
are taken with the variants INTERLEAVED; the median is reported with the spread (min .. max) beside it.  `beats` compares whole spreads:
true only when the slower end of one lies below the faster end of the other.
The gather kernel alone is not timed by the host clock.  It comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python select_bench.py --kernel-pass
    select_bench.py --kernel-trace DIR/p_kernel_trace.csv        (the timed run; merges the trace's gather_kernel times, row by row)
Useful bytes of the gather: every result byte read once and written once, 2 * n_bases_out; the share is that rate over bl_probe_hbm's copy
rate (which counts read + write bytes too) on the same card.  Without a trace the kernel's figures say "not measured".
    select_bench.py [--out profiles/select_bench.json] [--gbp 1.5] [--rounds 5] [--kernel-pass] [--kernel-trace FILE]"""
import argparse, csv, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import biolib_amd as B

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
ap.add_argument("--gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--kernel-pass", action="store_true", help="three select_raw calls per row and nothing else: the run to trace")
ap.add_argument("--kernel-trace", default=None, help="kernel_trace.csv of a --kernel-pass run")
args = ap.parse_args()
KERNEL_PASS_CALLS = 3
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(2026)
ACGT = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")


def random_bases(n):
    return ACGT[torch.randint(0, 4, (n,), device="cuda", generator=gen)]


def interleaved(variants):
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


def stats(seconds):
    return {"ms_median": round(statistics.median(seconds) * 1e3, 3), "ms_min": round(min(seconds) * 1e3, 3), "ms_max": round(max(seconds) * 1e3, 3)}


def rows():
    """name -> (bases tensor, host offsets or None, read_len, spans tensor [n, 2], keep_empty)"""
    n_reads = int(args.gbp * 1e9) // 150
    short = random_bases(n_reads * 150)
    whole = torch.zeros((n_reads, 2), dtype=torch.int64, device="cuda")
    whole[:, 1] = torch.where(torch.rand(n_reads, device="cuda", generator=gen) < 0.5, 150, 0)
    prefix = torch.zeros((n_reads, 2), dtype=torch.int64, device="cuda")
    prefix[:, 1] = torch.randint(0, 151, (n_reads,), device="cuda", generator=gen)
    yield "reads150_half_whole", short, None, 150, whole, False
    yield "reads150_prefix_trim", short, None, 150, prefix, False
    yield "reads150_keep_empty", short, None, 150, whole, True
    del short, whole, prefix
    n_long = int(args.gbp * 1e9) // 10_000
    lengths = torch.randint(5_000, 15_001, (n_long,), device="cuda", generator=gen)
    offsets = np.concatenate([[0], lengths.cumsum(0).cpu().numpy()]).astype(np.uint64)
    spans = torch.zeros((n_long, 2), dtype=torch.int64, device="cuda")
    spans[:, 1] = lengths // 2 + (torch.rand(n_long, device="cuda", generator=gen) * (lengths - lengths // 2 + 1)).long()
    yield "reads10k_trimmed", random_bases(int(offsets[-1])), offsets, 0, spans, False


def torch_composition(bases, d_offsets, spans, keep_empty, fixed_result):
    """what a caller has today -> (Batch, gathered tensor)"""
    L = d_offsets[1:] - d_offsets[:-1]
    b, e = torch.minimum(spans[:, 0], L), torch.minimum(spans[:, 1], L)
    n = (e - b).clamp(min=0)
    keep = torch.ones_like(n, dtype=torch.bool) if keep_empty else n > 0
    n, start = n[keep], (d_offsets[:-1] + b)[keep]
    out_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=n.device), n.cumsum(0)])
    total = int(out_offsets[-1])
    index = torch.repeat_interleave(start - out_offsets[:-1], n, output_size=total) + torch.arange(total, device=n.device)
    gathered = bases[index]
    if fixed_result:
        return ctx.from_tensor(gathered, read_len=fixed_result), gathered
    return ctx.from_tensor(gathered, offsets=out_offsets.cpu().numpy().astype(np.uint64)), gathered


def gather_times(path):
    """the durations (ms) of the gather kernel's launches in a --kernel-pass trace, in launch order"""
    found = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "gather_kernel" in r["Kernel_Name"] and "blsel" in r["Kernel_Name"]:
                found.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return [ms for _, ms in sorted(found)]


traced = gather_times(args.kernel_trace) if args.kernel_trace else None
out = {"rounds": args.rounds, "gbp": args.gbp,
       "note": "interleaved rounds after one warm-up pass; median with min .. max beside it; gather_kernel from a rocprofv3 kernel trace of a "
               "separate --kernel-pass run (median of %d launches per row), 'not measured' without one" % KERNEL_PASS_CALLS, "rows": {}}
if not args.kernel_pass:
    read_gbps, copy_gbps = ctx.probe_hbm(4 << 30, 3)
    out["probe_hbm"] = {"read_GB_s": round(read_gbps, 1), "copy_GB_s": round(copy_gbps, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

for row_no, (name, bases, offsets, read_len, spans, keep_empty) in enumerate(rows()):
    src = ctx.from_tensor(bases, offsets=offsets, read_len=read_len)
    n_seqs = src.n_seqs
    d_offsets = torch.from_numpy(offsets.view(np.int64)).cuda() if offsets is not None else torch.arange(n_seqs + 1, device="cuda") * read_len
    flags = 1 if keep_empty else 0
    raw_offsets = torch.zeros(n_seqs + 1, dtype=torch.int64, device="cuda")
    raw_index = torch.zeros(n_seqs, dtype=torch.int64, device="cuda")
    keep = {}

    def select_raw():
        h, keep["n_out"], keep["n_bases_out"] = src.select_raw(spans, flags, src._device_offsets(None), raw_offsets, raw_index)
        B.Batch(ctx, h).close()

    if args.kernel_pass:
        for _ in range(KERNEL_PASS_CALLS):
            select_raw()
        print(name, keep, flush=True)
        src.close()
        continue

    def select():
        if "new" in keep:
            keep.pop("new").close()
        keep["new"], keep["index"] = src.select(spans, keep_empty=keep_empty)

    fixed_result = 150 if name == "reads150_half_whole" else 0

    def composition():
        if "ref" in keep:
            keep.pop("ref").close()
        keep["ref"], keep["gathered"] = torch_composition(bases, d_offsets, spans, keep_empty, fixed_result)

    t = interleaved({"select": select, "select_raw": select_raw, "torch": composition})
    new, ref = keep["new"], keep["ref"]
    assert (new.n_bases, new.n_seqs) == (ref.n_bases, ref.n_seqs), "the two results differ in size"
    assert new.read_len == fixed_result, "the result's fixed length"
    mine = torch.from_numpy(new.download()).cuda()
    assert torch.equal(mine, keep["gathered"]), "the selected bases differ from torch's gather"
    res = {v: stats(s) for v, s in t.items()}
    n_out_bases = new.n_bases
    res.update(reads=n_seqs, bases=src.n_bases, reads_out=new.n_seqs, bases_out=n_out_bases, useful_bytes=2 * n_out_bases, keep_empty=keep_empty,
               result_read_len=new.read_len)
    for v in ("select", "select_raw"):
        res[v]["useful_GB_s"] = round(2 * n_out_bases / statistics.median(t[v]) / 1e9, 1)
        res[v + "_beats_torch"] = bool(res[v]["ms_max"] < res["torch"]["ms_min"])
    res["torch_over_select"] = round(res["torch"]["ms_median"] / res["select"]["ms_median"], 2)
    if traced and len(traced) >= KERNEL_PASS_CALLS * (row_no + 1):
        ms = traced[KERNEL_PASS_CALLS * row_no:KERNEL_PASS_CALLS * (row_no + 1)]
        rate = 2 * n_out_bases / (statistics.median(ms) / 1e3) / 1e9
        res["gather_kernel"] = {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                                "useful_GB_s": round(rate, 1), "share_of_copy_rate": round(rate / copy_gbps, 3)}
    else:
        res["gather_kernel"] = "not measured"
    out["rows"][name] = res
    print(json.dumps({name: res}), flush=True)
    with open(args.out, "w") as f:  # after every row: a run cut short keeps what it measured
        json.dump(out, f, indent=1)
        f.write("\n")
    for x in (keep.pop("new"), keep.pop("ref"), src):
        x.close()
    del keep, mine, raw_offsets, raw_index
    torch.cuda.empty_cache()
