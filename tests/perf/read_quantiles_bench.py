#!/usr/bin/env python3
"""What the per-read median of bl_select_read_counts costs beside the scan that feeds it, and against what a caller writes in torch
without it, on ONE GPU.  The batches and tables of read_counts_bench.py: synthetic reads (150 bp, and 10 kbp) against tables of random
distinct 62-bit keys (k = 31) of 2^22 and 2^26 entries.  Variants per (read length, table), all over the SAME chunks (Batch.read_medians'
default, cut on read boundaries):
  read_medians        Batch.read_medians: per chunk bl_scan_kmer_counts into one reused pair of buffers, then bl_select_read_counts;
  kmer_counts         the scans alone;
  then_torch_rows     the scans, each followed by the cheapest torch form, open to reads of ONE length only: a [reads, read_len] view with
                      the invalid positions masked to the top, torch.sort(dim=1) and a gather at the rank;
  then_torch_ragged   the scans, each followed by the form ragged reads need: one global torch.sort of (sequence << 32 | count) keys
                      and a gather at offset + rank.
  select_scan         bl_select_read_counts alone over the last chunk as the scan left it.  A table of RANDOM keys holds next to none of
                      the reads' k-mers: nearly every count is 0, and a sequence whose counts are all 0 is answered after the load.
  select_small        the same call over the same chunk with the counts replaced by random values below 1,000 — what a real table gives:
                      the narrowing runs its ten bits.
The medians of the first four are compared with each other inside the script.  Every call is synchronous, so the host clock around it
is the call time.  After one warm-up pass over all variants, `rounds` passes are taken with the variants INTERLEAVED; the median is
reported with the spread (min .. max) beside it.  `beats` compares whole spreads: true only when the slower end of one lies above the
faster end of the other.  What binds the kernels is not measured here (no counter run).  Writes one JSON file.
    read_quantiles_bench.py [--out profiles/read_quantiles_bench.json] [--log2 22 26] [--read-len 150 10000] [--scan-gbp 1.5] [--rounds 3]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B
from biolib_amd.scan import _flags

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_quantiles_bench.json"))
ap.add_argument("--log2", type=int, nargs="*", default=[22, 26])
ap.add_argument("--read-len", type=int, nargs="*", default=[150, 10000])
ap.add_argument("--scan-gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(4096)
K, KEY_BITS = 31, 62
U32 = (1 << 32) - 1
MEDIAN = ((1, 2),)


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
    return {"ms_median": round(statistics.median(seconds) * 1e3, 3), "ms_min": round(min(seconds) * 1e3, 3), "ms_max": round(max(seconds) * 1e3, 3),
            unit: round(statistics.median(rates), 3), unit + "_min": round(rates[0], 3), unit + "_max": round(rates[-1], 3)}


def beats(new, base, unit):
    return bool(new[unit + "_min"] > base[unit + "_max"])


def torch_rows(counts, valid, n_reads, read_len):
    """medians along the rows of a [reads, read_len] view: invalid positions sort to the top"""
    v = valid.view(n_reads, read_len) != 0
    c = torch.where(v, counts.view(n_reads, read_len).to(torch.int64) & U32, 1 << 40)
    m = v.sum(1)
    med = torch.sort(c, dim=1).values.gather(1, (m // 2).clamp(max=read_len - 1).unsqueeze(1)).squeeze(1)
    return torch.where(m > 0, med, 0)


def torch_ragged(counts, valid, seq_ids, n_reads):
    """medians of ragged reads: one global sort of (sequence << 32 | count) over the valid positions"""
    v = valid != 0
    keys = ((seq_ids[v] << 32) | (counts[v].to(torch.int64) & U32)).sort().values
    m = torch.zeros(n_reads, dtype=torch.int64, device=counts.device).index_add_(0, seq_ids[v], torch.ones_like(keys))
    start = torch.cumsum(m, 0) - m
    at = (start + m // 2).clamp(max=max(keys.numel() - 1, 0))
    return torch.where(m > 0, keys[at] & U32, 0)


def bench(table, lg, read_len):
    n_bases = int(args.scan_gbp * 1e9) // read_len * read_len
    n_reads = n_bases // read_len
    b = ctx.synth(7, n_bases, read_len)
    assert b.n_seqs == n_reads
    chunks = b._sequence_chunks(None, b.QUANTILE_CHUNK)
    widest = max(e - s for s, e in chunks)
    counts = torch.empty(widest, dtype=torch.int32, device="cuda")
    valid = torch.empty(widest, dtype=torch.uint8, device="cuda")
    flags = _flags(False, False, True)
    keep = {}

    def read_medians():
        keep["medians"] = b.read_medians(table, K)

    def scans(after=None):
        out = []
        for s, e in chunks:
            b.kmer_counts_raw(table, K, flags, s, e - s, counts, valid)
            if after:
                out.append(after(s, e))
        return out

    def then_torch_rows():
        keep["rows"] = torch.cat(scans(lambda s, e: torch_rows(counts[:e - s], valid[:e - s], (e - s) // read_len, read_len)))

    def then_torch_ragged():
        def after(s, e):
            ids = torch.arange(e - s, device="cuda") // read_len
            return torch_ragged(counts[:e - s], valid[:e - s], ids, (e - s) // read_len)
        keep["ragged"] = torch.cat(scans(after))

    # the selection alone, over the last chunk
    s_last, e_last = chunks[-1]
    span = e_last - s_last
    small = torch.randint(0, 1000, (span,), dtype=torch.int32, device="cuda", generator=gen)
    out_q = torch.zeros(n_reads, dtype=torch.int32, device="cuda")

    def select_scan():
        b.select_read_counts_raw(counts, valid, MEDIAN, out_q, None, s_last, span)

    def select_small():
        b.select_read_counts_raw(small, valid, MEDIAN, out_q, None, s_last, span)

    st = interleaved({"read_medians": read_medians, "kmer_counts": scans, "then_torch_rows": then_torch_rows, "then_torch_ragged": then_torch_ragged})
    mine = keep["medians"].to(torch.int64) & U32
    assert torch.equal(mine, keep["rows"]), "the medians differ from the row sort's"
    assert torch.equal(mine, keep["ragged"]), "the medians differ from the global sort's"
    b.kmer_counts_raw(table, K, flags, s_last, span, counts, valid)  # (the last chunk's arrays, as every variant above left them)
    st_sel = interleaved({"select_scan": select_scan, "select_small": select_small})
    first_read = s_last // read_len
    want = torch_rows(small, valid[:span], span // read_len, read_len)
    assert torch.equal(out_q[first_read:].to(torch.int64) & U32, want), "select_small differs from the row sort"
    res = {name: row(s, n_bases, "Gbp_s") for name, s in st.items()}
    res.update({name: row(s, span, "Gpos_s") for name, s in st_sel.items()})
    for name in st_sel:
        res[name]["GB_s_read"] = round(res[name]["Gpos_s"] * 5, 1)  # five bytes per position, once (the workgroup form: once per pass)
    res.update(bases=n_bases, reads=n_reads, read_len=read_len, table_entries=table.n_distinct, chunks=len(chunks), chunk_positions=widest,
               select_positions=span, nonzero_medians=int((mine != 0).sum()))
    res["selection_share_ms"] = round(res["read_medians"]["ms_median"] - res["kmer_counts"]["ms_median"], 3)
    res["read_medians_beats_then_torch_rows"] = beats(res["read_medians"], res["then_torch_rows"], "Gbp_s")
    res["read_medians_beats_then_torch_ragged"] = beats(res["read_medians"], res["then_torch_ragged"], "Gbp_s")
    del counts, valid, small, keep
    b.close()
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "k": K, "quantile": "1/2",
       "note": "interleaved rounds after one warm-up pass; median with min .. max beside it; what binds the kernels: not measured; "
               "sub-wave grouping of the wave form (16 or 32 lanes per read): not built, not measured", "rows": {}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
for lg in args.log2:
    table = ctx.count_table(torch.randint(0, 1 << KEY_BITS, (1 << lg,), dtype=torch.int64, device="cuda", generator=gen), None, key_bits=KEY_BITS)
    for read_len in args.read_len:
        name = f"reads_{read_len}_table_2^{lg}"
        out["rows"][name] = bench(table, lg, read_len)
        print(json.dumps({name: out["rows"][name]}), flush=True)
        with open(args.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(out, f, indent=1)
            f.write("\n")
    table.close()
