#!/usr/bin/env python3
"""Rates of the table graph (bl_table_adjacency, bl_table_unitigs) on ONE GPU.  Tables, all counts 1:
  genome   the canonical k-mers of a random sequence: a few very long unitigs (the doubling runs its full number of rounds)
  random   a random set of canonical k-mers: nearly every key isolated (every key is a start key: emission at its worst)
at 2^22 and 2^26 keys with k = 31 (one-word keys) and at 2^26 keys with k = 51 (two-word keys).  Timed per table:
  mask            bl_table_adjacency without links and statistics: the key check and the mask pass
  mask_link       ... with links: adds the link pass (link = mask_link - mask)
  labels          bl_table_unitigs without a batch and without count sums: adds labelling, placement and numbering
                  (labelling = labels - mask_link)
  unitigs         the whole call: adds emission, count sums and the batch (emission = unitigs - labels)
  torch_lookups   one-word tables only — what a caller could write before: eight neighbour-key arrays made with torch, each
                  canonicalised, eight CountTable.lookup calls, the bits packed into a byte; checked equal to the mask pass's bytes
The phases are differences of medians of calls that each contain the earlier phases; no kernel is timed alone.  Every call is
synchronous, so the host clock around it is the call time.  After one warm-up pass over all variants, `rounds` passes are taken with the
variants INTERLEAVED; the median is reported with the spread (min .. max).  `fused_beats_torch` compares whole spreads.  Clocks are not
pinned; rocm-smi's current sclk is noted before and after where the tool is there.  What binds labelling and emission is not measured
here (no counter run).  Writes one JSON file.
    graph_bench.py [--out profiles/graph_bench.json] [--log2 22 26] [--wide-log2 26] [--rounds 3]"""
import argparse, json, math, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_bench.json"))
ap.add_argument("--log2", type=int, nargs="*", default=[22, 26])
ap.add_argument("--wide-log2", type=int, nargs="*", default=[26])
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(950)
M3, MF = 0x3333333333333333, 0x0F0F0F0F0F0F0F0F


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout  # (a query, no setting)
        return [line.strip() for line in out.splitlines() if "sclk" in line][:1]
    except Exception:
        return []


def shr(x, s):
    """logical shift right of int64 words"""
    return (x >> s) & ((1 << (64 - s)) - 1) if s else x


def reverse_pairs(v):
    v = (shr(v, 2) & M3) | ((v & M3) << 2)
    v = (shr(v, 4) & MF) | ((v & MF) << 4)
    return v.contiguous().view(torch.uint8).reshape(-1, 8).flip(1).contiguous().view(torch.int64).reshape(v.shape)


def revcomp(lo, hi, k):
    """reverse complement in 2k bits of (lo, hi) int64 word tensors; hi None: one word (k <= 31)"""
    if hi is None:
        return shr(~reverse_pairs(lo), 64 - 2 * k), None
    top, bottom = ~reverse_pairs(lo), ~reverse_pairs(hi)
    sh = 128 - 2 * k
    assert 0 < sh < 64
    return shr(bottom, sh) | (top << (64 - sh)), shr(top, sh)


def canonical(lo, hi, k):
    rlo, rhi = revcomp(lo, hi, k)
    if hi is None:
        return torch.minimum(lo, rlo), None  # (below 2^62: the signed order is the key order)
    flip = 1 << 63
    smaller = (rhi < hi) | ((rhi == hi) & ((rlo ^ -flip) < (lo ^ -flip)))  # (hi below 2^62; lo unsigned through the sign flip)
    return torch.where(smaller, rlo, lo), torch.where(smaller, rhi, hi)


def genome_keys(n, k):
    """the k-mers of n + k - 1 random bases, first base in the most significant pair"""
    bases = torch.randint(0, 4, (n + k - 1,), dtype=torch.int64, device="cuda", generator=gen)
    lo = torch.zeros(n, dtype=torch.int64, device="cuda")
    hi = torch.zeros(n, dtype=torch.int64, device="cuda") if k > 32 else None
    for j in range(k):
        p = 2 * (k - 1 - j)
        if p >= 64:
            hi |= bases[j:j + n] << (p - 64)
        else:
            lo |= bases[j:j + n] << p
    return lo, hi


def random_keys(n, k):
    if k <= 31:
        return torch.randint(0, 1 << (2 * k), (n,), dtype=torch.int64, device="cuda", generator=gen), None
    lo = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda", generator=gen)
    return lo, torch.randint(0, 1 << (2 * k - 64), (n,), dtype=torch.int64, device="cuda", generator=gen)


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


def row(seconds, n):
    rates = sorted(n / s / 1e9 for s in seconds)
    return {"ms_median": round(statistics.median(seconds) * 1e3, 3), "ms_min": round(min(seconds) * 1e3, 3), "ms_max": round(max(seconds) * 1e3, 3),
            "Gkeys_s": round(statistics.median(rates), 4)}


def bench_table(kind, lg, k):
    n0 = 1 << lg
    lo, hi = (genome_keys if kind == "genome" else random_keys)(n0, k)
    lo, hi = canonical(lo, hi, k)
    src = lo if hi is None else torch.stack([lo, hi], dim=1).contiguous()
    del lo, hi
    table = ctx.count_table(src, None, key_bits=2 * k)
    del src
    n = table.n_distinct
    keys = table.keys
    dev = ctx.torch_device
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    links = torch.empty((n, 2), dtype=torch.int32, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sums = torch.empty(n, dtype=torch.int64, device=dev)
    nodes = torch.empty((n, 2), dtype=torch.int32, device=dev)
    st = B.capi.GraphStats()
    keep = {}

    def whole():
        h, nu, nb = table.unitigs_raw(k, True, offsets, sums, nodes, st)
        keep["unitigs"] = (nu, nb)
        B.capi.check(ctx._lib.bl_batch_destroy(h))

    variants = {"mask": lambda: table.adjacency_raw(k, mask), "mask_link": lambda: table.adjacency_raw(k, mask, links),
                "labels": lambda: table.unitigs_raw(k, False, offsets, None, nodes), "unitigs": whole}
    if table.key_words == 1:
        top = 1 << (2 * k)

        def torch_lookups():
            out = torch.zeros(n, dtype=torch.uint8, device=dev)
            for c in range(4):
                for bit, f in ((c, ((keys << 2) | c) & (top - 1)), (4 + c, (keys >> 2) | (c << (2 * k - 2)))):
                    y, _ = canonical(f, None, k)
                    out |= (table.lookup(y) != 0).to(torch.uint8) << bit
            keep["torch_mask"] = out
        variants["torch_lookups"] = torch_lookups
    before = clocks()
    times = interleaved(variants)
    res = {"keys": n, "k": k, "key_words": table.key_words, "prefix_bits": table.prefix_bits, "sclk_before": before, "sclk_after": clocks()}
    res["calls"] = {name: row(s, n) for name, s in times.items()}
    med = {name: statistics.median(s) for name, s in times.items()}
    res["phases_ms_by_difference"] = {"check_and_mask": round(med["mask"] * 1e3, 3), "link": round((med["mask_link"] - med["mask"]) * 1e3, 3),
                                      "labelling": round((med["labels"] - med["mask_link"]) * 1e3, 3), "emission": round((med["unitigs"] - med["labels"]) * 1e3, 3)}
    table.unitigs_raw(k, False, None, None, None, st)
    res["stats"] = st.as_dict()
    longest = max(res["stats"]["longest_unitig"], 1)
    res["labelling_rounds_from_longest"] = max(longest - 1, 1).bit_length() + 1  # (a table with cycles labels twice: n_cycles is in stats)
    res["unitigs"], res["bases"] = keep["unitigs"]
    if "torch_lookups" in variants:
        assert torch.equal(keep["torch_mask"], mask), "the eight lookups and the mask pass disagree"
        res["fused_over_torch"] = round(med["torch_lookups"] / med["mask"], 2)
        res["fused_beats_torch"] = bool(max(times["mask"]) < min(times["torch_lookups"]))
    keep.clear()
    table.close()
    del mask, links, offsets, sums, nodes, keys
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "tables": {},
       "note": "interleaved rounds after one warm-up pass; medians with min .. max; phases are differences of medians of nested calls; clocks not pinned; "
               "what binds labelling and emission: not measured (no counter run); labelling_rounds_from_longest is computed from the longest unitig, not read from the device"}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
plan = [(kind, lg, 31) for lg in args.log2 for kind in ("genome", "random")] + [(kind, lg, 51) for lg in args.wide_log2 for kind in ("genome", "random")]
for kind, lg, k in plan:
    name = f"{kind}_k{k}_2^{lg}"
    out["tables"][name] = bench_table(kind, lg, k)
    print(json.dumps({name: out["tables"][name]}), flush=True)
    with open(args.out, "w") as f:  # after every table: a run cut short keeps what it measured
        json.dump(out, f, indent=1)
        f.write("\n")
