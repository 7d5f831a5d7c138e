#!/usr/bin/env python3
"""Rates of graph cleaning (bl_unitigs_mark, bl_table_remove_unitigs) on ONE GPU.  Tables at k = 31 (one-word keys), all counts 1:
  genome_snp_spurs  links_bench.py's "genome + SNPs" table (a random sequence and a second haplotype that differs in one base about every
                    1,000) at 2^22 and 2^26 positions, with a spur of 5 keys planted about every 4,000 positions: most unitigs are about
                    1,000 bases long and leave the mark kernel after their own six words; the bubbles' branches (31 keys) and the spurs
                    go on to the second level
  random            a random set of 2^26 canonical k-mers: every key an isolated unitig, every one marked, the result the empty table
Timed per table, each a synchronous call with the host clock around it:
  unitigs       bl_table_unitigs (labels only: offsets, count sums, nodes)          } what has to run before, for proportion
  links         bl_unitig_links, records and offsets written                        }
  mark          bl_unitigs_mark with CountTable.clean's default rule (every limit 2 k)
  remove        bl_table_remove_unitigs: count, exclusive sum, write, and the result's prefix index (bllk::finish_table)
  torch_remove  what a caller could write before: marks[nodes[:, 0]], boolean selection of keys and counts, Context.count_table; checked
                to give the same table, keys and counts
After one warm-up pass over all variants, `rounds` passes are taken with the variants INTERLEAVED; the median is reported with the spread
(min .. max).  `remove_beats_torch` compares whole spreads.  Clocks are not pinned; rocm-smi's current sclk is noted before and after where
the tool is there.  What binds the mark kernel is not measured here (no counter run).  Writes one JSON file.
    clean_bench.py [--out profiles/clean_bench.json] [--log2 22 26] [--random-log2 26] [--rounds 3]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B
from biolib_amd.scan import CountTable

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clean_bench.json"))
ap.add_argument("--log2", type=int, nargs="*", default=[22, 26])
ap.add_argument("--random-log2", type=int, nargs="*", default=[26])
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(950)
M3, MF = 0x3333333333333333, 0x0F0F0F0F0F0F0F0F
K = 31
TOP = 1 << (2 * K)
SPUR_KEYS, SPUR_EVERY = 5, 4000


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


def canonical(x):
    return torch.minimum(x, shr(~reverse_pairs(x), 64 - 2 * K))  # (below 2^62: the signed order is the key order)


def kmers_of(bases, n):
    """the n k-mers of every row of `bases` ([rows, n + K - 1], or one sequence)"""
    lo = torch.zeros(bases.shape[:-1] + (n,), dtype=torch.int64, device="cuda")
    for j in range(K):
        lo |= bases[..., j:j + n] << (2 * (K - 1 - j))
    return lo.reshape(-1)


def genome_snp_spur_keys(n):
    bases = torch.randint(0, 4, (n + K - 1,), dtype=torch.int64, device="cuda", generator=gen)
    other = bases.clone()
    at = torch.arange(500, n + K - 1, 1000, device="cuda")
    other[at] = (bases[at] + torch.randint(1, 4, (at.numel(),), dtype=torch.int64, device="cuda", generator=gen)) & 3
    start = torch.arange(250, n - 2 * K, SPUR_EVERY, device="cuda")  # (between two SNPs: both haplotypes agree there)
    spurs = bases[start[:, None] + torch.arange(K - 1 + SPUR_KEYS, device="cuda")[None, :]]
    spurs[:, K - 1] = (spurs[:, K - 1] + torch.randint(1, 4, (start.numel(),), dtype=torch.int64, device="cuda", generator=gen)) & 3
    spurs[:, K:] = torch.randint(0, 4, (start.numel(), SPUR_KEYS - 1), dtype=torch.int64, device="cuda", generator=gen)
    return torch.cat([kmers_of(bases, n), kmers_of(other, n), kmers_of(spurs, SPUR_KEYS)]), int(start.numel())


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


def row(seconds):
    return {"ms_median": round(statistics.median(seconds) * 1e3, 3), "ms_min": round(min(seconds) * 1e3, 3), "ms_max": round(max(seconds) * 1e3, 3)}


def bench_table(kind, lg):
    n_spurs = 0
    if kind == "random":
        src = torch.randint(0, TOP, (1 << lg,), dtype=torch.int64, device="cuda", generator=gen)
    else:
        src, n_spurs = genome_snp_spur_keys(1 << lg)
    table = ctx.count_table(canonical(src), None, key_bits=2 * K)
    del src
    n, dev = table.n_distinct, ctx.torch_device
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sums = torch.empty(n, dtype=torch.int64, device=dev)
    nodes = torch.empty((n, 2), dtype=torch.int32, device=dev)
    st, ls, cs = B.capi.GraphStats(), B.capi.LinkStats(), B.capi.CleanStats()
    keep = {}

    def unitigs():
        _, nu, _ = table.unitigs_raw(K, False, offsets, sums, nodes, st)
        keep.update(nu=nu)

    unitigs()
    nu = keep["nu"]
    bound = int(st.n_arcs) - int(st.n_linked_sides) + 2 * int(st.n_cycles)
    link_offsets = torch.empty(2 * nu + 1, dtype=torch.int64, device=dev)
    d_links = torch.empty((max(bound, 1), 2), dtype=torch.int32, device=dev)

    def links():
        keep["n_links"] = table.unitig_links_raw(K, nodes, offsets, nu, 0, link_offsets, d_links, bound, ls)

    links()
    n_links = keep["n_links"]
    u = B.scan.Unitigs(None, offsets[:nu + 1], sums[:nu], None, None, nu, 0)
    u.k, u._ctx, u._lib, u.link_offsets, u.links = K, ctx, ctx._lib, link_offsets, d_links[:n_links]
    rule = B.capi.CleanRule()
    rule.flags, rule.k = 7, K
    rule.max_tip_keys = rule.max_isolated_keys = rule.max_bubble_keys = 2 * K
    rule.max_isolated_mean, rule.max_bubble_diff = 2**32 - 1, 0
    marks = torch.empty(nu, dtype=torch.uint8, device=dev)

    def mark():
        u.mark_raw(rule, marks, cs)

    def close(name):
        if name in keep:
            keep.pop(name).close()

    def remove():
        close("out")
        keep["out"] = CountTable(ctx, table.remove_unitigs_raw(nodes, marks, nu)[0])

    def torch_remove():
        close("torch_out")
        stay = marks[nodes[:, 0].long()] == 0
        keep["torch_out"] = ctx.count_table(table.keys[stay], table.counts[stay], key_bits=2 * K)

    variants = {"unitigs": unitigs, "links": links, "mark": mark, "remove": remove, "torch_remove": torch_remove}
    before = clocks()
    times = interleaved(variants)
    a, b = keep["out"], keep["torch_out"]
    assert a.n_distinct == b.n_distinct == n - int(cs.n_keys_marked), "the library, the torch composition and the stats disagree on the number of keys"
    assert torch.equal(a.keys, b.keys) and torch.equal(a.counts, b.counts), "the torch composition gives another table"
    n_out = a.n_distinct
    res = {"keys": n, "k": K, "unitigs": nu, "links": n_links, "spurs_planted": n_spurs, "clean_stats": cs.as_dict(), "keys_kept": n_out,
           "sclk_before": before, "sclk_after": clocks()}
    res["calls"] = {name: row(s) for name, s in times.items()}
    med = {name: statistics.median(s) for name, s in times.items()}
    res["mark_Munitigs_s"] = round(nu / med["mark"] / 1e6, 1)
    useful = n * 8 + n_out * 2 * (8 + 4)  # every node read once, the kept keys and counts read and written (mark bytes, the second read of the nodes and the index apart)
    res["remove_useful_bytes"] = useful
    res["remove_useful_GB_s"] = round(useful / med["remove"] / 1e9, 1)
    res["remove_over_torch"] = round(med["torch_remove"] / med["remove"], 2)
    res["remove_beats_torch"] = bool(max(times["remove"]) < min(times["torch_remove"]))
    res["mark_share_of_round"] = round(med["mark"] / (med["unitigs"] + med["links"] + med["mark"] + med["remove"]), 4)
    res["remove_share_of_round"] = round(med["remove"] / (med["unitigs"] + med["links"] + med["mark"] + med["remove"]), 4)
    close("out")
    close("torch_out")
    table.close()
    del offsets, sums, nodes, link_offsets, d_links, marks
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "tables": {},
       "note": "interleaved rounds after one warm-up pass; medians with min .. max; clocks not pinned; all counts 1, so ties in the keep order fall to "
               "the unitig number; what binds the mark kernel: not measured (no counter run)"}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
for kind, lg in [("genome_snp_spurs", lg) for lg in args.log2] + [("random", lg) for lg in args.random_log2]:
    name = f"{kind}_k{K}_2^{lg}"
    out["tables"][name] = bench_table(kind, lg)
    print(json.dumps({name: out["tables"][name]}), flush=True)
    with open(args.out, "w") as f:  # after every table: a run cut short keeps what it measured
        json.dump(out, f, indent=1)
        f.write("\n")
