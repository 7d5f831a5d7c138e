#!/usr/bin/env python3
"""Rates of the unitig links and the GFA text (bl_unitig_links, bl_unitigs_format_gfa) on ONE GPU.  Tables at k = 31 (one-word keys), all
counts 1, at 2^22 and 2^26 genome positions / keys:
  genome_snp  the canonical k-mers of a random sequence and of a second haplotype that differs in one base about every 1,000: many
              unitigs of about 1,000 bases, nearly every end of degree 2 (a bubble's fork or merge)
  random      a random set of canonical k-mers: every key an isolated unitig, two dead ends each, no record
Timed per table, each a synchronous call with the host clock around it:
  unitigs      bl_table_unitigs alone (batch, offsets, count sums, nodes): what has to run before the links
  links        bl_unitig_links, records and offsets written (capacity from the header's identity: no sizing call)
  gfa          bl_unitigs_format_gfa into a buffer sized by one earlier sizing call
  text_write   bl_text_write of that text to /dev/null
  torch_links  what a caller could write before: eight successor arrays made with torch (both sides of every key, four bases each), each
               canonicalised, torch.searchsorted on the sorted keys, gathers of the nodes, the `to` words formed, the records of end
               sides counted; checked equal to the library's record count
  python_gfa   (tables of at most --python-max-lines lines; ONE run, not a median) the per-line Python join the device writer replaces:
               download of bases, offsets, sums and links, then "\\t".join per line; checked equal to the device text byte for byte
After one warm-up pass over all variants, `rounds` passes are taken with the variants INTERLEAVED; the median is reported with the spread
(min .. max).  `links_beat_torch` compares whole spreads.  Clocks are not pinned; rocm-smi's current sclk is noted before and after where
the tool is there.  What binds the link kernel is not measured here (no counter run).  Writes one JSON file.
    links_bench.py [--out profiles/links_bench.json] [--log2 22 26] [--rounds 3] [--python-max-lines 6000000]"""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B
from biolib_amd.scan import Batch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "links_bench.json"))
ap.add_argument("--log2", type=int, nargs="*", default=[22, 26])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--python-max-lines", type=int, default=6000000)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(950)
M3, MF = 0x3333333333333333, 0x0F0F0F0F0F0F0F0F
K = 31
TOP = 1 << (2 * K)


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


def revcomp(x):
    return shr(~reverse_pairs(x), 64 - 2 * K)


def canonical(x):
    return torch.minimum(x, revcomp(x))  # (below 2^62: the signed order is the key order)


def kmers_of(bases, n):
    lo = torch.zeros(n, dtype=torch.int64, device="cuda")
    for j in range(K):
        lo |= bases[j:j + n] << (2 * (K - 1 - j))
    return lo


def genome_snp_keys(n):
    bases = torch.randint(0, 4, (n + K - 1,), dtype=torch.int64, device="cuda", generator=gen)
    other = bases.clone()
    at = torch.arange(500, n + K - 1, 1000, device="cuda")
    other[at] = (bases[at] + torch.randint(1, 4, (at.numel(),), dtype=torch.int64, device="cuda", generator=gen)) & 3
    return torch.cat([kmers_of(bases, n), kmers_of(other, n)])


def random_keys(n):
    return torch.randint(0, TOP, (n,), dtype=torch.int64, device="cuda", generator=gen)


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
    src = canonical((genome_snp_keys if kind == "genome_snp" else random_keys)(1 << lg))
    table = ctx.count_table(src, None, key_bits=2 * K)
    del src
    n, dev = table.n_distinct, ctx.torch_device
    keys = table.keys
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sums = torch.empty(n, dtype=torch.int64, device=dev)
    nodes = torch.empty((n, 2), dtype=torch.int32, device=dev)
    st, ls = B.capi.GraphStats(), B.capi.LinkStats()
    keep = {}

    def unitigs():
        if "batch" in keep:
            B.capi.check(ctx._lib.bl_batch_destroy(keep.pop("batch")))
        h, nu, nb = table.unitigs_raw(K, True, offsets, sums, nodes, st)
        keep.update(batch=h, nu=nu, nb=nb)

    unitigs()
    nu = keep["nu"]
    bound = int(st.n_arcs) - int(st.n_linked_sides) + 2 * int(st.n_cycles)
    link_offsets = torch.empty(2 * nu + 1, dtype=torch.int64, device=dev)
    d_links = torch.empty((max(bound, 1), 2), dtype=torch.int32, device=dev)

    def links():
        keep["n_links"] = table.unitig_links_raw(K, nodes, offsets, nu, 0, link_offsets, d_links, bound, ls)

    links()
    n_links = keep["n_links"]
    assert n_links == bound, "the header's identity"
    rule = B.capi.GfaRule()
    rule.k = K
    def gfa_call(out, capacity):
        nb = C.c_uint64()
        B.capi.check(ctx._lib.bl_unitigs_format_gfa(ctx._h, keep["batch"], C.c_void_p(offsets.data_ptr()), nu, C.c_void_p(sums.data_ptr()),
                                                    C.c_void_p(d_links.data_ptr()) if n_links else None, n_links, C.byref(rule),
                                                    C.c_void_p(out.data_ptr()) if out is not None else None, capacity, C.byref(nb)))
        return int(nb.value)

    n_bytes = gfa_call(None, 0)
    text = torch.empty(n_bytes, dtype=torch.uint8, device=dev)

    def text_write():
        B.capi.check(ctx._lib.bl_text_write(ctx._h, C.c_void_p(text.data_ptr()), n_bytes, b"/dev/null", 0))

    def torch_links():
        u, rf = nodes[:, 0].long(), nodes[:, 1].long()
        rank, flip = rf >> 1, rf & 1
        length = offsets[1:nu + 1] - offsets[:nu] - (K - 1)
        first, last = rank == 0, rank == length[u] - 1
        ends = {1: (last & (flip == 0)) | (first & (flip == 1)), 0: (last & (flip == 1)) | (first & (flip == 0))}  # side -> the side is an end
        rx = revcomp(keys)
        total = 0
        for side, z in ((1, keys), (0, rx)):
            for c in range(4):
                f = ((z << 2) | c) & (TOP - 1)
                y = canonical(f)
                pos = torch.searchsorted(keys, y).clamp(max=n - 1)
                found = (keys[pos] == y) & ends[side]
                to = (u[pos] << 1) | ((y != f).long() ^ flip[pos])
                keep["torch_to"] = torch.where(found, to, torch.full_like(to, -1))
                total += int(found.sum())
        keep["torch_n_links"] = total

    variants = {"unitigs": unitigs, "links": links, "gfa": lambda: gfa_call(text, n_bytes), "text_write": text_write, "torch_links": torch_links}
    before = clocks()
    times = interleaved(variants)
    assert keep["torch_n_links"] == n_links, "the torch composition and the library disagree on the number of records"
    res = {"keys": n, "k": K, "prefix_bits": table.prefix_bits, "unitigs": nu, "bases": keep["nb"], "links": n_links, "gfa_bytes": n_bytes,
           "link_stats": ls.as_dict(), "sclk_before": before, "sclk_after": clocks()}
    res["calls"] = {name: row(s) for name, s in times.items()}
    med = {name: statistics.median(s) for name, s in times.items()}
    res["links_Mends_s"] = round(2 * nu / med["links"] / 1e6, 1)
    res["gfa_GB_s"] = round(n_bytes / med["gfa"] / 1e9, 2)
    res["text_write_GB_s"] = round(n_bytes / med["text_write"] / 1e9, 2)
    res["links_over_torch"] = round(med["torch_links"] / med["links"], 2)
    res["links_beat_torch"] = bool(max(times["links"]) < min(times["torch_links"]))
    if 1 + nu + n_links <= args.python_max_lines:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = Batch(ctx, keep.pop("batch"))
        bases = batch.download().tobytes().decode("ascii")
        off, sm, lk = offsets[:nu + 1].cpu().tolist(), sums[:nu].cpu().tolist(), d_links[:n_links].cpu().tolist()
        lines = ["H\tVN:Z:1.0"]
        for i in range(nu):
            s = bases[off[i]:off[i + 1]]
            lines.append("\t".join(("S", str(i), s, "LN:i:%d" % len(s), "KC:i:%d" % sm[i])))
        for a, b in lk:
            lines.append("\t".join(("L", str(a >> 1), "+-"[a & 1], str(b >> 1), "+-"[b & 1], "%dM" % (K - 1))))
        joined = ("\n".join(lines) + "\n").encode("ascii")
        seconds = time.perf_counter() - t0
        assert joined == text.cpu().numpy().tobytes(), "the Python join and the device text differ"
        res["python_gfa_one_run_ms"] = round(seconds * 1e3, 1)
        res["gfa_over_python"] = round(seconds / med["gfa"], 1)
        batch.close()
    else:
        B.capi.check(ctx._lib.bl_batch_destroy(keep.pop("batch")))
    keep.clear()
    table.close()
    del keys, offsets, sums, nodes, link_offsets, d_links, text
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "tables": {},
       "note": "interleaved rounds after one warm-up pass; medians with min .. max; clocks not pinned; python_gfa is ONE run; what binds the link kernel: "
               "not measured (no counter run)"}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
for kind, lg in [(kind, lg) for lg in args.log2 for kind in ("genome_snp", "random")]:
    name = f"{kind}_k{K}_2^{lg}"
    out["tables"][name] = bench_table(kind, lg)
    print(json.dumps({name: out["tables"][name]}), flush=True)
    with open(args.out, "w") as f:  # after every table: a run cut short keeps what it measured
        json.dump(out, f, indent=1)
        f.write("\n")
