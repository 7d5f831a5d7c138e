#!/usr/bin/env python3
"""Rates of the reads' steps through the compacted graph (bl_scan_read_steps, bl_link_support, bl_steps_format_gaf) on ONE GPU.  The graph
is links_bench.py's genome_snp table at k = 31 (a random sequence of 2^26 positions and a second haplotype that differs in one base about
every 1,000: about 69 M keys).  Reads are drawn from both haplotypes and both strands: --gbp (1.5) Gbp as 150-bp reads and as 10-kbp reads,
error-free and with 1 % substitutions.  Timed per workload, each a synchronous call with the host clock around it:
  read_steps    (a) bl_scan_read_steps, the records stored (capacity from one earlier sizing call)
  kmer_counts   (b) bl_scan_kmer_counts on the same batch and table, counts only: the lookup pass no mapper avoids, the yardstick
  torch_steps   (c) the torch composition the call replaces, in chunks of whole reads: kmers128 twice (canonical and forward: the strand),
                torch.searchsorted on CountTable.keys, the node gather, offsets, diff and nonzero
  link_support  (d) bl_link_support on the records
  gaf           (e) bl_steps_format_gaf into a buffer sized by one earlier sizing call
  text_write    bl_text_write of that text to /dev/null
The records of (a) must equal those of (c) field by field before anything is timed.  After one warm-up pass over all variants, `rounds`
passes are taken with the variants INTERLEAVED; the median is reported with the spread (min .. max).  Clocks are not pinned.  The node pass
of (a) is timed by the event pair the call records around it under bl_ctx_kernel_timing, in `rounds` more calls; the step passes are the
call's median minus that.  What binds the node pass is not measured (no counter run).  Writes one JSON file.
    steps_bench.py [--out profiles/steps_bench.json] [--log2 26] [--gbp 1.5] [--rounds 3]"""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import biolib_amd as B

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steps_bench.json"))
ap.add_argument("--log2", type=int, default=26)
ap.add_argument("--gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(950)
M3, MF = 0x3333333333333333, 0x0F0F0F0F0F0F0F0F
K = 31
CHUNK = 1 << 27  # positions of a chunk of the torch composition (whole reads)


def shr(x, s):
    return (x >> s) & ((1 << (64 - s)) - 1) if s else x


def reverse_pairs(v):
    v = (shr(v, 2) & M3) | ((v & M3) << 2)
    v = (shr(v, 4) & MF) | ((v & MF) << 4)
    return v.contiguous().view(torch.uint8).reshape(-1, 8).flip(1).contiguous().view(torch.int64).reshape(v.shape)


def canonical(x):
    return torch.minimum(x, shr(~reverse_pairs(x), 64 - 2 * K))  # (below 2^62: the signed order is the key order)


def kmers_of(bases, n):
    lo = torch.zeros(n, dtype=torch.int64, device="cuda")
    for j in range(K):
        lo |= bases[j:j + n] << (2 * (K - 1 - j))
    return lo


def genome(n):
    """two haplotypes as 2-bit codes (uint8), and their canonical k-mers"""
    bases = torch.randint(0, 4, (n + K - 1,), dtype=torch.int64, device="cuda", generator=gen)
    other = bases.clone()
    at = torch.arange(500, n + K - 1, 1000, device="cuda")
    other[at] = (bases[at] + torch.randint(1, 4, (at.numel(),), dtype=torch.int64, device="cuda", generator=gen)) & 3
    keys = canonical(torch.cat([kmers_of(bases, n), kmers_of(other, n)]))
    return torch.stack([bases.to(torch.uint8), other.to(torch.uint8)]), keys


def make_reads(haps, read_len, n_reads, rate):
    """n_reads * read_len ASCII bases: a random haplotype, place and strand per read, substitutions at `rate`"""
    glen = haps.shape[1]
    out = torch.empty(n_reads * read_len, dtype=torch.uint8, device="cuda")
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    per = max(1, (1 << 26) // read_len)
    j = torch.arange(read_len, device="cuda")
    for r0 in range(0, n_reads, per):
        m = min(per, n_reads - r0)
        start = torch.randint(0, glen - read_len + 1, (m, 1), device="cuda", generator=gen)
        hap = torch.randint(0, 2, (m, 1), device="cuda", generator=gen)
        rev = torch.randint(0, 2, (m, 1), device="cuda", generator=gen).bool()
        idx = torch.where(rev, start + (read_len - 1) - j, start + j) + hap * glen
        codes = haps.reshape(-1)[idx]
        codes = torch.where(rev, 3 - codes, codes)
        if rate:
            err = torch.rand((m, read_len), device="cuda", generator=gen) < rate
            codes = torch.where(err, (codes + torch.randint(1, 4, (m, read_len), dtype=torch.uint8, device="cuda", generator=gen)) & 3, codes)
        out[r0 * read_len:(r0 + m) * read_len] = letters[codes.long()].reshape(-1)
    return out


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


def torch_steps(batch, table_keys, nodes, lengths, read_len, n_bases):
    """the composition: the records' six fields as int64 tensors, in chunks of whole reads"""
    n_keys = table_keys.numel()
    parts = []
    step = max(1, CHUNK // read_len) * read_len
    vc = torch.empty((min(step, n_bases), 2), dtype=torch.int64, device="cuda")
    vf = torch.empty_like(vc)
    ok = torch.empty(min(step, n_bases), dtype=torch.uint8, device="cuda")
    for b in range(0, n_bases, step):
        n = min(step, n_bases - b)
        batch.kmers128_raw(K, 0, B.FLAG_CANONICAL | B.FLAG_SYNC, b, n, vc, None, ok)
        batch.kmers128_raw(K, 0, B.FLAG_SYNC, b, n, vf, None, None)
        c, f = vc[:n, 0], vf[:n, 0]
        slot = torch.searchsorted(table_keys, c).clamp(max=n_keys - 1)
        found = (table_keys[slot] == c) & (ok[:n] != 0)
        nd = nodes[slot]
        u, rf = nd[:, 0].long(), nd[:, 1].long()
        o = (c != f).long() ^ (rf & 1)
        off = torch.where(o == 1, lengths[u] - 1 - (rf >> 1), rf >> 1)
        word = torch.where(found, (((u << 1) | o) << 32) | off, torch.full_like(off, -1))
        pos = torch.arange(b, b + n, device="cuda")
        cont = torch.zeros(n, dtype=torch.bool, device="cuda")
        cont[1:] = found[1:] & found[:-1] & ((word[1:] - word[:-1]) == 1) & ((pos[1:] % read_len) != 0)
        head = found & ~cont
        tail = found.clone()
        tail[:-1] &= ~cont[1:]
        hp, tp = torch.nonzero(head).reshape(-1), torch.nonzero(tail).reshape(-1)
        linked = torch.zeros(n, dtype=torch.bool, device="cuda")
        linked[1:] = found[:-1] & ((pos[1:] % read_len) != 0)
        parts.append(torch.stack([hp + b, (hp + b) // read_len, word[hp] >> 32, word[hp] & 0xFFFFFFFF, tp - hp + 1, (linked[hp] & head[hp]).long()], 1))
    return torch.cat(parts)


def bench(name, haps, table, u, read_len, rate):
    n_reads = int(args.gbp * 1e9) // read_len
    n_bases = n_reads * read_len
    bases = make_reads(haps, read_len, n_reads, rate)
    batch = ctx.from_tensor(bases, read_len=read_len)
    nodes, lengths = u._nodes, u.offsets[1:] - u.offsets[:-1] - (K - 1)
    call = (table, K, 0, nodes, u.offsets, u.n_unitigs)
    _, st = batch.read_steps_raw(*call, None, 0)
    n_steps = int(st.n_steps)
    steps = torch.empty((max(n_steps, 1), 4), dtype=torch.int64, device="cuda")
    batch.read_steps_raw(*call, steps, n_steps)
    want = torch_steps(batch, table.keys, nodes, lengths, read_len, n_bases)
    w32 = steps[:n_steps].view(torch.int32).long() & 0xFFFFFFFF
    got = torch.stack([steps[:n_steps, 0], steps[:n_steps, 1], w32[:, 4], w32[:, 5], w32[:, 6], w32[:, 7]], 1)
    assert got.shape == want.shape and bool((got == want).all()), "the library's records and the torch composition's differ"
    del want, got, w32
    counts = torch.empty(n_bases, dtype=torch.int32, device="cuda")
    rs = B.ReadSteps(batch, u, steps[:n_steps], st.as_dict(), None)
    n_links = int(u.links.shape[0])
    support = torch.empty(max(n_links, 1), dtype=torch.int32, device="cuda")
    sst = B.capi.SupportStats()
    rule = B.capi.GafRule()
    rule.k, rule.read_prefix = K, b"read"
    n_bytes = rs.format_gaf_raw(rule)
    text = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device="cuda")
    variants = {
        "read_steps": lambda: batch.read_steps_raw(*call, steps, n_steps),
        "kmer_counts": lambda: batch.kmer_counts_raw(table, K, B.FLAG_CANONICAL | B.FLAG_SYNC, 0, 0, counts, None),
        "torch_steps": lambda: torch_steps(batch, table.keys, nodes, lengths, read_len, n_bases),
        "link_support": lambda: rs.link_support_raw(u.link_offsets, u.links, n_links, u.n_unitigs, support, sst),
        "gaf": lambda: rs.format_gaf_raw(rule, text, n_bytes),
        "text_write": lambda: B.capi.check(ctx._lib.bl_text_write(ctx._h, C.c_void_p(text.data_ptr()), n_bytes, b"/dev/null", 0)),
    }
    times = interleaved(variants)
    med = {v: statistics.median(s) for v, s in times.items()}
    ctx.kernel_timing(True)  # the node pass alone, by the event pair the call records around it
    for _ in range(args.rounds):
        variants["read_steps"]()
    node_ms, launches = ctx.kernel_time()
    ctx.kernel_timing(False)
    res = {"read_len": read_len, "substitution_rate": rate, "bases": n_bases, "reads": n_reads, "step_stats": st.as_dict(), "support_stats": sst.as_dict(),
           "gaf_bytes": n_bytes, "calls": {v: row(s) for v, s in times.items()}}
    res["read_steps_passes"] = {"node_pass_ms": round(node_ms / max(launches, 1), 3), "launches": launches,
                                "step_passes_ms": round(med["read_steps"] * 1e3 - node_ms / max(launches, 1), 3),
                                "note": "node pass: device events (bl_ctx_kernel_timing), the mean of `launches` calls after the timed rounds; step passes: the "
                                        "call's median minus that, so the two exclusive sums' host syncs and the statistics' download are in it"}
    res["read_steps_Gbase_s"] = round(n_bases / med["read_steps"] / 1e9, 3)
    res["kmer_counts_Gbase_s"] = round(n_bases / med["kmer_counts"] / 1e9, 3)
    res["read_steps_over_kmer_counts"] = round(med["read_steps"] / med["kmer_counts"], 3)
    res["torch_over_read_steps"] = round(med["torch_steps"] / med["read_steps"], 2)
    res["gaf_over_text_write"] = round(med["gaf"] / med["text_write"], 3)
    # what each pass moves per base beside the searches' key loads: the packed codes are read by both scans
    res["bytes_per_base"] = {"kmer_counts": "4 written (the count)", "read_steps": "node pass: 8 gathered (the node) where the key is found, 8 written (the word); "
                             "step passes: 2 x 8 read (the words, counted and emitted), 1/8 read twice (the start bits); per step 8 + 32 written"}
    batch.close()
    del bases, steps, counts, text, support
    torch.cuda.empty_cache()
    return res


out = {"rounds": args.rounds, "k": K, "workloads": {},
       "note": "interleaved rounds after one warm-up pass; medians with min .. max; clocks not pinned; what binds the node pass: not measured "
               "(no counter run)"}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
haps, keys = genome(1 << args.log2)
table = ctx.count_table(keys, None, key_bits=2 * K)
del keys
u = table.unitigs(K, batch=False, links=True)
out["graph"] = {"keys": table.n_distinct, "prefix_bits": table.prefix_bits, "unitigs": u.n_unitigs, "links": int(u.links.shape[0])}
print(json.dumps(out["graph"]), flush=True)
for read_len in (150, 10000):
    for rate in (0.0, 0.01):
        name = "reads_%d_sub_%g" % (read_len, rate)
        out["workloads"][name] = bench(name, haps, table, u, read_len, rate)
        print(json.dumps({name: out["workloads"][name]}), flush=True)
        with open(args.out, "w") as f:  # after every workload: a run cut short keeps what it measured
            json.dump(out, f, indent=1)
            f.write("\n")
