#!/usr/bin/env python3
"""What BGZF written on the device costs and buys on ONE GPU (bl_bgzf_deflate, bl_text_write_bgzf).  Texts, made on the device:
  reads150_fastq   150-bp reads as 4-line FASTQ: names "@r<10 digits>", uniform random ACGT, qualities clip(normal(36, 4), 2, 40) + 33
  reads10k_fasta   10-kbp reads as FASTA wrapped at 60, generated names (Batch.format)
  gfa              the GFA text of a two-haplotype random genome with a SNP about every 1,000 bases (count_table -> unitigs(links) ->
                   format_gfa), 2^--gfa-log2 positions a haplotype (links_bench.py's genome_snp table, built through the Python interface)
--gbp bases for the first two.  Timed with the host clock around calls that end in a device synchronise; after one warm-up pass `rounds`
passes are taken with the variants INTERLEAVED; the median is reported with the spread (min .. max).  Variants:
  deflate           bl_bgzf_deflate into a buffer that exists: GB/s of TEXT, and the ratio
  write_null        bl_text_write to /dev/null            write_bgzf_null   bl_text_write_bgzf to /dev/null
  write_file        bl_text_write to a file in --dir      write_bgzf_file   bl_text_write_bgzf to a file in --dir
Once, not interleaved: zlib level 1 over 16 host threads on a sample of at most 256 MB in 65,280-byte blocks (the host alternative), and
the sizes zlib 1 and zlib 6 give on the same blocks of a 64 MB sample beside the device's on that sample.  The first members of the
device's output are inflated with zlib and compared with the text.  Clocks are not pinned.
    bgzf_bench.py [--out profiles/bgzf_bench.json] [--gbp 1.5] [--rounds 3] [--gfa-log2 25] [--dir DIR]"""
import argparse, ctypes as C, json, os, statistics, sys, tempfile, time, zlib
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import biolib_amd as B

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_bench.json"))
ap.add_argument("--gbp", type=float, default=1.5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--gfa-log2", type=int, default=25)
ap.add_argument("--dir", default=None)
args = ap.parse_args()
ctx = B.Context(0)
gen = torch.Generator(device="cuda").manual_seed(2026)
MEMBER = 65280
ACGT = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")


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


def stats(seconds, n_bytes):
    m = statistics.median(seconds)
    return {"ms_median": round(m * 1e3, 3), "ms_min": round(min(seconds) * 1e3, 3), "ms_max": round(max(seconds) * 1e3, 3), "text_GB_s": round(n_bytes / m / 1e9, 2)}


def fastq_text(n, L):
    width = 12 + 1 + L + 1 + 2 + L + 1
    rec = torch.empty((n, width), dtype=torch.uint8, device="cuda")
    rec[:, 0], rec[:, 1] = ord("@"), ord("r")
    num = torch.arange(n, dtype=torch.int64, device="cuda")
    for d in range(10):
        rec[:, 11 - d] = (48 + num % 10).to(torch.uint8)
        num = num // 10
    rec[:, 12] = 10
    step = max(1, (256 << 20) // width)
    for a in range(0, n, step):
        b = min(n, a + step)
        rec[a:b, 13:13 + L] = ACGT[torch.randint(0, 4, (b - a, L), device="cuda", generator=gen)]
        q = torch.empty((b - a, L), device="cuda").normal_(36, 4, generator=gen).round_().clamp_(2, 40) + 33
        rec[a:b, 16 + L:16 + 2 * L] = q.to(torch.uint8)
    rec[:, 13 + L], rec[:, 14 + L], rec[:, 15 + L], rec[:, 16 + 2 * L] = 10, ord("+"), 10, 10
    return rec.reshape(-1)


def gfa_text(lg):
    k, n = 31, 1 << lg
    a = torch.randint(0, 4, (n,), device="cuda", generator=gen)
    b = a.clone()
    at = torch.randint(0, n, (n // 1000,), device="cuda", generator=gen)
    b[at] = (b[at] + 1) % 4
    batch = ctx.from_tensor(ACGT[torch.cat([a, b])], read_len=n)
    scan = batch.kmers(k, canonical=True)
    keys = torch.from_numpy(np.ascontiguousarray(scan["values"][scan["valid"] != 0]).view(np.int64)).cuda()
    table = ctx.count_table(keys, key_bits=2 * k)
    u = table.unitigs(k, links=True)
    text = u.format_gfa().clone()
    table.close()
    batch.close()
    return text


def texts():
    yield "reads150_fastq", lambda: fastq_text(int(args.gbp * 1e9) // 150, 150)

    def fasta():
        L = 10_000
        n = int(args.gbp * 1e9) // L
        b = ctx.from_tensor(ACGT[torch.randint(0, 4, (n * L,), device="cuda", generator=gen)], read_len=L)
        t = b.format(fmt="fasta", prefix="r", line_width=60).clone()
        b.close()
        return t

    yield "reads10k_fasta", fasta
    yield "gfa", lambda: gfa_text(args.gfa_log2)


def zlib_blocks(sample, level):
    def one(i):
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        return len(z.compress(sample[i:i + MEMBER]) + z.flush()) + 26

    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        total = sum(pool.map(one, range(0, len(sample), MEMBER)))
    return total, time.perf_counter() - t0


out = {"rounds": args.rounds, "gbp": args.gbp, "gfa_log2": args.gfa_log2,
       "note": "interleaved rounds after one warm-up pass; median with min .. max; host clock around synchronous calls; clocks not pinned; GB/s are "
               "bytes of TEXT per second; zlib rows: 16 host threads, 65,280-byte blocks, 26 bytes of framing a member counted", "rows": {}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
tmp = tempfile.mkdtemp(prefix="bgzf_bench_", dir=args.dir)
lib, check = ctx._lib, B.capi.check

for name, make in texts():
    text = make()
    n = int(text.numel())
    bound = int(lib.bl_bgzf_bound(n, 0))
    dest = torch.empty(bound, dtype=torch.uint8, device="cuda")
    nb = C.c_uint64()
    plain, packed = os.path.join(tmp, name + ".txt").encode(), os.path.join(tmp, name + ".gz").encode()
    torch.cuda.synchronize()

    def deflate():
        check(lib.bl_bgzf_deflate(ctx._h, text.data_ptr(), n, 0, dest.data_ptr(), bound, C.byref(nb), None, None))

    variants = {"deflate": deflate,
                "write_null": lambda: check(lib.bl_text_write(ctx._h, text.data_ptr(), n, b"/dev/null", 0)),
                "write_bgzf_null": lambda: check(lib.bl_text_write_bgzf(ctx._h, text.data_ptr(), n, b"/dev/null", 0, 0)),
                "write_file": lambda: check(lib.bl_text_write(ctx._h, text.data_ptr(), n, plain, 0)),
                "write_bgzf_file": lambda: check(lib.bl_text_write_bgzf(ctx._h, text.data_ptr(), n, packed, 0, 0))}
    res = {v: stats(s, n) for v, s in interleaved(variants).items()}
    n_out = int(nb.value)
    res.update(text_bytes=n, bgzf_bytes=n_out, ratio=round(n_out / n, 4), file_bytes=os.path.getsize(packed))
    res["write_bgzf_over_write_null"] = round(res["write_bgzf_null"]["ms_median"] / res["write_null"]["ms_median"], 3)
    res["write_bgzf_over_write_file"] = round(res["write_bgzf_file"]["ms_median"] / res["write_file"]["ms_median"], 3)
    # the first members, judged by zlib
    head = dest[:min(n_out, 4 * (MEMBER + 31))].cpu().numpy().tobytes()
    at = done = 0
    while at + 18 <= len(head) and at + int.from_bytes(head[at + 16:at + 18], "little") + 1 <= len(head):
        size = int.from_bytes(head[at + 16:at + 18], "little") + 1
        part = zlib.decompress(head[at + 18:at + size - 8], -15)
        assert part == text[done:done + len(part)].cpu().numpy().tobytes(), "the device's member does not inflate to its text"
        at, done = at + size, done + len(part)
    assert done > 0
    # the host alternative, and the sizes on the same blocks
    sample = text[:min(n, 256 << 20) // MEMBER * MEMBER or n].cpu().numpy().tobytes()
    z1_bytes, z1_s = zlib_blocks(sample, 1)
    res["zlib1_16_threads"] = {"sample_bytes": len(sample), "s": round(z1_s, 3), "text_GB_s": round(len(sample) / z1_s / 1e9, 3), "ratio": round(z1_bytes / len(sample), 4)}
    small = sample[:min(len(sample), 64 << 20) // MEMBER * MEMBER or len(sample)]
    ours = int(ctx.bgzf_deflate(text[:len(small)], eof=False).numel())
    res["sizes_on_64MB"] = {"sample_bytes": len(small), "device": round(ours / len(small), 4), "zlib1": round(zlib_blocks(small, 1)[0] / len(small), 4),
                            "zlib6": round(zlib_blocks(small, 6)[0] / len(small), 4)}
    out["rows"][name] = res
    print(json.dumps({name: res}), flush=True)
    with open(args.out, "w") as f:  # after every row: a run cut short keeps what it measured
        json.dump(out, f, indent=1)
        f.write("\n")
    for p in (plain, packed):
        if os.path.exists(p):
            os.unlink(p)
    del text, dest, sample, small
    torch.cuda.empty_cache()
os.rmdir(tmp)
