"""CPU-only: the range sweep of tests/range_cases.py through the CPU emulation of the kernels.  Every scan entry point, cut at every kind of
place (every residue of `first` mod 16, every position around a tile and a wave border, sequence starts, N's, the repeat island, planted tie
windows, the batch's end; two- and three-way), every range element for element against the rule of range_cases.py, and the concatenation
over every cut set against the whole scan.  64-bit entries through libbl_emu.so (the planner and the phase code of the kernels); 128-bit
entries through the stand-alone emulators (tests/emu/emu_*128.cpp, built with the sanitizers), which take a list of ranges in one run.
What the emulation does not share with the device — bl_capi.hip's planning calls, the tile prefix scan, capacity handling, lazy start bits,
the choice of layout, the lanes — is test_gpu_range_seams.py's.

Breaks tried, one at a time, on a scratch copy of the tree (emulation rebuilt, this module run on the CPU; none committed), and the items that
failed; without a break all 35 pass.
  plan_scan takes align_down16(first) for the minimizer modes       all 9 minimizer / hash-sample / super-k-mer items of test_position_tiled_ranges
                                                                    and all 4 of test_read_tiled_ranges (their unaligned halves); the syncmer items pass
  kmer_thread: range_mask(first - j0, end + 1 - j0)                 all 6 test_dense_kmer_ranges items
  the seam rule ignores window first - 1 (both window forms)        the 5 minimizer items of test_position_tiled_ranges with w > 1 and the 3 minimizer
                                                                    items of test_read_tiled_ranges
  a group that opens a range behind the batch's start reports       the 2 super-k-mer items of test_position_tiled_ranges and the super-k-mer item of
  mm_pos + 1 (a stand-in for an mm_pos that is not re-based)        test_read_tiled_ranges
  plan_kmers128 rounds the origin up                                all 9 test_ranges_128 items (the record items plan with plan_scan and pass)"""
import concurrent.futures
import ctypes as C
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import kernel_cases as K
import oracle_lib as O
import range_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
TALLY = dict(cut_sets=0, ranges=0, seconds=0.0, cut_sets128=0, ranges128=0, seconds128=0.0)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    L = C.CDLL(os.path.join(EMU_DIR, "_build", "libbl_emu.so"))
    vp, u64, u = C.c_void_p, C.c_uint64, C.c_uint
    L.emu_batch.restype = vp
    L.emu_batch.argtypes = [vp, u64, vp, u64, u64]
    L.emu_batch_free.argtypes = [vp]
    L.emu_minimizers.argtypes = [vp, u64, u64, u, u, u64, u, vp, vp, vp, u64, vp]
    L.emu_hash_sample.argtypes = [vp, u64, u64, u, u64, u64, u, vp, vp, vp, u64, vp]
    L.emu_super_kmers.argtypes = [vp, u64, u64, u, u, u64, u, vp, vp, vp, vp, vp, u64, vp]
    L.emu_syncmers.argtypes = [vp, u64, u64, u, u, u, u, u64, u, vp, u64, vp]
    L.emu_kmers.argtypes = [vp, u64, u64, u, u64, u, vp, vp, vp, vp]
    return L


class Scanner:
    """one emulated batch and its output arrays, reused over the ranges of an input"""

    def __init__(self, emu, inp):
        self.emu, self.inp = emu, inp
        seq = inp.seq
        self.b = emu.emu_batch(O._ptr(seq), len(seq), None if inp.read_len else O._ptr(inp.offs), 0 if inp.read_len else len(inp.offs) - 1, inp.read_len)
        self.cap = len(seq) + 1
        self.a = [np.zeros(self.cap, np.uint64) for _ in range(3)]
        self.mp, self.sz = np.zeros(self.cap, np.uint8), np.zeros(self.cap, np.uint8)
        self.res = np.zeros(8, np.uint64)

    def close(self):
        self.emu.emu_batch_free(self.b)

    def scan(self, r, first, n):
        """the row's scan of [first, first + n): (what kernel_cases.assert_same compares, read-tiled scans taken)"""
        emu, a, res, cap, seed = self.emu, self.a, self.res, self.cap, self.inp.seed
        flags = 1 if r.canonical else 0
        frl = emu.emu_frl_scans()
        if r.entry == "minimizers":
            emu.emu_minimizers(self.b, first, n, r.unit, r.w, seed, flags, O._ptr(a[0]), O._ptr(a[1]), O._ptr(a[2]), cap, O._ptr(res))
        elif r.entry == "hash_sample":
            emu.emu_hash_sample(self.b, first, n, r.unit, seed, K.THRESHOLD, flags, O._ptr(a[0]), O._ptr(a[1]), O._ptr(a[2]), cap, O._ptr(res))
        elif r.entry == "super_kmers":
            emu.emu_super_kmers(self.b, first, n, r.unit + r.w - 1, r.unit, seed, flags, O._ptr(a[0]), O._ptr(a[1]), O._ptr(self.mp), O._ptr(self.sz), O._ptr(a[2]), cap, O._ptr(res))
        else:
            emu.emu_syncmers(self.b, first, n, r.unit + r.w - 1, r.unit, r.offsets[0], r.offsets[1], seed, flags, O._ptr(a[0]), cap, O._ptr(res))
        c = int(res[0])
        got = dict(count=c, xor_value=int(res[1]), xor_hash=int(res[2]), xor_pos=int(res[3]), aux=int(res[4]))
        if r.entry in ("minimizers", "hash_sample"):
            got.update(values=a[0][:c].copy(), positions=a[1][:c].copy(), hashes=a[2][:c].copy())
        elif r.entry == "super_kmers":
            got.update(minimizers=a[0][:c].copy(), first_pos=a[1][:c].copy(), mm_pos=self.mp[:c].copy(), sizes=self.sz[:c].copy(), hashes=a[2][:c].copy())
        else:
            got.update(positions=a[0][:c].copy())
        return got, emu.emu_frl_scans() - frl


def merged_groups(parts):
    """super-k-mer pieces of consecutive ranges put together again: a piece that opens a range continues the piece that closed the range
    before iff it starts at the next k-mer and has the same minimizer occurrence"""
    cat = {f: np.concatenate([p[f] for p in parts]).astype(np.int64 if f in ("mm_pos", "sizes", "first_pos") else np.uint64) for f in K.SK_FIELDS}
    keep = np.ones(len(cat["sizes"]), bool)
    at = 0
    for p in parts[:-1]:
        at += int(p["count"])
        if 0 < at < len(keep) and keep[at]:
            j = at - 1
            while not keep[j]:
                j -= 1
            if (cat["first_pos"][at] == cat["first_pos"][j] + cat["sizes"][j] and cat["first_pos"][at] + cat["mm_pos"][at] == cat["first_pos"][j] + cat["mm_pos"][j]
                    and cat["hashes"][at] == cat["hashes"][j]):
                cat["sizes"][j] += cat["sizes"][at]
                keep[at] = False
    return {f: cat[f][keep] for f in K.SK_FIELDS}


def check_cut_set(sc, r, W, whole, cuts, frl_expected=None):
    """every range against its rule; the concatenation against the whole scan"""
    n, parts = W.n, []
    for first, end in RC.ranges_of(cuts, n):
        got, frl = sc.scan(r, *RC.call_args(first, end, n))
        K.assert_same(r.entry, got, W.of_range(first, end), (K.row_id(r), sc.inp.label, cuts, first, end))
        if frl_expected is not None:
            assert frl == int(frl_expected(first, end)), (K.row_id(r), cuts, first, end, "read-tiled" if frl else "position-tiled")
        parts.append(got)
    what = (K.row_id(r), sc.inp.label, cuts, "concatenation")
    if r.entry == "super_kmers":
        assert sum(int(p["sizes"].astype(np.int64).sum()) for p in parts) == W.kmers, what
        m = merged_groups(parts)
        for f in K.SK_FIELDS:
            assert np.array_equal(m[f].astype(whole[f].dtype), whole[f]), (what, f)
    else:
        K.assert_same(r.entry, RC.concat(parts, r.entry), whole, what)
    TALLY["cut_sets"] += 1
    TALLY["ranges"] += len(parts)


def run_row(emu, r, inputs, cut_sets_of, frl=False):
    t0 = time.time()
    for inp in inputs:
        W = RC.Whole(r, inp)
        whole = W.whole()
        sc = Scanner(emu, inp)
        try:
            got, took = sc.scan(r, 0, 0)
            K.assert_same(r.entry, got, whole, (K.row_id(r), inp.label, "whole"))
            assert took == int(frl) and whole["count"] > (20 if r.entry != "hash_sample" else 5)
            sets = cut_sets_of(inp)
            assert len(sets) > 10
            for cuts in sets:
                check_cut_set(sc, r, W, whole, cuts, (lambda a, b: RC.read_tiled(a, b, inp.read_len)) if frl else None)
        finally:
            sc.close()
    TALLY["seconds"] += time.time() - t0


# ----------------------------------------------------------------------------- the rules themselves

def test_the_rules_agree_with_kernel_cases_and_the_oracle():
    """range_cases.Whole derives a range from ONE oracle run; kernel_cases.expected runs the oracle's rule per range: the same records"""
    for r in RC.POS_ROWS:
        for inp in RC.pos_inputs(r):
            if inp.label == "planted":
                continue  # (its seed is the corpus's: kernel_cases.expected hashes with its own)
            W = RC.Whole(r, inp)
            g = inp.plan
            for first, end in ((g["origin"] + g["stride"] + 37, g["origin"] + 2 * g["stride"] + 592), (5, 6), (len(inp.seq) - 3, len(inp.seq))):
                want = K.expected(r, inp.seq, inp.offs, 0, first, end - first)
                got = W.of_range(first, end)
                K.assert_same(r.entry, got, want, (K.row_id(r), inp.label, first, end))
            K.assert_same(r.entry, W.of_range(0, W.n), W.whole(), (K.row_id(r), inp.label))


def test_the_cut_places_are_where_they_are_meant_to_be():
    for r in RC.POS_ROWS:
        mode = K.MODE[r.entry]
        for inp in RC.pos_inputs(r):
            n, g = len(inp.seq), inp.plan
            cuts = RC.two_way(inp, r.unit, r.w)
            assert {c % 16 for c in cuts if c <= 17} == set(range(16)) and {1, 16, 17} <= set(cuts)
            # the range's own plan: origin 0 up to first = 16 (17 for the window scans), 16 behind it
            assert K.P.plan_pos(mode, 16, n, r.w)["origin"] == (16 if mode == K.P.MODE_SYNCMER else 0) and K.P.plan_pos(mode, 17, n, r.w)["origin"] == 16
            T = g["origin"] + g["stride"]
            assert set(range(T - 17, T + 18)) <= set(cuts) and n - 1 in cuts and n - (r.unit + r.w - 1) in cuts
            assert {K.P.plan_pos(mode, c, n, r.w)["origin"] % 16 for c in cuts} == {0}
            # somewhere a border of the second range's tiles falls on every residue relative to the whole scan's
            assert len({(K.P.plan_pos(mode, c, n, r.w)["origin"] - g["origin"]) % g["stride"] for c in cuts}) > 8
            if inp.label == "ragged":
                assert set(K.planted_places(g)) <= set(cuts) & set(inp.offs.tolist()) and RC.short_read_followers(inp.offs, r.unit)
            if inp.label == "ragged_n":
                assert all(inp.seq[p] == ord("N") and {p - r.unit, p - 1, p, p + 1} <= set(cuts) for p in K.planted_places(g))
            if inp.label == "contig":
                a, mid, b = RC.island_of(g)
                assert bytes(inp.seq[a:b + 1]).upper() == K.ISLAND and bytes(inp.seq[mid - 1:mid + 1]).upper() == b"AA"
            if inp.label == "planted":
                assert len(inp.extra) == 3 and all(set(range(at - 2, at + r.w + 3)) <= set(cuts) for at in inp.extra)
            three = RC.three_way(inp, r.unit, r.w)
            assert {b - a for a, b in three} >= {1, 2, 16, g["stride"]} | ({r.w - 1, r.w, r.w + 1} - {0})
    planted = [K.row_id(r) for r in RC.POS_ROWS if any(i.label == "planted" for i in RC.pos_inputs(r))]
    assert len(planted) >= 3, planted


# ----------------------------------------------------------------------------- the 64-bit entries

@pytest.mark.parametrize("r", RC.POS_ROWS, ids=K.row_id)
def test_position_tiled_ranges(emu, r):
    run_row(emu, r, RC.pos_inputs(r), lambda inp: RC.cut_sets(inp, r.unit, r.w))


@pytest.mark.parametrize("r", RC.FRL_ROWS, ids=K.row_id)
def test_read_tiled_ranges(emu, r):
    """halves of one scan in different layouts: whole reads take the read-tiled plan, any other range the position-tiled one"""
    inp = RC.frl_input(r)
    sets = RC.frl_cut_sets(inp, r)
    mixed = [cs for cs in sets if len({RC.read_tiled(a, b, inp.read_len) for a, b in RC.ranges_of(cs, len(inp.seq))}) == 2]
    assert len(mixed) >= 2, mixed  # (a two-way cut off a read's start leaves both halves position-tiled: the three-way sets mix)
    run_row(emu, r, [inp], lambda _: sets, frl=True)


@pytest.mark.parametrize("k,drop_last", RC.KMER_SHAPES)
def test_dense_kmer_ranges(emu, k, drop_last):
    t0 = time.time()
    res = np.zeros(8, np.uint64)
    for inp in RC.dense_inputs(k):
        n = len(inp.seq)
        W = RC.WholeKmers(inp, k, True, K.SEED, drop_last)
        assert {d: W.of_range(0, n)[d] for d in ("count", "xor_value", "xor_hash", "sum_hash")} == O.kmer_digest(inp.seq, inp.offs, k, True, K.SEED, drop_last=drop_last)
        assert W.of_range(0, n)["count"] > 1000
        b = emu.emu_batch(O._ptr(inp.seq), n, O._ptr(inp.offs), len(inp.offs) - 1, 0)
        v, h, ok = np.zeros(n + RC.GUARD, np.uint64), np.zeros(n + RC.GUARD, np.uint64), np.zeros(n + RC.GUARD, np.uint8)
        try:
            for cuts in RC.cut_sets(inp, k, 1):
                parts = []
                for first, end in RC.ranges_of(cuts, n):
                    v[:], h[:], ok[:] = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 0xA5
                    f, cnt = RC.call_args(first, end, n)
                    emu.emu_kmers(b, f, cnt, k, K.SEED, 1 | (2 if drop_last else 0), O._ptr(v), O._ptr(h), O._ptr(ok), O._ptr(res))
                    span = end - first
                    got = dict(count=int(res[0]), xor_value=int(res[1]), xor_hash=int(res[2]), sum_hash=int(res[3]), values=v[:span].copy(), hashes=h[:span].copy(),
                               valid=ok[:span].copy())
                    RC.assert_same_kmers(got, W.of_range(first, end), (k, drop_last, inp.label, cuts, first, end))
                    assert np.all(v[span:] == 0x5A5A5A5A5A5A5A5A) and np.all(h[span:] == 0x5A5A5A5A5A5A5A5A) and np.all(ok[span:] == 0xA5), (k, cuts, first, "written behind the range")
                    parts.append(got)
                cat = dict(count=sum(p["count"] for p in parts), sum_hash=sum(p["sum_hash"] for p in parts) % 2**64,
                           xor_value=O.xor_reduce(np.array([p["xor_value"] for p in parts], np.uint64)), xor_hash=O.xor_reduce(np.array([p["xor_hash"] for p in parts], np.uint64)),
                           **{f: np.concatenate([p[f] for p in parts]) for f in ("values", "hashes", "valid")})
                RC.assert_same_kmers(cat, W.of_range(0, n), (k, drop_last, inp.label, cuts, "concatenation"))
                TALLY["cut_sets"] += 1
                TALLY["ranges"] += len(parts)
        finally:
            emu.emu_batch_free(b)
    TALLY["seconds"] += time.time() - t0


# ----------------------------------------------------------------------------- the 128-bit entries

ORIGIN128 = 1_000_000_007  # fixed in the stand-alone emulators
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
            "-Wno-unused-parameter", "-Wno-unused-function"]
MODES128 = ((1, 0), (0, 1))  # (canonical, drop_last) held against the Python models; the emulators hold all four against their own plain evaluation


@pytest.fixture(scope="module")
def exes():
    out = {}
    os.makedirs(os.path.join(EMU_DIR, "_build"), exist_ok=True)
    for name in ("emu_kmers128", "emu_minimizers128", "emu_syncmers128", "emu_records128"):
        out[name] = os.path.join(EMU_DIR, "_build", name)
        subprocess.check_call([CXX if os.path.exists(CXX) else "clang++"] + SANITIZE + (["-DBL_CPU_EMU"] if name != "emu_records128" else [])
                              + [os.path.join(EMU_DIR, name + ".cpp"), "-o", out[name]], timeout=900)
    return out


def run_list(exe, args_before, args_after, path, ranges):
    """the emulator over a list of (first, n) in one run: per range the output lines, split into words"""
    with open(path + ".ranges", "w") as f:
        f.write("".join(f"{a} {b}\n" for a, b in ranges))
    run = subprocess.run([exe, path] + [str(x) for x in args_before] + ["@" + path + ".ranges", "0"] + [str(x) for x in args_after], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = []
    for ln in run.stdout.splitlines():
        if ln.startswith("range "):
            out.append([])
        else:
            out[-1].append(ln.split())
    assert len(out) == len(ranges)
    return out


DIGEST_WORDS = {"dense": ("count", "xor_value", "aux", "xor_hash", "sum_hash"), "sample": ("count", "xor_value", "aux", "xor_hash", "xor_pos"),
                "min": ("count", "xor_value", "aux", "xor_hash", "xor_pos"), "sync": ("count", "xor_pos")}


@pytest.mark.parametrize("shape", [s for s in RC.SHAPES128 if s[0] != "records128"], ids=RC.id128)
def test_ranges_128(exes, tmp_path, shape):
    """kmers128, hash_sample128, minimizers128, syncmers128: the digest words of every range against the model's view of that range, for both
    strand modes and with and without the last k-mer of a sequence; inside the emulator every record of every range against its plain evaluation"""
    t0 = time.time()
    entry, a = shape
    line = {"kmers128": "dense", "hash_sample128": "sample", "minimizers128": "min", "syncmers128": "sync"}[entry]
    unit, w = (a[0], 1) if len(a) == 1 else ((a[0], a[1]) if entry == "minimizers128" else (a[1], a[0] - a[1] + 1))
    runs = []
    with concurrent.futures.ThreadPoolExecutor(4) as pool:  # one emulator process per input, side by side
        for inp in RC.inputs128(shape):
            n = len(inp.seq)
            path = str(tmp_path / f"{inp.label}.bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<QQ", n, len(inp.offs) - 1) + np.ascontiguousarray(inp.offs, np.uint64).tobytes() + inp.seq.tobytes())
            models = {(c, d): RC.Whole128(shape, inp, bool(c), bool(d)) for c, d in MODES128}
            sets = RC.cut_sets(inp, unit, w)
            jobs = [(first, end - first) for cuts in sets for first, end in RC.ranges_of(cuts, n)]
            if entry in ("kmers128", "hash_sample128"):
                fut = pool.submit(run_list, exes["emu_kmers128"], [a[0]], [RC.THRESHOLD128], path, jobs)
            elif entry == "minimizers128":
                fut = pool.submit(run_list, exes["emu_minimizers128"], [a[0], a[1]], [], path, jobs)
            else:
                W0 = models[MODES128[0]]
                fut = pool.submit(run_list, exes["emu_syncmers128"], [a[0], a[1]], [W0.soff, W0.eoff], path, jobs)
            runs.append((inp, models, sets, fut))
    for inp, models, sets, fut in runs:
        n, got = len(inp.seq), fut.result()
        words = DIGEST_WORDS[line]
        at = 0
        for cuts in sets:
            spans = RC.ranges_of(cuts, n)
            for c, d in MODES128:
                fold = dict.fromkeys(words, 0)
                for (first, end), lines in zip(spans, got[at:at + len(spans)]):
                    ln = [x for x in lines if x[0] == line and (int(x[1]), int(x[2])) == (c, d)]
                    assert len(ln) == 1, (RC.id128(shape), inp.label, first, end, lines)
                    vals = dict(zip(words, (int(x) for x in ln[0][3:])))
                    want = models[c, d].of_range(first, end, ORIGIN128)
                    assert vals == {k: int(want[k]) for k in words}, (RC.id128(shape), inp.label, cuts, first, end, c, d, vals)
                    for k in words:
                        fold[k] = (fold[k] + vals[k]) % 2**64 if k in ("count", "sum_hash") else fold[k] ^ vals[k]
                whole = models[c, d].of_range(0, n, ORIGIN128)
                assert fold == {k: int(whole[k]) for k in words} and whole["count"] > 5, (RC.id128(shape), inp.label, cuts, c, d, "concatenation")
            at += len(spans)
            TALLY["cut_sets128"] += 1
            TALLY["ranges128"] += len(spans)
    TALLY["seconds128"] += time.time() - t0


@pytest.mark.parametrize("shape", [s for s in RC.SHAPES128 if s[0] == "records128"], ids=RC.id128)
def test_record_ranges_128(exes, tmp_path, shape):
    """bl_scan_super_kmer_records128's emulation: the records and hashes of every range against records128_cases.Expect.of_range; the k-mers of
    the ranges of a cut set are the batch's, none twice"""
    import records128_cases as R
    from test_emu_records128 import check, run_jobs

    t0 = time.time()
    k, m = shape[1]
    runs = []
    with concurrent.futures.ThreadPoolExecutor(4) as pool:  # one emulator process per input, side by side
        for inp in RC.inputs128(shape):
            n = len(inp.seq)
            sets = RC.cut_sets(inp, m, k - m + 1)
            jobs = [(first, end - first) for cuts in sets for first, end in RC.ranges_of(cuts, n)]
            (tmp_path / inp.label).mkdir()
            runs.append((inp, sets, pool.submit(run_jobs, exes["emu_records128"], tmp_path / inp.label, inp.seq, inp.offs, 0, k, m, True, jobs)))
    for inp, sets, fut in runs:
        n, got = len(inp.seq), fut.result()
        W = RC.Whole128(shape, inp, True, False, seed=R.SEED)
        sizes = lambda recs: int(((recs[:, 3] & np.uint64(63)) + np.uint64(1)).sum()) if len(recs) else 0
        total = sizes(W.of_range(0, n)["records"])
        assert total > 1000
        at = 0
        for cuts in sets:
            spans = RC.ranges_of(cuts, n)
            for (first, end), res in zip(spans, got[at:at + len(spans)]):
                x = W.of_range(first, end)
                check(res, (x["records"], x["hashes"]), (RC.id128(shape), inp.label, cuts, first, end))
            assert sum(sizes(res[0]) for res in got[at:at + len(spans)]) == total, (RC.id128(shape), inp.label, cuts)
            at += len(spans)
            TALLY["cut_sets128"] += 1
            TALLY["ranges128"] += len(spans)
    TALLY["seconds128"] += time.time() - t0


def test_tally():
    """runs last: what the sweeps of this session covered"""
    print(f"\nrange seams, 64-bit entries through the emulation: {TALLY['cut_sets']} cut sets, {TALLY['ranges']} ranges, {TALLY['seconds']:.1f} s")
    print(f"range seams, 128-bit entries through the stand-alone emulators: {TALLY['cut_sets128']} cut sets, {TALLY['ranges128']} ranges, {TALLY['seconds128']:.1f} s")
