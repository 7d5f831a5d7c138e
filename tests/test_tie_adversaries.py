"""CPU-only: the mined pairs of tests/golden/tie_adversaries.json (two DIFFERENT keys that tie in what the fast form of an exact window kernel
keeps: 26 or 25 bits of the hash's high dword, or the whole dword) through the CPU emulation of the kernels, record for record against the
oracle, planted where the lane maps make them hard (tests/tie_plant.py).

On random data such a tie has a chance of 2^-26 .. 2^-32 per compared pair, and on repeats the tied keys are equal, so that either side is as good as
the other: without these inputs the exact fallbacks (window_argmin on the hashes, window_argmin_lds_exact, the read-tiled exact form, the
closed-syncmer kernels' second look, scan_redo_kernel) run only where they cannot be seen to be wrong.  Here the fast form alone elects the WRONG
key at every entry with teeth (winner "right"; "left" on the reverse strand of a canonical syncmer scan); the tests below first prove that on the
model (tests/hash_top_model.py: fast_argmins) and then demand the oracle's records from the emulated kernels.

The emulation mirrors launch_count_mode and launch_count_frl width for width, but builds a lane's halo from its neighbours' state where the
device hops by DPP or reads LDS: the placements at lanes 62 | 63 and at wave borders are fully meaningful only in test_gpu_tie_adversaries.py.

Breaks tried, one at a time, on a scratch copy of the tree (emulation library rebuilt, this module run; none committed), and the cases that failed.
The model and corpus tests pass under all of them; without the break all 115 cases pass.
  window_argmin compares the high dwords only                      test_emulation_windows: the 6 shapes with an hi32 entry up to w = 32 (w = 2, 16, 17, 32 and
                                                                   both specialised shapes); test_emulation_read_tiled: (31, 11) at every length and the
                                                                   super-k-mers; test_emulation_syncmers: (21, 11) and (11, 21) canonical, open
  lane_window_argmin: the exact branch never taken                 test_emulation_windows: all 36 shapes with w <= 32; test_emulation_syncmers: the 4 open
                                                                   cases on the templated widths 11, 17, 21
  lane_window_argmin_generic: the exact branch never taken         test_emulation_windows: w = 33, 48, 64; test_emulation_syncmers: (24, 8), (13, 19) open
  window_argmin_lds_exact (whole hashes) compares high dwords      test_emulation_windows: w = 48 (its hi32 entries); test_emulation_syncmers: (24, 8), (13, 19)
  lane_window_argmin_frl: the exact branch never taken             all 14 test_emulation_read_tiled cases
  phase_sync_closed_rt: the second look (closed_exact_kmers) off   all 4 closed test_emulation_syncmers cases
  closed_exact_kmers compares the high dwords only                 the same 4 cases
  the deferred exact run skipped (run_tiles: `if (sy2_tie)`)       test_emulation_syncmers[11-21-1-(0, 20)-open]
  lane_window_argmin_generic: bound 64 for 128                     test_emulation_windows[31-64-1] (tags of a pair 63 apart differ in bit 6)
  the second run of a read-tiled tile skipped (run_tiles_frl)      test_emulation_read_tiled: (31, 11) at all four lengths
  the second run of a position-tiled tile skipped (run_tiles)      test_emulation_windows[31-11-1]
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hash_top_model as T
import oracle_lib as O
import tie_plant as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

WINDOW_SHAPES, CLOSED_SHAPES, SYNC_CASES, FRL_CASES, ids = P.WINDOW_SHAPES, P.CLOSED_SHAPES, P.SYNC_CASES, P.FRL_CASES, P.ids


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    L = C.CDLL(os.path.join(EMU_DIR, "_build", "libbl_emu.so"))
    vp, u64, u = C.c_void_p, C.c_uint64, C.c_uint
    L.emu_batch.restype = vp
    L.emu_batch.argtypes = [vp, u64, vp, u64, u64]
    L.emu_batch_free.argtypes = [vp]
    L.emu_minimizers.argtypes = [vp, u64, u64, u, u, u64, u, vp, vp, vp, u64, vp]
    L.emu_super_kmers.argtypes = [vp, u64, u64, u, u, u64, u, vp, vp, vp, vp, vp, u64, vp]
    L.emu_syncmers.argtypes = [vp, u64, u64, u, u, u, u, u64, u, vp, u64, vp]
    L.emu_plan.argtypes = [C.c_int, u64, u64, u64, u64, u, u, u, vp]
    return L


# ----------------------------------------------------------------------------- the plan transcriptions

def emu_plan(emu, mode, n_bases, read_len, unit, w, canonical, first=0, n=0):
    out = np.zeros(9, np.int64)
    emu.emu_plan(mode, first, n, n_bases, read_len, unit, w, 1 if canonical else 0, O._ptr(out))
    return dict(zip(("frl", "origin", "stride", "n_tiles", "read_len", "lpr", "rpw", "ns", "nwin"), (int(x) for x in out)))


def test_plans_match_the_emulation(emu):
    for w in range(2, 65):
        for mode in (P.MODE_MINIMIZER, P.MODE_SUPERKMER, P.MODE_SYNCMER):
            n = P.pos_length(w)
            g, q = P.plan_pos(mode, 0, n, w), emu_plan(emu, mode, n, 0, 21, w, 1)
            assert (q["frl"], q["origin"], q["stride"], q["n_tiles"]) == (0, g["origin"], g["stride"], g["n_tiles"]), (mode, w)
    seen_general_31 = False
    for mode, unit, w, canonical, L in FRL_CASES + [(P.MODE_MINIMIZER, 31, 11, 1, L) for L in range(60, 320, 7)] + [(P.MODE_MINIMIZER, 21, 12, 1, 100)]:
        for n_reads in (1, 149, 1000):
            g, q = P.plan_frl(mode, L * n_reads, L, unit, w, canonical), emu_plan(emu, mode, L * n_reads, L, unit, w, canonical)
            assert bool(q["frl"]) == (g is not None), (mode, unit, w, L)
            if g:
                assert all(q[k] == g[k] for k in ("origin", "stride", "n_tiles", "read_len", "lpr", "rpw", "ns", "nwin")), (mode, unit, w, L)
    for mode, unit, w, canonical, L in FRL_CASES:
        g = P.plan_frl(mode, L * 149, L, unit, w, canonical)
        assert g is not None, "every read-tiled case of this module and of test_gpu_tie_adversaries.py takes the read-tiled layout"
        if (unit, w) == (31, 11):
            assert (g["ns"] in (14, 15, 16) and g["ns"] * g["lpr"] >= g["nu"]) if L != 79 else g["ns"] == 16
            seen_general_31 |= L == 79 and (g["nu"] + g["lpr"] - 1) // g["lpr"] < 14
        else:
            assert g["ns"] == 16
    assert seen_general_31


# ----------------------------------------------------------------------------- the corpus

def test_every_entry_is_what_it_claims():
    for e in P.corpus():
        unit, w, seed, canonical, cls = e["unit"], e["w"], e["seed"], e["canonical"], e["class"]
        keys = [int(k, 16) for k in e["keys"]]
        a, b = P.pair_of(e)
        assert len(e["bases"]) == unit + w - 1 and cls in ("p26", "p25", "hi32") and e["winner"] in ("left", "right")
        if e["mode"] == "window":
            u = T.units(e["bases"], unit, bool(canonical))
            ov, _ = O.units(e["bases"], np.array([0, len(e["bases"])], np.uint64), unit, bool(canonical))
            assert np.array_equal(ov[:w], u)
        else:
            assert seed == 0 and unit + w - 1 <= 32 and e["strand"] in ("forward", "reverse")
            k = unit + w - 1
            kv = int(T.units(e["bases"], k, False)[0])
            rc = int(T.revcomp_value(np.array([kv], np.uint64), k)[0])
            reverse = bool(canonical) and rc < kv
            assert (e["strand"] == "reverse") == reverse and (not canonical or rc != kv)
            u = T.units(T.revcomp_str(e["bases"]) if reverse else e["bases"], unit, False)  # the s-mers of the strand that counts, in its order
            assert 0 <= a < b <= w - 1
        h = T.hash64(u, seed)
        assert np.array_equal(h, O.hash64_np(u, seed))
        assert [int(u[a]), int(u[b])] == keys and keys[0] != keys[1]
        ha, hb = int(h[a]), int(h[b])
        assert T.tie_class(ha, hb) == cls
        if cls == "p26":
            assert ha >> 38 == hb >> 38 and ha >> 32 != hb >> 32
        elif cls == "p25":
            assert ha >> 39 == hb >> 39 and (ha ^ hb) >> 38 & 1
        else:
            assert ha >> 32 == hb >> 32 and ha & 0xFFFFFFFF != hb & 0xFFFFFFFF
        others = np.delete(h, [a, b])
        assert len(others) == 0 or int(others.min()) >> 39 > max(ha, hb) >> 39  # every other unit is larger in what the coarsest form keeps
        t = int(h.argmin())
        assert t == P.true_offset(e) and t in (a, b)
        f = T.fast_argmins(h, w)
        for form in {"p26": ("p26", "p25"), "p25": ("p25",), "hi32": ("hi32", "p26", "p25")}[cls]:
            assert int(f[form + "_left"][0]) == a and int(f[form + "_right"][0]) == b  # the form ties: the tag (or a fixed side) decides
        for form in {"p26": ("hi32",), "p25": ("hi32", "p26"), "hi32": ()}[cls]:
            assert int(f[form + "_left"][0]) == int(f[form + "_right"][0]) == t      # a finer form does not tie
        assert int(f["true_left"][0]) == int(f["true_right"][0]) == t
        # teeth: the fast form's choice (the lower offset along the strand) is not the true one; control: it is
        assert P.has_teeth(e) == (t == b)
        if e["mode"] == "window":
            assert P.has_teeth(e) == (e["winner"] == "right")
        else:
            assert P.has_teeth(e) == (e["winner"] == ("right" if e["strand"] == "forward" else "left"))
            off, rev = T.syncmer_offsets(e["bases"], unit + w - 1, unit, seed, bool(canonical))
            assert int(off[0]) == t and bool(rev[0]) == (e["strand"] == "reverse")
            for soff, eoff in ([(0, w - 1), (w - 1, 0)] if (a, b) != (0, w - 1) else P.open_offsets(w)):
                assert (a in (soff, eoff)) != (b in (soff, eoff))  # the test's offsets name exactly one of the pair
                n0, _ = O.syncmers(e["bases"], np.array([0, len(e["bases"])], np.uint64), unit + w - 1, unit, soff, eoff, bool(canonical))
                assert n0 == int(t in (soff, eoff))


def test_coverage():
    """the lists of the issue, literally"""
    have = {(e["mode"], e["unit"], e["w"], e["canonical"], e["class"], e["winner"]) + ((tuple(e["pair"]), e["strand"]) if e["mode"] == "syncmer" else ())
            for e in P.corpus()}
    win = lambda w, cls, winner, canon=None, unit=None: any(
        x[0] == "window" and x[2] == w and x[4] == cls and x[5] == winner and canon in (None, x[3]) and unit in (None, x[1]) for x in have)
    for side in ("left", "right"):
        for w in range(2, 33):
            assert win(w, "p26", side), w
        for w in (33, 48, 64):
            assert win(w, "p26", side) and win(w, "p25", side), w
        for unit, w in ((31, 11), (15, 17)):
            assert win(w, "p26", side, 1, unit) and win(w, "hi32", side, 1, unit)
        for w in (2, 16, 17, 32, 48):
            assert win(w, "hi32", side), w
        for w in (2, 11, 32):
            assert win(w, "p26", side, 0) and win(w, "p26", side, 1)
    syn = lambda s, w, canon, cls, winner, strand, closed: any(
        x[0] == "syncmer" and x[1:6] == (s, w, canon, cls, winner) and x[7] == strand and (x[6] != (0, w - 1)) == closed for x in have)
    for side in ("left", "right"):
        for s, w, canon in ((21, 11, 1), (15, 17, 0), (11, 21, 0), (11, 21, 1), (24, 8, 1), (13, 19, 1)):  # templated 11, 17, 21; the deferred (21, 11); run time <= 16, 17 .. 32
            for strand in ("forward", "reverse") if canon else ("forward",):
                assert syn(s, w, canon, "p26", side, strand, False), (s, w)
        for s, w in ((24, 8), (13, 19)):
            assert syn(s, w, 1, "p25", side, "forward", False) and syn(s, w, 1, "p25", side, "reverse", False)
        for s, w in ((19, 13), (12, 20)):  # closed: w <= 17 and 18 .. 32, the whole dword
            for strand in ("forward", "reverse"):
                assert syn(s, w, 1, "hi32", side, strand, True)
    for s, w, canon, pr in CLOSED_SHAPES:
        assert (pr[0] == 0) != (pr[1] == w - 1)  # an end s-mer against an inner one
    assert {pr[0] == 0 for s, w, c, pr in CLOSED_SHAPES if w == 13} == {True, False} == {pr[0] == 0 for s, w, c, pr in CLOSED_SHAPES if w == 20}
    assert len(WINDOW_SHAPES) == 39 and all(e["class"] == "hi32" for e in P.corpus() if e["mode"] == "syncmer" and tuple(e["pair"]) != (0, e["w"] - 1))


# ----------------------------------------------------------------------------- what the fast form alone would report

def teeth(batch):
    return [(at, e) for at, e in batch["plants"] if P.has_teeth(e)]


@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=ids)
def test_window_records_against_the_model(shape):
    """the oracle's records are the model's true ones and NOT what the fast form of that width alone would give, at every plant with teeth"""
    unit, w, canonical = shape
    b = P.pos_batch("window", unit, w, canonical)
    s, seed = bytes(b["seq"]).decode(), b["seed"]
    assert len(teeth(b)) >= 16 and {e["winner"] for _, e in b["plants"]} == {"left", "right"}
    one = np.array([0, len(s)], np.uint64)
    _, p, _ = O.minimizers(b["seq"], one, unit, w, seed, bool(canonical))
    assert np.array_equal(p, P.minimizer_positions(s, unit, w, seed, canonical, "true_left"))
    fast = P.minimizer_positions(s, unit, w, seed, canonical, P.fast_form(w))
    assert not np.array_equal(p, fast)
    f = T.fast_argmins(T.hash64(T.units(s, unit, bool(canonical)), seed), w)
    mn, fp, mp, sz, hs = O.super_kmers(b["seq"], one, unit + w - 1, unit, seed, bool(canonical))
    oracle_mm = set((fp + mp.astype(np.uint64)).tolist())
    true_set, fast_set = set(p.tolist()), set(fast.tolist())
    for at, e in b["plants"]:
        ties = e["class"] != "p25" or w > 32  # (a 25-bit tie is no tie for the 6-bit-tag kernels)
        chosen, true = int(f[P.fast_form(w)][at]), int(f["true_left"][at])
        assert true == P.true_offset(e) and (chosen != true) == (P.has_teeth(e) and ties)
        if P.has_teeth(e):  # the entry's first unit is a record of the fast form alone, of no exact scan
            assert at + w - 1 in true_set and at + w - 1 in oracle_mm and at not in true_set and at not in oracle_mm
            assert (at in fast_set) == ties
    # the control: no window anywhere near a tie
    c = bytes(b["control"]).decode()
    assert np.array_equal(P.minimizer_positions(c, unit, w, seed, canonical, "p25_left"), P.minimizer_positions(c, unit, w, seed, canonical, "true_left"))


@pytest.mark.parametrize("case", SYNC_CASES, ids=ids)
def test_syncmer_records_against_the_model(case):
    s, w, canonical, pair, kind = case
    k = s + w - 1
    b = P.pos_batch("syncmer", s, w, canonical, pair=pair)
    seq = bytes(b["seq"]).decode()
    assert len(teeth(b)) >= 16
    one = np.array([0, len(seq)], np.uint64)
    for soff, eoff in (P.open_offsets(w) if kind == "open" else [(0, w - 1), (w - 1, 0)]):
        n0, pos = O.syncmers(b["seq"], one, k, s, soff, eoff, bool(canonical))
        assert np.array_equal(pos, P.syncmer_positions(seq, k, s, 0, canonical, (soff, eoff)))
        true = set(pos.tolist())
        for cls in {e["class"] for _, e in b["plants"]}:
            fast = set(P.syncmer_positions(seq, k, s, 0, canonical, (soff, eoff), form=cls).tolist())
            for at, e in b["plants"]:
                if e["class"] == cls:
                    assert (at in true) == (P.true_offset(e) in (soff, eoff))
                    assert ((at in fast) != (at in true)) == P.has_teeth(e)  # the wrong winner flips the verdict


# ----------------------------------------------------------------------------- through the emulated kernels

def emu_minimizers(emu, seq, offsets, read_len, unit, w, seed, canonical, first=0, n=0):
    b = emu.emu_batch(O._ptr(seq), len(seq), O._ptr(offsets) if offsets is not None else None, len(offsets) - 1 if offsets is not None else 0, read_len)
    cap = len(seq) + 1
    v, p, h, res = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(8, np.uint64)
    frl = emu.emu_frl_scans()
    emu.emu_minimizers(b, first, n, unit, w, seed, 1 if canonical else 0, O._ptr(v), O._ptr(p), O._ptr(h), cap, O._ptr(res))
    emu.emu_batch_free(b)
    m = int(res[0])
    return v[:m], p[:m], h[:m], emu.emu_frl_scans() - frl


def emu_super_kmers(emu, seq, offsets, read_len, k, m, seed, canonical, first=0, n=0):
    b = emu.emu_batch(O._ptr(seq), len(seq), O._ptr(offsets) if offsets is not None else None, len(offsets) - 1 if offsets is not None else 0, read_len)
    cap = len(seq) + 1
    mn, fp, hs, res = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(8, np.uint64)
    mp, sz = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    frl = emu.emu_frl_scans()
    emu.emu_super_kmers(b, first, n, k, m, seed, 1 if canonical else 0, O._ptr(mn), O._ptr(fp), O._ptr(mp), O._ptr(sz), O._ptr(hs), cap, O._ptr(res))
    emu.emu_batch_free(b)
    c = int(res[0])
    return mn[:c], fp[:c], mp[:c], sz[:c], hs[:c], emu.emu_frl_scans() - frl


def same(got, want, what):
    assert len(got) >= len(want)
    for g, x, name in zip(got, want, what):
        assert len(g) == len(x) and np.array_equal(g, x), name


MIN_FIELDS = ("values", "positions", "hashes")
SK_FIELDS = ("minimizers", "first_pos", "mm_pos", "sizes", "hashes")


@pytest.mark.parametrize("shape", WINDOW_SHAPES, ids=ids)
def test_emulation_windows(emu, shape):
    """minimizers and super-k-mers, one sequence and the ragged cut of the same bases, and the scan as two ranges cut inside a planted window"""
    unit, w, canonical = shape
    b = P.pos_batch("window", unit, w, canonical)
    seq, seed, k = b["seq"], b["seed"], unit + w - 1
    for offsets in (None, b["offsets"]):
        offs = offsets if offsets is not None else np.array([0, len(seq)], np.uint64)
        want = O.minimizers(seq, offs, unit, w, seed, bool(canonical))
        same(emu_minimizers(emu, seq, offsets, 0, unit, w, seed, canonical), want, MIN_FIELDS)
        want_sk = O.super_kmers(seq, offs, k, unit, seed, bool(canonical))
        same(emu_super_kmers(emu, seq, offsets, 0, k, unit, seed, canonical), want_sk, SK_FIELDS)
    cut = [at for at, e in b["plants"] if P.has_teeth(e) and at > len(seq) // 2][0] + w // 2
    parts = [emu_minimizers(emu, seq, None, 0, unit, w, seed, canonical, first, n)[:3] for first, n in ((0, cut), (cut, len(seq) - cut))]
    # an occurrence belongs to the range in which its first electing window starts: the plain concatenation is the whole scan
    # (every cut of every planted window: test_range_seams.py)
    want = O.minimizers(seq, np.array([0, len(seq)], np.uint64), unit, w, seed, bool(canonical))
    same([np.concatenate([x[i] for x in parts]) for i in range(3)], want, MIN_FIELDS)
    same(emu_minimizers(emu, b["control"], None, 0, unit, w, seed, canonical), O.minimizers(b["control"], np.array([0, len(seq)], np.uint64), unit, w, seed, bool(canonical)),
         MIN_FIELDS)


@pytest.mark.parametrize("case", FRL_CASES, ids=ids)
def test_emulation_read_tiled(emu, case):
    mode, unit, w, canonical, L = case
    b = P.frl_batch(mode, unit, w, canonical, L)
    seq, seed = b["seq"], b["seed"]
    assert len(teeth(b)) >= 16 and b["plan"]["n_tiles"] == 4
    offs = O.fixed_offsets(len(seq), L)
    if mode == P.MODE_MINIMIZER:
        got = emu_minimizers(emu, seq, None, L, unit, w, seed, canonical)
        same(got, O.minimizers(seq, offs, unit, w, seed, bool(canonical)), MIN_FIELDS)
    else:
        got = emu_super_kmers(emu, seq, None, L, unit + w - 1, unit, seed, canonical)
        same(got, O.super_kmers(seq, offs, unit + w - 1, unit, seed, bool(canonical)), SK_FIELDS)
    assert got[-1] == 1, "the read-tiled layout was taken"
    # ranges of whole reads, cut inside a tile that holds plants
    if mode == P.MODE_MINIMIZER:
        cut = (b["plan"]["reads_per_tile"] + 3) * L
        parts = [emu_minimizers(emu, seq, None, L, unit, w, seed, canonical, first, n)[:3] for first, n in ((0, cut), (cut, len(seq) - cut))]
        same([np.concatenate([x[i] for x in parts]) for i in range(3)], O.minimizers(seq, offs, unit, w, seed, bool(canonical)), MIN_FIELDS)


@pytest.mark.parametrize("case", SYNC_CASES, ids=ids)
def test_emulation_syncmers(emu, case):
    s, w, canonical, pair, kind = case
    k = s + w - 1
    b = P.pos_batch("syncmer", s, w, canonical, pair=pair)
    seq = b["seq"]
    deferred = (s, w, canonical) == (11, 21, 1) and kind == "open"
    for offsets in (None, b["offsets"]):
        offs = offsets if offsets is not None else np.array([0, len(seq)], np.uint64)
        for soff, eoff in (P.open_offsets(w) if kind == "open" else [(0, w - 1), (w - 1, 0)]):
            for drop_last in (False, True):
                n0, pos = O.syncmers(seq, offs, k, s, soff, eoff, bool(canonical), drop_last=drop_last)
                eb = emu.emu_batch(O._ptr(seq), len(seq), O._ptr(offsets) if offsets is not None else None, len(offs) - 1 if offsets is not None else 0, 0)
                got, res = np.zeros(len(seq) + 1, np.uint64), np.zeros(8, np.uint64)
                before = emu.emu_sy2_redone()
                emu.emu_syncmers(eb, 0, 0, k, s, soff, eoff, 0, (1 if canonical else 0) | (2 if drop_last else 0), O._ptr(got), len(got), O._ptr(res))
                emu.emu_batch_free(eb)
                assert int(res[0]) == n0 and np.array_equal(got[:n0], pos), (soff, eoff, drop_last)
                if deferred:  # every tile holds a plant: each is decided a second time
                    assert emu.emu_sy2_redone() - before >= 4
