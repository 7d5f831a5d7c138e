"""The batches of test_tie_adversaries.py (tests/tie_plant.py: mined pairs of DIFFERENT keys that tie in what the fast form of an exact window
kernel keeps, planted across the lane maps) through the C ABI, record for record against the oracle.  One case per (family, w).  Here the halos
come by DPP hops and through LDS as on no CPU: the placements at lanes 62 | 63, at wave borders and in a wave's last read are checked with the
device's own halo only in this module.  Every comparison is exact equality of arrays.

Which scans take the read-tiled layout cannot be read off a Result: test_tie_adversaries.py::test_plans_match_the_emulation asserts that
plan_scan_frl_for says yes for every case of FRL_CASES (and which units-per-lane form it gives)."""
import numpy as np
import pytest

import oracle_lib as O
import tie_plant as P

pytestmark = pytest.mark.gpu

MIN_FIELDS = ("values", "positions", "hashes")
SK_FIELDS = ("minimizers", "first_pos", "mm_pos", "sizes", "hashes")
SPECIALISED = {(31, 11, 1), (15, 17, 1)}


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def same(got, want, fields, what):
    assert got["count"] == len(want[0]), what
    for name, x in zip(fields, want):
        assert np.array_equal(np.asarray(got[name]).astype(x.dtype), x), (what, name)


def redone_of(ctx, b, unit, w, seed, canonical):
    import biolib_amd as B

    cap = b.n_bases + 1
    v, p, h = ctx.empty_u64(cap), ctx.empty_u64(cap), ctx.empty_u64(cap)
    r = b.minimizers_raw(unit, w, seed, (B.FLAG_CANONICAL if canonical else 0) | B.FLAG_SYNC, values=v, positions=p, hashes=h, capacity=cap)
    return int(r.redone)


def one(n):
    return np.array([0, n], np.uint64)


def teeth(batch):
    return [(at, e) for at, e in batch["plants"] if P.has_teeth(e)]


@pytest.mark.parametrize("shape", P.WINDOW_SHAPES, ids=P.ids)
def test_position_tiled(ctx, shape):
    """minimizers (unit, w) and super-k-mers (m = unit, k = unit + w - 1), one sequence and a ragged cut of the same bases, default and exact windows"""
    unit, w, canonical = shape
    bt = P.pos_batch("window", unit, w, canonical)
    seq, seed, k = bt["seq"], bt["seed"], unit + w - 1
    assert len(teeth(bt)) >= 16
    for offsets in (None, bt["offsets"]):
        offs = one(len(seq)) if offsets is None else offsets
        want = O.minimizers(seq, offs, unit, w, seed, bool(canonical))
        want_sk = O.super_kmers(seq, offs, k, unit, seed, bool(canonical))
        b = ctx.upload(seq) if offsets is None else ctx.upload(seq, offsets=offsets)
        try:
            for exact in (False, True):
                try:
                    ctx.set_exact_windows(exact)
                    what = (shape, "ragged" if offsets is not None else "one sequence", "exact windows" if exact else "default")
                    same(b.minimizers(unit, w, seed=seed, canonical=bool(canonical)), want, MIN_FIELDS, what)
                    same(b.super_kmers(k, unit, seed=seed, canonical=bool(canonical)), want_sk, SK_FIELDS, what)
                    if exact and shape in SPECIALISED:
                        assert redone_of(ctx, b, unit, w, seed, canonical) == 0
                finally:
                    ctx.set_exact_windows(False)
        finally:
            b.close()


@pytest.mark.parametrize("case", P.FRL_CASES, ids=P.ids)
def test_read_tiled(ctx, case):
    """reads of one length: the general read-tiled kernels (w = 5, 10, 11, 19; super-k-mers at 17) and, for canonical (31, 11), the kernels on
    murmur64_top with their second run and, under exact windows, the exact ns = 14 / 15 / 16 kernels (79 bp: the planner's general 16-units-per-lane layout)"""
    mode, unit, w, canonical, L = case
    bt = P.frl_batch(mode, unit, w, canonical, L)
    seq, seed = bt["seq"], bt["seed"]
    assert len(teeth(bt)) >= 16
    offs = O.fixed_offsets(len(seq), L)
    b = ctx.upload(seq, read_len=L)
    try:
        for exact in (False, True):
            try:
                ctx.set_exact_windows(exact)
                if mode == P.MODE_MINIMIZER:
                    same(b.minimizers(unit, w, seed=seed, canonical=bool(canonical)), O.minimizers(seq, offs, unit, w, seed, bool(canonical)), MIN_FIELDS, (case, exact))
                    if exact and (unit, w, canonical) in SPECIALISED:
                        assert redone_of(ctx, b, unit, w, seed, canonical) == 0
                else:
                    same(b.super_kmers(unit + w - 1, unit, seed=seed, canonical=bool(canonical)), O.super_kmers(seq, offs, unit + w - 1, unit, seed, bool(canonical)),
                         SK_FIELDS, (case, exact))
            finally:
                ctx.set_exact_windows(False)
    finally:
        b.close()


@pytest.mark.parametrize("case", P.SYNC_CASES, ids=P.ids)
def test_syncmers(ctx, case):
    """open offsets on the templated and the run-time widths and on the (31, 11) kernel whose exact form is deferred; closed offsets both ways
    round, also under exact windows (the argmin kernels); with and without the last k-mer of a sequence"""
    s, w, canonical, pair, kind = case
    k = s + w - 1
    bt = P.pos_batch("syncmer", s, w, canonical, pair=pair)
    seq = bt["seq"]
    assert len(teeth(bt)) >= 16
    deferred = (s, w, canonical) == (11, 21, 1) and kind == "open"
    for offsets in (None, bt["offsets"]):
        offs = one(len(seq)) if offsets is None else offsets
        b = ctx.upload(seq) if offsets is None else ctx.upload(seq, offsets=offsets)
        try:
            for soff, eoff in (P.open_offsets(w) if kind == "open" else [(0, w - 1), (w - 1, 0)]):
                for drop_last in (False, True):
                    n0, pos = O.syncmers(seq, offs, k, s, soff, eoff, bool(canonical), drop_last=drop_last)
                    for exact in (False, True):
                        try:
                            ctx.set_exact_windows(exact)
                            got = b.syncmers(k, s, soff, eoff, seed=0, canonical=bool(canonical), drop_last=drop_last)
                        finally:
                            ctx.set_exact_windows(False)
                        assert got["count"] == n0 and np.array_equal(got["positions"], pos), (case, soff, eoff, drop_last, exact)
                if deferred:  # every tile holds plants: each is listed for its exact second run
                    r = b.syncmers_raw(k, s, soff, eoff, 0, 1 | 4)
                    assert int(r.count) == O.syncmers(seq, offs, k, s, soff, eoff, True)[0]
                    assert int(r.redone) >= 4
        finally:
            b.close()


def concat(parts, fields):
    return {"count": sum(p["count"] for p in parts), **{f: np.concatenate([p[f] for p in parts]) for f in fields}}


@pytest.mark.parametrize("shape", [(31, 11, 1), (15, 17, 1), (27, 16, 0), (21, 33, 0), (25, 48, 1)], ids=P.ids)
def test_minimizer_ranges(ctx, shape):
    """the scan as two ranges cut inside a planted window (a range reports the windows that start in it; ranges with first != 0 take other kernel
    variants): the plain concatenation is the whole scan, since an occurrence that windows on both sides of the cut elect belongs to the range in
    which its first electing window starts (include/biolib_amd.h; every cut of every planted window: test_gpu_range_seams.py)"""
    unit, w, canonical = shape
    bt = P.pos_batch("window", unit, w, canonical)
    seq, seed = bt["seq"], bt["seed"]
    want = O.minimizers(seq, one(len(seq)), unit, w, seed, bool(canonical))
    b = ctx.upload(seq)
    try:
        for pick in (len(teeth(bt)) // 3, 2 * len(teeth(bt)) // 3):
            cut = teeth(bt)[pick][0] + w // 2
            parts = [b.minimizers(unit, w, seed=seed, canonical=bool(canonical), first=f, n=n) for f, n in ((0, cut), (cut, len(seq) - cut))]
            same(concat(parts, MIN_FIELDS), want, MIN_FIELDS, (shape, cut))
    finally:
        b.close()


@pytest.mark.parametrize("case", [(P.MODE_MINIMIZER, 31, 11, 1, 150), (P.MODE_MINIMIZER, 21, 19, 1, 100)], ids=P.ids)
def test_read_tiled_ranges(ctx, case):
    mode, unit, w, canonical, L = case
    bt = P.frl_batch(mode, unit, w, canonical, L)
    seq, seed = bt["seq"], bt["seed"]
    want = O.minimizers(seq, O.fixed_offsets(len(seq), L), unit, w, seed, bool(canonical))
    cut = (bt["plan"]["reads_per_tile"] + 3) * L
    b = ctx.upload(seq, read_len=L)
    try:
        parts = [b.minimizers(unit, w, seed=seed, canonical=bool(canonical), first=f, n=n) for f, n in ((0, cut), (cut, len(seq) - cut))]
        same(concat(parts, MIN_FIELDS), want, MIN_FIELDS, case)
    finally:
        b.close()


@pytest.mark.parametrize("case", [c for c in P.SYNC_CASES if (c[0], c[1]) in ((11, 21), (13, 19), (19, 13))][:4], ids=P.ids)
def test_syncmer_ranges(ctx, case):
    s, w, canonical, pair, kind = case
    k = s + w - 1
    bt = P.pos_batch("syncmer", s, w, canonical, pair=pair)
    seq = bt["seq"]
    cut = teeth(bt)[len(teeth(bt)) // 2][0] + w // 2  # inside a planted k-mer
    b = ctx.upload(seq)
    try:
        for soff, eoff in (P.open_offsets(w) if kind == "open" else [(0, w - 1), (w - 1, 0)]):
            n0, pos = O.syncmers(seq, one(len(seq)), k, s, soff, eoff, bool(canonical))
            parts = [b.syncmers(k, s, soff, eoff, seed=0, canonical=bool(canonical), first=f, n=n) for f, n in ((0, cut), (cut, len(seq) - cut))]
            got = np.concatenate([p["positions"] for p in parts])
            assert len(got) == n0 and np.array_equal(got, pos), (case, soff, eoff)
    finally:
        b.close()
