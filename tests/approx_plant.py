"""Batches that plant the entries of tests/golden/approx_adversaries.json where the lane maps of the pass-1 kernels make them hard, and
what tests/hash_top_model.py says about those batches.  TEST INFRASTRUCTURE shared by test_approx_adversaries.py (CPU emulation) and
test_gpu_approx_adversaries.py.

Geometry used (bl_scan_core.hpp: plan_scan, plan_scan_frl; all for canonical 31-mers, w = 11):
  read-tiled   a read of L bases has nu = L - 30 units on lpr = ceil(nu / 16) lanes, ns = ceil(nu / lpr) units per lane; lane j owns the
               units and windows j * ns ..; a wave takes rpw reads, a tile 4 * rpw; lane 63 is the last lane of a wave's last read when
               rpw * lpr == 64.  Dword form: top_plus_one.
  position-tiled  tile t, wave v starts at ws = -16 + 4032 t + 1008 v; lane l holds positions ws + 16 l .. + 15 and decides the windows
               that start one position later; lane 63 owns none: its units are only the halo of lane 62.  Dword form: top.
  closed syncmers (k = 31, s = 11)  position-tiled with a halo of 32: wave v of tile t starts at 3968 t + 992 v, lane l decides the k-mers at
               ws + 16 l .. + 15, lanes 62 and 63 own none.  Dword form: top_plus_one of 11-mers that are not canonical themselves.

On the device lane 63 of a read-tiled wave takes its halo by a rotation (lane 0's keys); the CPU emulation gives it pad keys.  The "lanes 62 / 63"
placements are therefore checked with the device's own halo only by test_gpu_approx_adversaries.py.
"""
import json
import os

import numpy as np

import hash_top_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
UNIT, W, SEED = 31, 11, 42
SPAN = UNIT + W - 1  # bases of one window
POS_STRIDE, POS_WAVE, POS_ORIGIN = 4032, 1008, -16


def corpus():
    with open(os.path.join(HERE, "golden", "approx_adversaries.json")) as f:
        return json.load(f)["entries"]


def entries(form, classes=None, unit=UNIT):
    return [e for e in corpus() if e["form"] == form and e["unit"] == unit and (classes is None or e["class"] in classes)]


# one entry per batch, at every spot: a window that needs its second look never shares all of its tiles with one that gets it anyway
WINDOW_CASES = ("misordered_one_apart-left", "misordered_one_apart-right", "one_apart_same_order", "equal_prefix")
KEY_CLASSES = ("near_wrap", "wrap", "wrap_plus_one")
CLOSED_CLASSES = ("closed_misordered_hit", "closed_misordered_miss", "closed_one_apart_same", "closed_wrap_plus_one", "closed_wrap")


def case_entries(form, case):
    cls, _, winner = case.partition("-")
    es = [e for e in entries(form, (cls,)) if not winner or e["winner"] == winner]
    assert len(es) == 1
    return es


def frl_plan(L):
    nu = L - UNIT + 1
    lpr = (nu + 15) // 16
    ns = (nu + lpr - 1) // lpr
    rpw = min(64 // lpr, (512 * 16 - 64 - 32) // 4 // L)
    return dict(nu=nu, lpr=lpr, ns=ns, rpw=rpw, nwin=nu - W + 1, reads_per_tile=4 * rpw)


def random_bases(seed, n):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].copy()


def plant(seq, at, bases):
    b = np.frombuffer(bases.encode(), np.uint8)
    seq[at:at + len(b)] = b


def frl_spots(L, n_reads):
    """(read, offset of the window inside the read, what it is hard for) for window entries of SPAN bases"""
    g = frl_plan(L)
    ns, rpt, nwin = g["ns"], g["reads_per_tile"], g["nwin"]
    last_of_wave = g["rpw"] - 1  # its last lane is lane 63 when the wave is full
    spots = [
        (1, ns, "inside one lane" if ns >= W else "lane border"),
        (3, ns - 5, "split across a lane border"),
        (last_of_wave, min((g["lpr"] - 1) * ns - 5, nwin - 1), "split across the border of the read's last two lanes (lanes 62 / 63 of a full wave)"),
        (rpt + 2, 0, "first window of a read"),
        (2 * rpt + last_of_wave, nwin - 1, "last window of a read, in the wave's last lane"),
        (n_reads - 1, nwin // 2, "last, partial tile"),
    ]
    return [(r, o, why) for (r, o, why) in spots if r < n_reads]


FRL_KEY_TILES = 6


def frl_key_spots(L, n_reads):
    """(read, offset of the unit) for single keys, ONE PER TILE (a tile's redo count is all the evidence a key that changes no record leaves):
    every lane role, and in tile 2 the read's last unit, which a lane may hold without owning a window (143 bp)"""
    g = frl_plan(L)
    ns, rpt, nu = g["ns"], g["reads_per_tile"], g["nu"]
    assert n_reads == (FRL_KEY_TILES - 1) * rpt + 5
    return [(0, 0), (rpt + 2, ns - 1), (2 * rpt + g["rpw"] - 1, nu - 1), (3 * rpt + 1, ns), (4 * rpt + 3, nu - 3), (n_reads - 1, nu // 2)]


def pos_ws(tile, wave):
    return POS_ORIGIN + POS_STRIDE * tile + POS_WAVE * wave


def pos_spots(n):
    """start positions of planted windows in one sequence of n bases (position-tiled layout)"""
    return [
        (0, "first window of the sequence"),
        (pos_ws(0, 1) + 16 * 5 + 1, "inside one lane"),
        (pos_ws(0, 2) + 16 * 9 + 10, "split across a lane border"),
        (pos_ws(0, 3) + 1000, "second key in lane 63 of the tile's last wave: the halo of lane 62, and the next tile's lane 0"),
        (pos_ws(1, 1) + 1000, "second key in lane 63 of an inner wave"),
        (n - SPAN, "last window, in the last, partial tile"),
    ]


def pos_key_spots(n):
    return [(pos_ws(0, 3) + 1010, "lane 63 of the tile's last wave: owns no window"), (pos_ws(1, 0) + 1012, "lane 63 of wave 0"), (pos_ws(1, 2) + 500, "an owning lane"),
            (n - UNIT, "last unit")]


# ----------------------------------------------------------------------------- what the model says about a batch

def redo_bounds(seq, read_len, form):
    """(tiles that MUST be decided again, tiles that MAY be) by the model.
    must: the tile owns a window whose prefix argmin the rule cannot vouch for (hash_top_model.must_redo).
    may : the tile holds two units fewer than 32 positions apart (any lane's keys: at most 16 + 11 - 1) whose prefixes are two or
          fewer apart -- the kernels fold the distance of every pair of keys they compare, and a packed-key distance below 128 reaches
          from equal prefixes to prefixes two apart -- or a key a wrap guard fires for.  Units that straddle reads are included: lanes hash them.
          Position-tiled: the last tile too when it reaches 48 or more positions past the end of the bases -- what it stages there reads as
          code 0, and lanes that own (non-existent) windows there hold the same all-zero unit several times over."""
    s = bytes(seq).decode()
    must, may = set(), set()
    if read_len:
        g = frl_plan(read_len)
        n_reads = len(s) // read_len
        for r in range(n_reads):
            u = T.units(s[r * read_len:(r + 1) * read_len], UNIT, True)
            if T.must_redo(u, SEED, form, W).any():
                must.add(r // g["reads_per_tile"])
        tile_of = lambda pos: min(pos // read_len, n_reads - 1) // g["reads_per_tile"]
    else:
        u = T.units(s, UNIT, True)
        hit = np.flatnonzero(T.must_redo(u, SEED, form, W))  # window at position x is decided by the owner of position x - 1
        must.update(int((x - 1 - POS_ORIGIN) // POS_STRIDE) for x in hit)
        n_tiles = (len(s) - 1 - POS_ORIGIN) // POS_STRIDE + 1
        if POS_ORIGIN + POS_STRIDE * n_tiles >= len(s) + 48:
            may.add(n_tiles - 1)
    u = T.units(s, UNIT, True)
    a = T.approx(u, SEED, form)
    p = T.prefix(a).astype(np.int64)
    guard = T.near_wrap(u, SEED, form) | T.wraps(u, SEED, form)
    close = np.zeros(len(u), bool)
    for d in range(1, 32):
        near = np.abs(p[d:] - p[:-d]) <= 2
        close[:-d] |= near
        close[d:] |= near
    for x in np.flatnonzero(close | guard):
        if read_len:
            may.add(tile_of(int(x)))
            may.add(tile_of(int(x) + SPAN))
        else:  # a position may be staged by two tiles (halo): charge both
            for y in (int(x) - 32, int(x) + 32):
                t = (y - POS_ORIGIN) // POS_STRIDE
                if 0 <= t < n_tiles:
                    may.add(int(t))
    return must, may | must


def frl_batch(entry_list, L, n_reads, seed, keys=False):
    """random reads with the entries planted at the spots, cycling through the entries; and the same reads unplanted"""
    control = random_bases(seed, L * n_reads)
    seq = control.copy()
    spots = frl_key_spots(L, n_reads) if keys else [(r, o) for (r, o, _) in frl_spots(L, n_reads)]
    for i, (r, o) in enumerate(spots):
        plant(seq, r * L + o, entry_list[i % len(entry_list)]["bases"])
    return seq, control


def pos_batch(entry_list, n, seed, keys=False):
    control = random_bases(seed, n)
    seq = control.copy()
    spots = pos_key_spots(n) if keys else pos_spots(n)
    for i, (at, _) in enumerate(spots):
        plant(seq, at, entry_list[i % len(entry_list)]["bases"])
    return seq, control


# ----------------------------------------------------------------------------- closed syncmers

CK, CS = 31, 11
CL_STRIDE, CL_WAVE = 3968, 992


def closed_spots(n):
    ws = lambda t, v: CL_STRIDE * t + CL_WAVE * v
    return [
        (0, "first k-mer of the sequence"),
        (ws(0, 1) + 16 * 5, "k-mer at a lane's first position"),
        (ws(0, 2) + 16 * 9 + 10, "s-mers across two lane borders"),
        (ws(0, 3) + 975, "last s-mer at + 995: lane 62 of the tile's last wave, which owns no k-mer"),
        (ws(1, 1) + 991, "last k-mer a wave owns: its s-mers reach into lanes 62 and 63"),
        (n - CK, "last k-mer, in the last, partial tile"),
    ]


def closed_batch(entry, n, seed):
    control = random_bases(seed, n)
    seq = control.copy()
    for at, _ in closed_spots(n):
        plant(seq, at, entry["bases"])
    return seq, control


def closed_quiet(seq, seed):
    """the condition on a control batch: on either strand no k-mer's end dword comes within 2 of its inner minimum, and no dword is below 2"""
    s = bytes(seq).decode()
    u = T.units(s, CS, False)
    for x in (T.top_plus_one(u, seed).astype(np.int64), T.top_plus_one(T.revcomp_value(u, CS), seed).astype(np.int64)):
        w = np.lib.stride_tricks.sliding_window_view(x, CK - CS + 1)
        e, mid = np.minimum(w[:, 0], w[:, -1]), w[:, 1:-1].min(axis=1)
        if (np.abs(e - mid) < 2).any() or x.min() < 2:
            return False
    return True
