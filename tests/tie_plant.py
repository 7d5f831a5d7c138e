"""Batches that plant the entries of tests/golden/tie_adversaries.json (two different keys that tie in what a fast window form keeps) where the lane
maps of the pass-1 kernels make them hard, and what tests/hash_top_model.py says about those batches.  TEST INFRASTRUCTURE shared by
test_tie_adversaries.py (CPU emulation) and test_gpu_tie_adversaries.py.

A window entry with teeth has its guard base planted in front of it: the unit that starts there is smaller than the entry's first unit, which
therefore no window elects; a scan that elects it in the planted window reports one record more than the exact scan.  (Without the guard the
window before would elect that unit anyway, and a wrong decision in the planted window would change no record.)

One batch holds the entries of ONE shape (mode, unit, w, canonical), about three tiles of random filler around them:
  dense    every entry 16 times, the plant's start at every residue mod 16: every in-lane offset, every way of splitting the pair across a lane border
  borders  from the plan of that w (plan_pos / plan_frl below, Python transcriptions of plan_scan and plan_scan_frl_for that test_tie_adversaries.py
           pins against the emulation library's emu_plan): first window of the sequence, last window of the batch (in a partial tile), the pair
           split across lanes 62 | 63 of a wave, across a wave border, across a tile border, a window decided by the last owner of a wave and of
           a tile; read-tiled: first and last window of a read, the pair across the border of a read's last two lanes in a wave's last read,
           a lane border in an inner tile, the last, partial tile.
The filler is drawn again (seed, seed + 1, ...) until the model says that every planted window has exactly the planted pair as its two minima and
that no other window of the batch, and no window of the unplanted control, has its two smallest hashes equal in their top 25 bits.

Geometry (bl_scan_core.hpp).  Position-tiled: a wave owns own = 1024 - 16 * ceil(w / 16) positions, a tile 4 * own; wave v of tile t starts at
origin + 4 * own * t + own * v, origin = -16 for the window scans (the owner of position x decides the window that starts at x + 1) and 0 for
syncmers; lane l holds positions + 16 l .. + 15, the lanes past `own` are halo only.  Read-tiled: a read's nu units lie ns per lane on lpr lanes,
a wave takes rpw reads, a tile 4 * rpw.

The emulation builds a lane's halo from its neighbours' state, the device by DPP hops (and by LDS in the exact forms): the placements at lanes
62 | 63 and at wave borders meet the device's own halo only in test_gpu_tie_adversaries.py.
"""
import functools
import json
import os

import numpy as np

import hash_top_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
M = np.uint64
MODE_MINIMIZER, MODE_SUPERKMER, MODE_SYNCMER = 0, 1, 2
S, NWAVE, NCHUNK = 16, 4, 512


@functools.lru_cache(None)
def corpus():
    with open(os.path.join(HERE, "golden", "tie_adversaries.json")) as f:
        return json.load(f)["entries"]


def shape_entries(mode, unit, w, canonical, classes=None, pair=None):
    return [e for e in corpus() if (e["mode"], e["unit"], e["w"], e["canonical"]) == (mode, unit, w, canonical)
            and (classes is None or e["class"] in classes) and (pair is None or tuple(e["pair"]) == tuple(pair))]


def pair_of(e):
    return tuple(e["pair"]) if e["mode"] == "syncmer" else (0, e["w"] - 1)


def true_offset(e):
    """offset (along the strand that counts) of the entry's smallest hash"""
    a, b = pair_of(e)
    if e["mode"] == "window" or e["strand"] == "forward":
        return a if e["winner"] == "left" else b
    return a if e["winner"] == "right" else b


def has_teeth(e):
    """the fast forms elect the lower offset of a tied pair (leftmost; on the reverse strand rightmost in sequence order, the lower offset along it)"""
    return true_offset(e) != pair_of(e)[0]


# ----------------------------------------------------------------------------- the plans

def plan_pos(mode, first, end, w):
    own = 64 * S - 16 * ((w + 15) // 16)
    stride = NWAVE * own
    x = first if mode == MODE_SYNCMER else first - 1
    origin = (x // 16) * 16
    return dict(frl=0, origin=origin, stride=stride, own=own, n_tiles=(end - 1 - origin) // stride + 1 if end > first else 0)


def _plan_frl(n_bases, L, unit, w, ns_fixed):
    if L <= 0 or L > 4096 or n_bases % L or n_bases <= 0:
        return None
    nu = L - unit + 1
    nwin = nu - w + 1
    if nwin < 1 or w < 2:
        return None
    lpr = (nu + S - 1) // S
    if lpr > 64:
        return None
    ns = ns_fixed or (nu + lpr - 1) // lpr
    if ns * lpr < nu or ns > S or w - 1 > 3 * ns:
        return None
    rpw = min(64 // lpr, (NCHUNK * 16 - 64 - 32) // NWAVE // L)
    if rpw < 1:
        return None
    frl_eff = (rpw * nwin) / (64.0 * ns)
    pos_eff = nwin / L * (64 * S - 16 * ((w + 15) // 16)) / (64.0 * S)
    if frl_eff <= pos_eff:
        return None
    n_reads = n_bases // L
    return dict(frl=1, origin=0, stride=NWAVE * rpw * L, n_tiles=(n_reads + NWAVE * rpw - 1) // (NWAVE * rpw), read_len=L, lpr=lpr, rpw=rpw, ns=ns, nwin=nwin,
                nu=nu, reads_per_tile=NWAVE * rpw)


def frl_width_built(mode, w):
    return (mode == MODE_MINIMIZER and w in (11, 5, 10, 19)) or (mode == MODE_SUPERKMER and w == 17)


def plan_frl(mode, n_bases, L, unit, w, canonical):
    """the read-tiled plan of a whole batch of n_bases / L reads, None where the scan stays position-tiled"""
    if not frl_width_built(mode, w):
        return None
    if mode == MODE_MINIMIZER and w == 11 and unit == 31 and canonical:
        g = _plan_frl(n_bases, L, unit, w, 0)
        if g and 14 <= g["ns"] <= 16:
            return g
    return _plan_frl(n_bases, L, unit, w, S)


# ----------------------------------------------------------------------------- batches

def random_bases(seed, n):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].copy()


def _put(seq, at, bases):
    b = np.frombuffer(bases.encode(), np.uint8)
    seq[at:at + len(b)] = b


def pos_spots(mode, w, span, n, pair):
    """(start of the planted string, why) for one sequence of n bases, position-tiled"""
    g = plan_pos(mode, 0, n, w)
    own, a = g["own"], pair[0]
    ws = lambda t, v: g["origin"] + g["stride"] * t + own * v
    split = lambda x: x - 1 - a  # the pair's first key at position x - 1, its second at or after x
    lead = 0 if mode == MODE_SYNCMER else 1  # the window that starts at x + lead is decided by the owner of x
    assert g["n_tiles"] == 4 and n - (g["origin"] + 3 * g["stride"]) < g["stride"]
    return [
        (0, "first window of the sequence"),
        (split(ws(0, 1) + 16 * 63), "the pair split across lanes 62 | 63"),
        (split(ws(0, 2)), "the pair split across a wave border"),
        (ws(0, 3) - 1 + lead, "decided by the last owner of a wave, every key in the next wave's lanes too"),
        (split(ws(1, 0)), "the pair split across a tile border"),
        (ws(2, 0) - 1 + lead, "decided by the last owner of a tile"),
        (split(ws(2, 2) + 16 * 63), "the pair split across lanes 62 | 63, another tile"),
        (n - span, "last window of the batch, in the last, partial tile"),
    ]


def pos_length(w):
    return 3 * NWAVE * (64 * S - 16 * ((w + 15) // 16)) + 1391


def _layout(entries, unit, span, n, spots):
    """[(start, entry)]: the border spots cycling through the entries, then every entry at 16 starts that cover the residues mod 16"""
    plants, taken = [], []
    for i, (at, _) in enumerate(spots):
        if any(at < hi and lo < at + span + unit for lo, hi in taken):
            continue  # (two borders that coincide for this w)
        plants.append((at, entries[i % len(entries)]))
        taken.append((at - unit, at + span + unit))
    taken.sort()
    cursor = unit + span + 7
    for e in entries:
        for r in range(16):
            at = cursor + (r - cursor) % 16
            while True:
                hit = [hi for lo, hi in taken if at < hi and lo < at + span + unit]
                if not hit:
                    break
                at = max(hit) + (r - max(hit)) % 16
            plants.append((at, e))
            cursor = at + span + unit + 4
    assert cursor + span + unit < n, "the dense plants do not fit"
    return sorted(plants, key=lambda x: x[0])


def _quiet(h, w, skip=()):
    """no window of w consecutive hashes has its two smallest equal in their top 25 bits, the windows at `skip` aside"""
    part = np.partition(np.lib.stride_tricks.sliding_window_view(h >> M(39), w), 1, axis=1)
    tie = part[:, 0] == part[:, 1]
    tie[[x for x in skip if x < len(tie)]] = False
    return not tie.any()


def _both(plants, w):
    """the windows (k-mers) that hold both keys of a planted pair: the planted one, and for a pair that is not (0, w - 1) its neighbours"""
    out = []
    for at, e in plants:
        a, b = pair_of(e)
        if e["mode"] == "syncmer" and e["strand"] == "reverse":  # offsets along the reverse strand count from the k-mer's far end
            a, b = w - 1 - b, w - 1 - a
        out += [x for x in range(at + b - w + 1, at + a + 1) if x >= 0]
    return out


def _hashes(s, mode, unit, seed, canonical):
    """the hash arrays a window decision can be made on: the units' (window scans), the s-mers' on either strand (syncmers)"""
    if mode == "window":
        return [T.hash64(T.units(s, unit, bool(canonical)), seed)]
    u = T.units(s, unit, False)
    return [T.hash64(u, seed)] + ([T.hash64(T.revcomp_value(u, unit), seed)] if canonical else [])


def _planted_ok(s, plants, mode, unit, w, seed, canonical):
    """every planted window (k-mer) elects what its entry says, on the strand its entry says"""
    if mode == "window":
        h = T.hash64(T.units(s, unit, bool(canonical)), seed)
        am = T.argmin_hash(h, w)
        return all(int(am[at]) == true_offset(e) for at, e in plants)
    off, rev = T.syncmer_offsets(s, unit + w - 1, unit, seed, bool(canonical))
    return all(int(off[at]) == true_offset(e) and bool(rev[at]) == (e["strand"] == "reverse") for at, e in plants)


def _draw(n, seed, plants, mode, unit, w, hseed, canonical):
    """(seq, control, generator seed used): see the module docstring"""
    for k in range(64):
        control = random_bases(seed + k, n)
        seq = control.copy()
        for at, e in plants:
            _put(seq, at, e["bases"])
            if e.get("guard") and at > 0:  # the unit in front hashes below the entry's first: no other window elects that one (make_tie_adversaries.py)
                _put(seq, at - 1, e["guard"])
        s, c = bytes(seq).decode(), bytes(control).decode()
        if not all(_quiet(h, w) for h in _hashes(c, mode, unit, hseed, canonical)):
            continue
        if not _planted_ok(s, plants, mode, unit, w, hseed, canonical):
            continue
        if mode == "window":
            skip = _both(plants, w)
            if _quiet(_hashes(s, mode, unit, hseed, canonical)[0], w, skip):
                return seq, control, seed + k
        else:  # a planted k-mer ties on the strand that counts; its other strand, and every other k-mer, must be quiet
            hs = _hashes(s, mode, unit, hseed, canonical)
            fw = _both([(at, e) for at, e in plants if e["strand"] == "forward"], w)
            rv = _both([(at, e) for at, e in plants if e["strand"] == "reverse"], w)
            if _quiet(hs[0], w, fw) and (len(hs) == 1 or _quiet(hs[1], w, rv)):
                return seq, control, seed + k
    raise AssertionError("no quiet filler in 64 draws")


@functools.lru_cache(None)
def pos_batch(mode, unit, w, canonical, classes=None, pair=None, seed=5000):
    """one sequence, position-tiled: dict(seq, control, plants=[(start, entry)], offsets=a ragged cut of the same bases that keeps every plant whole)"""
    es = shape_entries(mode, unit, w, canonical, classes, pair)
    assert es, (mode, unit, w, canonical)
    span = unit + w - 1
    n = pos_length(w)
    md = MODE_SYNCMER if mode == "syncmer" else MODE_MINIMIZER
    spots = pos_spots(md, w, span, n, pair_of(es[0]))
    plants = _layout(es, unit, span, n, spots)
    seq, control, used = _draw(n, seed + 97 * w + unit, plants, mode, unit, w, es[0]["seed"], canonical)
    # ragged sequences: cut right before every fifth plant (it becomes the first window of a sequence) and right behind every fifth (the last)
    cuts = sorted({at for at, _ in plants[2::5]} | {at + span for at, _ in plants[4::5]})
    offsets = np.array([0] + [c for c in cuts if 0 < c < n] + [n], np.uint64)
    return dict(seq=seq, control=control, plants=plants, offsets=offsets, entries=es, span=span, seed=es[0]["seed"], filler_seed=used)


def frl_spots(g, w, n_reads):
    """(read, offset of the planted window inside the read, why)"""
    ns, rpt, rpw, nwin, nu = g["ns"], g["reads_per_tile"], g["rpw"], g["nwin"], g["nu"]
    last_lane = (nu - 1) // ns
    clamp = lambda o: max(0, min(o, nwin - 1))
    return [
        (0, 0, "first window of the first read"),
        (1, nwin - 1, "last window of a read"),
        (rpw - 1, clamp(last_lane * ns - 1), "a wave's last read: the pair across the border of its last two lanes"),
        (rpt + 2, clamp(ns - 1), "the pair across a lane border, second tile"),
        (rpt + rpw, 0, "first window of a wave's first read"),
        (2 * rpt + rpw - 1, nwin - 1, "last window of a wave's last read"),
        (3 * rpt - 1, clamp(ns + 1), "last read of a tile"),
        (n_reads - 1, nwin // 2, "last, partial tile"),
    ]


@functools.lru_cache(None)
def frl_batch(md, unit, w, canonical, L, classes=None, seed=7000):
    """three tiles of reads of L bases and a partial one: dict(seq, control, plants, plan)"""
    es = shape_entries("window", unit, w, canonical, classes)
    assert es, (unit, w, canonical)
    span = unit + w - 1
    g0 = plan_frl(md, L * 1000, L, unit, w, canonical)
    assert g0 is not None, "the read-tiled layout does not apply"
    n_reads = 3 * g0["reads_per_tile"] + 5
    g = plan_frl(md, L * n_reads, L, unit, w, canonical)
    used, plants = set(), []
    for i, (r, o, _) in enumerate(frl_spots(g, w, n_reads)):
        if r in used:
            continue
        used.add(r)
        plants.append((r * L + o, es[i % len(es)]))
    # dense: every entry at window offsets of every residue mod 16, as many plants to a read as fit with a clear gap between them
    step = span + unit + 16
    slots = max(1, (g["nwin"] - 16) // step + 1)
    r, t = 2, 0
    for e in es:
        for res in range(min(16, g["nwin"])):
            if t == slots:
                r, t = r + 1, 0
            while r in used:
                r += 1
            plants.append((r * L + t * step + (res - t * step) % 16, e))
            t += 1
        used.add(r)
        r, t = r + 1, 0
    assert r < n_reads, "the dense plants do not fit"
    plants.sort(key=lambda x: x[0])
    seq, control, fs = _draw(L * n_reads, seed + 97 * w + L, plants, "window", unit, w, es[0]["seed"], canonical)
    return dict(seq=seq, control=control, plants=plants, plan=g, entries=es, span=span, seed=es[0]["seed"], n_reads=n_reads, filler_seed=fs)


# ----------------------------------------------------------------------------- what a fast form alone would report

def dedupe(pos):
    pos = np.asarray(pos, np.int64)
    return pos[np.r_[True, pos[1:] != pos[:-1]]] if len(pos) else pos


def minimizer_positions(s, unit, w, seed, canonical, form):
    """positions of the minimizers of ONE sequence as `form` (a key of hash_top_model.fast_argmins) elects them"""
    h = T.hash64(T.units(s, unit, bool(canonical)), seed)
    am = T.fast_argmins(h, w)[form]
    return dedupe(np.arange(len(am)) + am)


def fast_form(w):
    """the fast form of the kernel a window scan of width w takes: 6-bit tags up to 32, 7-bit tags beyond"""
    return "p26_left" if w <= 32 else "p25_left"


def syncmer_positions(s, k, unit, seed, canonical, offsets, form="true"):
    """k-mers of ONE sequence whose elected s-mer offset (along the strand that counts) is one of `offsets`; form 'true', or the prefix a fast
    form keeps ('p26', 'p25', 'hi32') with ties to the lower offset along the strand"""
    w = k - unit + 1
    shift = {"true": 0, "p26": 38, "p25": 39, "hi32": 32}[form]
    u = T.units(s, unit, False)
    win = lambda x: np.lib.stride_tricks.sliding_window_view(x >> M(shift), w)
    off = win(T.hash64(u, seed)).argmin(axis=1)
    if canonical:
        kf = T.units(s, k, False)
        rev = T.revcomp_value(kf, k) < kf
        off = np.where(rev, win(T.hash64(T.revcomp_value(u, unit), seed))[:, ::-1].argmin(axis=1), off)
    return np.flatnonzero(np.isin(off, list(offsets))).astype(np.uint64)


def open_offsets(w):
    """two pairs of open offsets, each naming one end and the middle: a planted pair (0, w - 1) has exactly one key in either"""
    return [(0, w // 2), (w // 2, w - 1)]


# ----------------------------------------------------------------------------- the cases of both test modules

WINDOW_SHAPES = sorted({(e["unit"], e["w"], e["canonical"]) for e in corpus() if e["mode"] == "window"}, key=lambda x: (x[1], x[0], x[2]))
OPEN_SHAPES = sorted({(e["unit"], e["w"], e["canonical"]) for e in corpus() if e["mode"] == "syncmer" and tuple(e["pair"]) == (0, e["w"] - 1)})
CLOSED_SHAPES = sorted({(e["unit"], e["w"], e["canonical"], tuple(e["pair"])) for e in corpus() if e["mode"] == "syncmer" and tuple(e["pair"]) != (0, e["w"] - 1)})
SYNC_CASES = [(s, w, c, (0, w - 1), "open") for s, w, c in OPEN_SHAPES] + [(s, w, c, pr, "closed") for s, w, c, pr in CLOSED_SHAPES]
# (mode, unit, w, canonical, read length): the general kernels (a unit other than 31), the exact ns = 14 / 15 / 16 kernels' shape, and for it one
# length (79) where the planner falls back to the general 16-units-per-lane layout (served by that shape's ns = 16 kernel)
FRL_CASES = [(MODE_MINIMIZER, u, w, c, L) for (u, w, c) in [(21, 5, 1), (25, 10, 0), (23, 11, 1), (21, 19, 1)] for L in (100, 150)] \
    + [(MODE_MINIMIZER, 31, 11, 1, L) for L in (100, 150, 286, 79)] + [(MODE_SUPERKMER, 25, 17, 1, L) for L in (100, 150)]


def ids(x):
    return "-".join(str(v) for v in x) if isinstance(x, tuple) else str(x)
