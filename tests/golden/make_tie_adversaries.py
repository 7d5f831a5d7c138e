"""Mines tests/golden/tie_adversaries.json: windows and k-mers whose two smallest hashes are DIFFERENT keys that tie in what the fast form of an
exact window kernel keeps (tests/hash_top_model.py: fast_argmins), so that only the exact fallback can order them.  Data only: base strings,
64-bit keys, shape parameters, class and winner side.

    python tests/golden/make_tie_adversaries.py          # rewrites the JSON beside this file

Deterministic: counters in fixed chunks on 8 threads, whole waves of chunks at a time, the first hit in counter order; run twice it writes the
same bytes.  The search itself is tie_mine.c beside this file, compiled when this script runs; every hit is checked against the model here.

Classes (a, b = the two smallest hashes of the window):
  p26   a, b equal in bits 63..38, their high dwords differ      a tie of window_argmin_packed (26-bit prefix, 6-bit tag) and of everything coarser
  p25   equal in bits 63..39, bit 38 differs                      a tie of the 7-bit-tag kernels only (run-time widths)
  hi32  equal high dwords, different low dwords                   a tie of every fast form, the closed-syncmer kernels' whole-dword compare included
Every other unit of the window is larger in its top 25 bits already.  winner: the side (in sequence coordinates) the smaller hash is on.
guard (window entries whose winner is "right"): one base that, planted in front of the string, makes the unit that starts there hash below the
string's first unit, so that no window of a longer sequence elects that first unit: a scan that takes it for the string's own window then reports a
record the exact scan does not have (without the guard the window before would elect it anyway and the records would be the same).

mode "window": unit + w - 1 bases, the pair is the first and the last unit; serves minimizers (unit, w) and super-k-mers (m = unit, k = unit + w - 1).
   p26   every w in 2 .. 32 (units 19 .. 31, canonical for odd w; both for w = 2, 11, 32), w = 33, 48, 64, and canonical (31, 11), (15, 17)
   p25   w = 33, 48, 64
   hi32  w = 2, 16, 17, 32, 48 and canonical (31, 11), (15, 17)
mode "syncmer": one k-mer (k = unit + w - 1 <= 32 bases, s-mers of `unit` bases), seed 0 (the only seed the oracle has).  `pair`: the offsets of the
   two smallest s-mers along the strand that counts; `strand`: "forward" when the k-mer as it stands is that strand, "reverse" when its reverse
   complement is (canonical entries: mined on the counting strand with k-mer < reverse complement, and stored either way round).
   open    pair (0, w - 1), for offsets that name one end and an inner s-mer: (s, w) = (21, 11), (15, 17), (11, 21) on the templated widths, (11, 21)
           canonical on the kernel whose exact form is deferred, (24, 8) and (13, 19) on the run-time widths
   closed  hi32 only, pair (0, j) and (j, w - 1) with j inside: (19, 13) and (12, 20), canonical, both strands
   A run-time syncmer width above 32 does not exist: the scan takes k <= 32.

Measured: 59 s wall on 8 threads (6.5 CPU-minutes) for 158 entries, 1.96e9 counters tried.  A counter is one drawn middle (or gap) with its two
tables: 4 .. 65536 keys each side.  Nearly all of the time goes to the two hi32 searches at w = 2, where a counter holds 4 x 4 pairs and a
whole-dword tie takes 2^28 of them per winner; every other search is done in a second or two.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hash_top_model as T  # noqa: E402

THREADS = 8
LOG_TABLE = 16
CLS = {"p26": 0, "p25": 1, "hi32": 2}
STATS = {"counters": 0}
WSEED = 42  # window entries; syncmer entries: seed 0


def helper():
    d = tempfile.mkdtemp(prefix="tie_mine_")
    so = os.path.join(d, "tie_mine.so")
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "tie_mine.c")])
    L = C.CDLL(so)
    L.tie_mine.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.tie_mine.restype = None
    return L


def mine(L, pool, unit, w, seed, canon, cls, pi, pj, kcanon, guard=0):
    """(left, right): (base string, guard base or None) whose smaller hash of the pair is at pi / at pj"""
    span, d = unit + w - 1, pj - pi
    e = min(d, unit)
    chunk = max(4, (1 << 20) >> (2 * min(e, 9) - 2))

    def task(i):
        out, at = np.full(2 * span + 2, 255, np.uint8), np.zeros(2, np.uint64)
        L.tie_mine(unit, w, seed, canon, CLS[cls], pi, pj, kcanon, guard, LOG_TABLE, i * chunk, chunk, out.ctypes.data, at.ctypes.data)
        return out, at

    found, i = {}, 0
    while len(found) < 2:
        wave = list(pool.map(task, range(i, i + THREADS)))
        i += THREADS
        STATS["counters"] += THREADS * chunk
        for out, at in wave:
            for side in (0, 1):
                if side not in found and at[side] != np.uint64(0xFFFFFFFFFFFFFFFF):
                    g = int(out[2 * span + side])
                    found[side] = ("".join("ACGT"[c] for c in out[side * span:(side + 1) * span]), None if g == 255 else "ACGT"[g])
    return found[0], found[1]


def _keys(vals):
    return ["0x%016x" % int(v) for v in vals]


def window_entries(L, pool, unit, w, canon, cls):
    out = []
    for winner, (bases, guard) in zip(("left", "right"), mine(L, pool, unit, w, WSEED, canon, cls, 0, w - 1, 0, guard=1)):
        u = T.units(bases, unit, canon)
        h = T.hash64(u, WSEED)
        assert T.tie_class(h[0], h[-1]) == cls and (h[0] < h[-1]) == (winner == "left") and (guard is None) == (winner == "left")
        if guard:
            assert T.hash64(T.units(guard + bases[:unit - 1], unit, canon), WSEED)[0] >> np.uint64(39) < h[0] >> np.uint64(39)
        out.append({"mode": "window", "unit": unit, "w": w, "seed": WSEED, "canonical": canon, "class": cls, "winner": winner, "bases": bases,
                    "keys": _keys((u[0], u[-1])), "guard": guard})
    return out


def syncmer_entries(L, pool, s, w, canon, cls, pi, pj):
    out = []
    k = s + w - 1
    for side, (K, _) in zip((0, 1), mine(L, pool, s, w, 0, 0, cls, pi, pj, canon)):
        u = T.units(K, s, False)
        h = T.hash64(u, 0)
        assert T.tie_class(h[pi], h[pj]) == cls and (h[pi] < h[pj]) == (side == 0) and int(h.argmin()) == (pi, pj)[side]
        for strand in (("forward", "reverse") if canon else ("forward",)):
            bases = K if strand == "forward" else T.revcomp_str(K)
            winner = ("left", "right")[side] if strand == "forward" else ("right", "left")[side]
            off, rev = T.syncmer_offsets(bases, k, s, 0, bool(canon))
            assert int(off[0]) == (pi, pj)[side] and bool(rev[0]) == (strand == "reverse")
            out.append({"mode": "syncmer", "unit": s, "w": w, "seed": 0, "canonical": canon, "class": cls, "winner": winner, "bases": bases,
                        "keys": _keys((u[pi], u[pj])), "pair": [pi, pj], "strand": strand})
    return out


def unit_for(w):
    return 31 - 2 * (w % 7)


WINDOW_SHAPES = (
    [(unit_for(w), w, w % 2, "p26") for w in range(2, 33)]
    + [(unit_for(w), w, 1 - w % 2, "p26") for w in (2, 11, 32)]
    + [(21, 33, 0, c) for c in ("p26", "p25")] + [(25, 48, 1, c) for c in ("p26", "p25", "hi32")] + [(31, 64, 1, c) for c in ("p26", "p25")]
    + [(31, 11, 1, c) for c in ("p26", "hi32")] + [(15, 17, 1, c) for c in ("p26", "hi32")]
    + [(unit_for(w), w, w % 2, "hi32") for w in (2, 16, 17, 32)]
)
OPEN_SHAPES = (
    [(21, 11, 1, c) for c in ("p26", "hi32")] + [(15, 17, 0, c) for c in ("p26",)] + [(11, 21, 0, c) for c in ("p26",)]
    + [(11, 21, 1, c) for c in ("p26", "hi32")] + [(24, 8, 1, c) for c in ("p26", "p25", "hi32")] + [(13, 19, 1, c) for c in ("p26", "p25", "hi32")]
)
CLOSED_SHAPES = [(19, 13, 1, 0, 6), (19, 13, 1, 5, 12), (12, 20, 1, 0, 13), (12, 20, 1, 4, 19)]


def main():
    t0 = time.time()
    L = helper()
    entries = []
    with ThreadPoolExecutor(THREADS) as pool:
        for unit, w, canon, cls in WINDOW_SHAPES:
            entries += window_entries(L, pool, unit, w, canon, cls)
        for s, w, canon, cls in OPEN_SHAPES:
            entries += syncmer_entries(L, pool, s, w, canon, cls, 0, w - 1)
        for s, w, canon, pi, pj in CLOSED_SHAPES:
            entries += syncmer_entries(L, pool, s, w, canon, "hi32", pi, pj)
    with open(os.path.join(HERE, "tie_adversaries.json"), "w") as f:
        json.dump({"entries": entries}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d entries in %.0f s; searched %s" % (len(entries), time.time() - t0, STATS), file=sys.stderr)


if __name__ == "__main__":
    main()
