"""Mines tests/golden/approx_adversaries.json: windows and keys on which the approximate hash dword of pass 1 (tests/hash_top_model.py)
is wrong, nearly wrong, or must trip a wrap guard.  Data only: base strings and 64-bit keys, each with its (unit, w, seed, canonical),
the dword form it is aimed at ('top': position-tiled scans, 'top_plus_one': read-tiled scans), the offset of the window and its class.

    python tests/golden/make_approx_adversaries.py          # rewrites the JSON beside this file

Deterministic: fixed generator seeds, fixed search order, single process; run twice it writes the same bytes.

Shape mined: canonical 31-mers, w = 11, seed 42 (the shape of every kernel that decides on murmur64_top in a default build).

  misordered_one_apart   the two smallest prefixes of a window are one apart and the hashes order the other way.  By the rule this needs
                         S(b) == S(a) + 1 across a prefix border with carries (1, 0) and the low dwords the right way round: about 2^-41
                         per pair.  The two 31-mers of a pair overlap, so: fix the 21 bases they share (first and last unit of one window
                         of 41 bases), hash all 4^10 left and all 4^10 right extensions, sort, and join on S + 1.  One entry per form and
                         per side the true winner is on.
  one_apart_same_order,  controls from random 150-bp reads: a second look is needed and changes nothing.
  equal_prefix
  near_wrap              a key whose dword has every prefix bit set ('top') or prefix 0 ('top_plus_one') without a wrap: random canonical keys.

  wrap, wrap_plus_one    canonical 31-mers with S == 0xffffffff exactly, carry 1 and carry 0 (2^-32 per key): approx_mine.c, compiled when this
                         script runs, over keys splitmix64(counter) >> 2 in fixed chunks of 2^27 counters on 16 threads, whole waves of 16
                         chunks at a time, the first hit in counter order.  Each key is entered for both forms.
  closed_*               the C5 closed-syncmer kernel (k = 31, s = 11): see mine_closed.  The pairs at seed 0, the reference's seed for s-mers,
                         from the full table of 4^11 keys; the wraps from every 11-mer under seeds 0, 1, 2, ... (none at seed 0: exhaustive).

Measured: the numpy part 495 s on one core (sequential so that its order is fixed): 125 shared middles (2 x 2^20 keys each) for the misordered
pairs, 28.6 M windows of random reads for the controls, 50 M random keys for the near-wrap keys.  The C part 55 s on 16 cores: 1.77e10 keys
(31-mers up to the wave that held both carries, 11-mers under seeds 0 .. 1151).
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hash_top_model as T  # noqa: E402

M = np.uint64
UNIT, W, SEED, CANON = 31, 11, 42, 1
FORMS = ("top", "top_plus_one")
STATS = {"middles": 0, "windows": 0, "keys": 0}


def _entry(cls, form, bases, keys, **extra):
    e = {"class": cls, "form": form, "unit": UNIT, "w": W, "seed": SEED, "canonical": CANON, "offset": 0, "bases": bases,
         "keys": ["0x%016x" % int(k) for k in keys]}
    e.update(extra)
    return e


def _window_facts(bases, form):
    u = T.units(bases, UNIT, CANON)
    a, h = T.approx(u, SEED, form), T.hash64(u, SEED)
    return u, a, h


def mine_misordered():
    """per form: one window whose true winner is its first unit, one whose true winner is its last"""
    rng = np.random.default_rng(20240611)
    want = {(f, side) for f in FORMS for side in ("left", "right")}
    found = {}
    ext = np.arange(1 << 20, dtype=np.uint64)  # all 10-base extensions
    while want:
        mid = int(rng.integers(0, 1 << 42))    # the 21 shared bases
        STATS["middles"] += 1
        left = (ext << M(42)) | M(mid)          # X + mid: the window's first unit
        right = (M(mid) << M(20)) | ext         # mid + Y: its last unit
        cl = np.minimum(left, T.revcomp_value(left, UNIT))
        cr = np.minimum(right, T.revcomp_value(right, UNIT))
        sl, sr = T.top(cl, SEED), T.top(cr, SEED)
        # pairs one dword apart, either way round: a = the smaller S (needs carry 1), b = a + 1 (needs carry 0)
        for (sa, ca, sb, cb, a_is_left) in ((sl, cl, sr, cr, True), (sr, cr, sl, cl, False)):
            order = np.argsort(sb, kind="stable")
            ssb = sb[order]
            at = np.searchsorted(ssb, sa + M(1))
            ok = (at < len(ssb))
            ok[ok] &= ssb[at[ok]] == sa[ok] + M(1)
            for ia in np.flatnonzero(ok):
                ib = int(order[at[ia]])
                ka, kb = ca[ia], cb[ib]
                if int(T.carry(ka, SEED)[0]) != 1 or int(T.carry(kb, SEED)[0]) != 0:
                    continue
                x, y = (int(ia), ib) if a_is_left else (ib, int(ia))
                bases = T.decode(x, 10) + T.decode(mid, 21) + T.decode(y, 10)
                for form in FORMS:
                    u, a, h = _window_facts(bases, form)
                    if not (T.one_apart(a, W)[0] and T.misordered(a, h, W)[0]):
                        continue
                    win = int(T.argmin_hash(h, W)[0])
                    if win not in (0, W - 1) or int(T.argmin_prefix(a, W)[0]) not in (0, W - 1):
                        continue
                    side = "left" if win == 0 else "right"
                    if (form, side) in want:
                        want.discard((form, side))
                        found[(form, side)] = _entry("misordered_one_apart", form, bases, (u[0], u[W - 1]), winner=side)
    return [found[(f, s)] for f in FORMS for s in ("left", "right")]


def mine_controls():
    """per form: windows of random reads whose two smallest prefixes are equal / one apart, the prefix argmin being the hash argmin"""
    rng = np.random.default_rng(20240612)
    want = {(f, c) for f in FORMS for c in ("equal_prefix", "one_apart_same_order")}
    found = {}
    while want:
        reads = rng.integers(0, 4, (20000, 150), dtype=np.uint8)
        STATS["windows"] += reads.shape[0] * (150 - UNIT - W + 2)
        for r in reads:
            s = "".join("ACGT"[c] for c in r)
            u = T.units(s, UNIT, CANON)
            h = T.hash64(u, SEED)
            for form in FORMS:
                a = T.approx(u, SEED, form)
                eq, oa, mis = T.equal_prefix(a, W), T.one_apart(a, W), T.misordered(a, h, W)
                for cls, hit in (("equal_prefix", eq & ~mis), ("one_apart_same_order", oa & ~mis)):
                    if (form, cls) in want and hit.any():
                        i = int(np.flatnonzero(hit)[0])
                        bases = s[i:i + UNIT + W - 1]
                        pa = np.argsort(T.prefix(a[i:i + W]), kind="stable")[:2]
                        want.discard((form, cls))
                        found[(form, cls)] = _entry(cls, form, bases, (u[i + int(pa[0])], u[i + int(pa[1])]))
            if not want:
                break
    return [found[(f, c)] for f in FORMS for c in ("equal_prefix", "one_apart_same_order")]


def mine_near_wrap():
    rng = np.random.default_rng(20240613)
    want = set(FORMS)
    found = {}
    while want:
        v = rng.integers(0, 1 << 62, 1 << 22, dtype=np.uint64)
        STATS["keys"] += len(v)
        k = np.minimum(v, T.revcomp_value(v, UNIT))
        for form in FORMS:
            if form in want:
                hit = np.flatnonzero(T.near_wrap(k, SEED, form))
                if len(hit):
                    want.discard(form)
                    key = k[hit[0]]
                    found[form] = _entry("near_wrap", form, T.decode(key, UNIT), (key,))
    return [found[f] for f in FORMS]


# ----------------------------------------------------------------------------- the searches in C (approx_mine.c)

THREADS = 16


def helper():
    """approx_mine.c beside this file, compiled into a temporary directory"""
    import ctypes as C
    import subprocess
    import tempfile

    d = tempfile.mkdtemp(prefix="approx_mine_")
    so = os.path.join(d, "approx_mine.so")
    subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "approx_mine.c")])
    L = C.CDLL(so)
    L.mine_wrap31.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.mine_wrap_small.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


def _waves(task, first=0):
    """task(i) for i = first, first + 1, ... on THREADS threads, a whole wave of THREADS at a time: what is returned depends on the wave, not on
    which thread finished first"""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(THREADS) as pool:
        i = first
        while True:
            yield list(pool.map(task, range(i, i + THREADS)))
            i += THREADS


def mine_wrap31(L):
    """canonical 31-mers with S == 0xffffffff at seed 42, one per carry: carry 1 is the wrap of `top` (dword all ones, T == 0, the smallest hash
    there is), carry 0 the wrap of `top_plus_one` (dword 0, T == 0xffffffff).  Each key goes into the corpus for both forms: in the other
    form it is a key at the guarded end of the range that did not wrap."""
    CHUNK = 1 << 27

    def task(i):
        out, at = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
        L.mine_wrap31(SEED, i * CHUNK, CHUNK, out.ctypes.data, at.ctypes.data)
        return out, at

    best = {}
    for wave in _waves(task):
        STATS["keys"] += THREADS * CHUNK
        for out, at in wave:
            for c in (0, 1):
                if at[c] != M(0xFFFFFFFFFFFFFFFF) and c not in best:
                    best[c] = out[c]
        if len(best) == 2:
            break
    entries = []
    for c, cls in ((1, "wrap"), (0, "wrap_plus_one")):
        key = best[c]
        assert int(T.top(key, SEED)[0]) == 0xFFFFFFFF and int(T.carry(key, SEED)[0]) == c and key <= T.revcomp_value(np.array([key]), UNIT)[0]
        for form in FORMS:
            entries.append(_entry(cls, form, T.decode(key, UNIT), (key,)))
    return entries


# closed syncmers (k = 31, s = 11, offsets {0, 20}: the C5 kernel compares murmur64_top<true> of 11-mers that are NOT canonical themselves)
CK, CS = 31, 11
CSEED = 0  # the reference hashes s-mers with seed 0; the wrap entries carry the seed they were found under


def _closed_entry(cls, seed, kmer, keys):
    return {"class": cls, "form": "top_plus_one", "unit": CS, "w": CK - CS + 1, "seed": int(seed), "canonical": CANON, "offset": 0, "bases": kmer,
            "keys": ["0x%016x" % int(k) for k in keys]}


def _closed_kmers(rng, e, m, seed, want, tries=400):
    """31-mers with 11-mer e at one end and 11-mer m right beside it, 9 random bases at the far end, that are their own canonical strand and
    for which want(true_hit, approx_hit, gap, low) holds; e at the first position, then e at the last"""
    for e_first in (True, False):
        for _ in range(tries):
            fill = T.decode(int(rng.integers(0, 1 << 18)), 9)
            kmer = T.decode(e, CS) + T.decode(m, CS) + fill if e_first else fill + T.decode(m, CS) + T.decode(e, CS)
            if T.units(kmer, CK, False)[0] > T.units(T.revcomp_str(kmer), CK, False)[0]:
                continue
            if want(*T.closed_facts(kmer, CS, seed)):
                yield kmer
                break


def mine_closed(L):
    """closed_misordered_hit   end s-mer e and inner minimum m with dwords ONE apart, e above m, equal true dwords and hash(e) < hash(m):
                             the approximate comparison says "no syncmer", the hashes say syncmer
       closed_misordered_miss  the other way round
       closed_one_apart_same   dwords one apart, same verdict either way (control)
       closed_wrap_plus_one    an 11-mer with S == 0xffffffff, carry 0, at the k-mer's end: dword 0 looks like the minimum, its hash is the
                             largest.  4^11 keys hold a wrap for one seed in a thousand: every 11-mer under seeds 0, 1, 2, ... until both
                             carries have turned up (exhaustive per seed; seed 0, the seed of the reference's syncmers, holds none, checked below)
       closed_wrap             the same with carry 1: dword 0, true dword 0 (the guard fires, nothing changes)"""
    rng = np.random.default_rng(20240614)
    keys = np.arange(1 << (2 * CS), dtype=np.uint64)
    s1, cy, h = T.top_plus_one(keys, CSEED).astype(np.int64), T.carry(keys, CSEED).astype(np.int64), T.hash64(keys, CSEED)
    assert not (T.top(keys, CSEED) == T.MASK32).any()  # no wrap among the 11-mers at seed 0
    STATS["keys"] += len(keys)
    order = np.argsort(s1, kind="stable")
    lo, hi = order[:-1], order[1:]
    adj = np.flatnonzero(s1[hi] - s1[lo] == 1)[:20000]  # ascending dwords: small ones are the likeliest minima of a k-mer
    entries, have = [], set()
    for i in adj:
        a, b = int(lo[i]), int(hi[i])  # dword(b) == dword(a) + 1
        flips = cy[a] == 1 and cy[b] == 0  # equal true dwords
        for cls, e, m, want in (
                ("closed_misordered_hit", b, a, lambda t, ap, gap, low: t and not ap and gap == 1 and low >= 2),
                ("closed_misordered_miss", a, b, lambda t, ap, gap, low: not t and ap and gap == 1 and low >= 2),
                ("closed_one_apart_same", a, b, lambda t, ap, gap, low: t == ap and gap == 1 and low >= 2)):
            if cls in have or (cls != "closed_one_apart_same" and not flips):
                continue
            if cls == "closed_misordered_hit" and not h[e] < h[m]:
                continue
            if cls == "closed_misordered_miss" and not h[m] < h[e]:
                continue
            for kmer in _closed_kmers(rng, e, m, CSEED, want):
                entries.append(_closed_entry(cls, CSEED, kmer, (e, m)))
                have.add(cls)
        if len(have) == 3:
            break
    assert len(have) == 3
    entries.sort(key=lambda x: (x["class"], x["bases"]))

    PER = 8  # seeds per task

    def task(i):
        so, ko = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
        L.mine_wrap_small(CS, i * PER, PER, so.ctypes.data, ko.ctypes.data)
        return so, ko

    best = {}
    for wave in _waves(task):
        STATS["keys"] += THREADS * PER * len(keys)
        for so, ko in wave:
            for c in (0, 1):
                if so[c] != M(0xFFFFFFFFFFFFFFFF) and c not in best:
                    best[c] = (int(so[c]), int(ko[c]))
        if len(best) == 2:
            break
    for c, cls, want in ((0, "closed_wrap_plus_one", lambda t, ap, gap, low: ap and not t and low == 0),
                         (1, "closed_wrap", lambda t, ap, gap, low: ap and t and low == 0)):
        seed, key = best[c]
        assert int(T.top(key, seed)[0]) == 0xFFFFFFFF and int(T.carry(key, seed)[0]) == c
        other = int(rng.integers(0, 1 << 22))
        got = list(_closed_kmers(rng, key, other, seed, want, tries=4000))
        assert got, cls
        entries += [_closed_entry(cls, seed, kmer, (key,)) for kmer in got]
    return entries


def mine_c(L=None):
    L = L or helper()
    return mine_wrap31(L) + mine_closed(L)


def main():
    t0 = time.time()
    entries = mine_misordered() + mine_controls() + mine_near_wrap() + mine_c()
    doc = {"shape": {"unit": UNIT, "w": W, "seed": SEED, "canonical": CANON}, "entries": entries}
    with open(os.path.join(HERE, "approx_adversaries.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d entries in %.0f s; searched %s" % (len(entries), time.time() - t0, STATS), file=sys.stderr)


if __name__ == "__main__":
    main()
