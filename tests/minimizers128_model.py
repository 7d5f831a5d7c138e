"""Independent model of bl_scan_minimizers128 (sampler::minimizer_sampler over kmer_view<KmerType>), in numpy.

TEST INFRASTRUCTURE: shares no code with the library.  The rule (include/biolib_amd.h):
  units     the (canonical) k-mers of kmers128_model.scan, with their validity (drop_last removes the unit that ends its sequence)
  hash      MurmurHash3_x64_128 (first word) over the bytes of the unit AS A KmerType: `width` = 16 bytes for __uint128_t
            (kmers128_model.hash_u128), 8 for uint64_t (syncmers128_model.hash_keys; unit <= 32: what bl_scan_minimizers hashes)
  window    w consecutive unit start positions p .. p+w-1; it exists iff all w units are valid
  occurrence  the position of the smallest hash in the window, the leftmost of equal ones
  record    window p exists and (window p-1 does not exist or its occurrence is another position): value, position, hash of the
            occurrence's unit
How it is evaluated: brute force, sliding_window_view(...).argmin(axis=1) — numpy returns the first minimum.  window_by_hand() evaluates
one window in Python integers, word for word; the tests hold the two against each other.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import kmers128_model as K
import syncmers128_model as S

U = np.uint64


def scan(seq, offsets, unit, w, seed=0, canonical=False, drop_last=False, width=16):
    """dict over the whole batch: lo, hi, hashes, valid of the units; exist (bool), occ (int64, -1 where no window), tied (bool) of the
    windows by their first position"""
    assert 1 <= unit <= 64 and 1 <= w <= 64 and width in (8, 16)
    m = K.scan(bytes(seq), offsets, unit, seed, canonical, drop_last)
    hashes = m["hashes"]
    if width == 8:
        assert unit <= 32 and not m["hi"].any()
        hashes = S.hash_keys(m["lo"], seed, 8)
    n = len(hashes)
    valid = m["valid"].astype(bool)
    exist = np.zeros(n, bool)
    occ = np.full(n, -1, np.int64)
    tied = np.zeros(n, bool)
    nw = n - w + 1
    if nw > 0:
        rows = sliding_window_view(hashes, w)
        ex = sliding_window_view(valid, w).all(axis=1)
        exist[:nw] = ex
        occ[:nw] = np.where(ex, np.arange(nw) + rows.argmin(axis=1), -1)
        tied[:nw] = ex & ((rows == rows.min(axis=1)[:, None]).sum(axis=1) > 1)
    return dict(lo=m["lo"], hi=m["hi"], hashes=hashes, valid=m["valid"], exist=exist, occ=occ, tied=tied, w=w)


def window_by_hand(m, p, seed, canonical_values=None):
    """window p in Python integers: (exists, occurrence position); the hashes are recomputed from the unit values (16 key bytes)"""
    w, n = m["w"], len(m["valid"])
    if p + w > n or not all(int(m["valid"][q]) for q in range(p, p + w)):
        return False, -1
    best, arg = None, -1
    for q in range(p, p + w):
        h = K.hash_u128(int(m["lo"][q]), int(m["hi"][q]), seed)
        if best is None or h < best:  # strict: the leftmost minimum stays
            best, arg = h, q
    return True, arg


def minimizers(m, first=0, end=None, origin=0):
    """records of bl_scan_minimizers128 over the windows that start in [first, end): lo, hi, hashes, positions (numpy uint64), the
    windows' own positions (for the tests) and the digest words"""
    end = len(m["valid"]) if end is None else min(end, len(m["valid"]))
    exist, occ = m["exist"], m["occ"]
    rec = exist.copy()
    rec[1:] &= ~exist[:-1] | (occ[1:] != occ[:-1])
    win = np.nonzero(rec[first:end])[0] + first
    idx = occ[win]
    pos = (idx + origin).astype(U)
    xr = lambda a: int(np.bitwise_xor.reduce(a)) if len(a) else 0
    return dict(lo=m["lo"][idx], hi=m["hi"][idx], hashes=m["hashes"][idx], positions=pos, windows=win, count=len(idx), xor_value=xr(m["lo"][idx]),
                aux=xr(m["hi"][idx]), xor_hash=xr(m["hashes"][idx]), xor_pos=xr(pos), redone=0)
