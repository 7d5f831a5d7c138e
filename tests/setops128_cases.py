"""Inputs shared by the CPU emulation test and the GPU test of the 16-byte intersection kernels: pairs of sorted duplicate-free key
sets, as Python-int lists, built to put equal pairs across tile and thread boundaries of the merge kernel (tile T = 2048 merged
elements, 8 per thread).  TEST INFRASTRUCTURE: shares no code with the library."""
import numpy as np

T = 2048
M64 = (1 << 64) - 1
SIZES = [(0, 0), (0, 5), (5, 0), (1, 1), (T - 1, T + 1), (T, T), (3 * T + 17, 5 * T - 3)]


def _distinct(rng, n, kind):
    """n distinct keys, ascending"""
    out = set()
    while len(out) < n:
        need = n - len(out) + 8
        lo = rng.integers(0, 1 << 63, need, dtype=np.uint64).astype(object) * 2 + rng.integers(0, 2, need).astype(object)
        hi = rng.integers(0, 1 << 63, need, dtype=np.uint64).astype(object) * 2 + rng.integers(0, 2, need).astype(object)
        for x, y in zip(lo.tolist(), hi.tolist()):
            if kind == "high_only":     # keys that differ only in the high word
                out.add((y << 64) | 0x0123456789ABCDEF)
            elif kind == "low_only":    # keys that differ only in the low word
                out.add((0x8000000000000001 << 64) | x)
            elif kind == "top_bits" or (kind == "signs" and len(out) % 2):
                # low words >= 2^63 and high words >= 2^63; "signs" mixes them with ordinary keys: a signed compare of either word
                # puts them in front of the others
                out.add(((y | (1 << 63)) << 64) | (x | (1 << 63)))
            else:
                out.add((y << 64) | x)
            if len(out) == n:
                break
    return sorted(out)


def _split(rng, pool, na, nb, shared):
    """A and B of exactly na and nb keys from the na + nb - shared keys of pool, `shared` of them in both"""
    idx = rng.permutation(len(pool)).tolist()
    both = [pool[i] for i in idx[:shared]]
    a = both + [pool[i] for i in idx[shared:na]]
    b = both + [pool[i] for i in idx[na:]]
    assert len(a) == na and len(b) == nb
    return sorted(a), sorted(b)


def _interleave(pool, na, nb):
    """disjoint A and B taking the keys of pool in turn while both still need one"""
    a, b = [], []
    for key in pool:
        if len(a) < na and (len(a) <= len(b) or len(b) == nb):
            a.append(key)
        else:
            b.append(key)
    return a, b


def cases():
    """list of (name, A, B): sorted duplicate-free lists of Python ints < 2^128"""
    rng = np.random.default_rng(128128)
    out = []
    for n in (1, T, 3 * T + 17):
        pool = _distinct(rng, n + 1, "any")
        a = pool[1:]
        out.append((f"{n}-equal", a, list(a)))                              # A == B
        # one smaller key in front shifts the merged sequence by one: every even tile and thread diagonal falls BETWEEN an equal pair
        out.append((f"{n}-a-shifted", pool, a))                              # A == B u {one smaller key}
        out.append((f"{n}-b-shifted", a, pool))
    for na, nb in SIZES:
        tag = f"{na}x{nb}"
        if na and nb:
            shared = min(na, nb) // 2
            for kind in ("any", "high_only", "low_only", "top_bits", "signs"):
                a, b = _split(rng, _distinct(rng, na + nb - shared, kind), na, nb, shared)
                out.append((f"{tag}-{kind}", a, b))
            p = _distinct(rng, na + nb, "any")
            out.append((f"{tag}-interleaved", *_interleave(p, na, nb)))
            out.append((f"{tag}-a-below-b", p[:na], p[na:]))
            out.append((f"{tag}-b-below-a", p[nb:], p[:nb]))
            top = (1 << 128) - 1
            out.append((f"{tag}-last-common", p[:na - 1] + [top], p[na:na + nb - 1] + [top]))  # a common key as the very last element of both
        else:
            p = _distinct(rng, na + nb, "any")
            out.append((f"{tag}-empty", p[:na], p[na:]))
    for name, a, b in out:
        assert a == sorted(set(a)) and b == sorted(set(b)), name
    return out


def with_duplicates():
    """two inputs that break the contract (sorted, but with duplicates): run for memory safety only"""
    rng = np.random.default_rng(7)
    p = _distinct(rng, 3 * T, "any")
    a = sorted(p[: 2 * T] + p[:T] + [p[5]] * 40)
    b = sorted(p[T:] + p[T: 2 * T] + [p[-1]] * 9)
    return [("dup-both", a, b), ("dup-runs", [p[3]] * (T + 5) + [p[9]] * T, [p[3]] * (2 * T + 1) + [p[9]] * 3)]


def to_array(keys):
    """Python ints -> uint64[n, 2] (low, high)"""
    out = np.zeros((len(keys), 2), np.uint64)
    if keys:
        out[:, 0] = np.array([k & M64 for k in keys], dtype=np.uint64)
        out[:, 1] = np.array([k >> 64 for k in keys], dtype=np.uint64)
    return out
