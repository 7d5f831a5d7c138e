"""Independent model of the 128-bit k-mer scans (bl_scan_kmers128 / bl_scan_hash_sample128), in Python integers.

TEST INFRASTRUCTURE: shares no code with the library.  Semantics:
  value      bases packed 2 bits each (A 0, C 1, G 2, T/U 3, either case), first base in the most significant occupied pair, 1 <= k <= 64
  canonical  min(forward, reverse complement) as integers, the reverse complement taken in 2k bits
  hash       first word of MurmurHash3_x64_128 over the 16 little-endian bytes of the value, 32-bit seed (closed form for len = 16)
  valid      a k-mer starts at p: k good bases inside one sequence; drop_last removes the k-mer that ends its sequence
"""
import numpy as np

M64 = (1 << 64) - 1
CODE = {c: i for i, c in enumerate(b"ACGT")}
CODE.update({c: i for i, c in enumerate(b"acgt")})
CODE[ord("U")] = CODE[ord("u")] = 3


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k


def hash_u128(lo, hi, seed):
    c1, c2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
    h1 = h2 = seed & 0xFFFFFFFF
    k1 = (_rotl((lo * c1) & M64, 31) * c2) & M64
    h1 ^= k1
    h1 = (_rotl(h1, 27) + h2) & M64
    h1 = (h1 * 5 + 0x52DCE729) & M64
    k2 = (_rotl((hi * c2) & M64, 33) * c1) & M64
    h2 ^= k2
    h2 = (_rotl(h2, 31) + h1) & M64
    h2 = (h2 * 5 + 0x38495AB5) & M64
    h1 ^= 16
    h2 ^= 16
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1, h2 = _fmix(h1), _fmix(h2)
    return (h1 + h2) & M64


def scan(seq, offsets, k, seed=0, canonical=False, drop_last=False):
    """Dense result over the whole batch: dict of numpy arrays lo, hi, hashes (uint64) and valid (uint8), 0 where no k-mer starts."""
    seq = bytes(seq)
    n = len(seq)
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)
    hs = np.zeros(n, np.uint64)
    ok = np.zeros(n, np.uint8)
    mask = (1 << (2 * k)) - 1
    top = 2 * (k - 1)
    for a, e in zip(offsets[:-1], offsets[1:]):
        a, e = int(a), int(e)
        fwd = rc = run = 0
        for i in range(a, e):
            c = CODE.get(seq[i])
            if c is None:
                run = 0
                continue
            fwd = ((fwd << 2) | c) & mask
            rc = (rc >> 2) | ((3 ^ c) << top)
            run += 1
            if run < k:
                continue
            if drop_last and i == e - 1:
                continue
            v = min(fwd, rc) if canonical else fwd
            p = i - k + 1
            lo[p] = v & M64
            hi[p] = v >> 64
            hs[p] = hash_u128(v & M64, v >> 64, seed)
            ok[p] = 1
    return dict(lo=lo, hi=hi, hashes=hs, valid=ok)


def digest(m, first=0, end=None):
    """the five digest words of bl_scan_kmers128 over positions [first, end)"""
    s = slice(first, end)
    xr = lambda a: int(np.bitwise_xor.reduce(a)) if len(a) else 0
    return dict(count=int(m["valid"][s].sum()), xor_value=xr(m["lo"][s]), aux=xr(m["hi"][s]), xor_hash=xr(m["hashes"][s]),
                sum_hash=int(m["hashes"][s].sum(dtype=np.uint64)) if len(m["hashes"][s]) else 0)


def sample(m, threshold, first=0, end=None, origin=0):
    """records of bl_scan_hash_sample128 over [first, end): dict of lo, hi, hashes, positions (numpy uint64) and the digest words"""
    end = len(m["valid"]) if end is None else end
    idx = np.nonzero((m["valid"][first:end] == 1) & (m["hashes"][first:end] < np.uint64(threshold)))[0] + first
    pos = (idx + origin).astype(np.uint64)
    xr = lambda a: int(np.bitwise_xor.reduce(a)) if len(a) else 0
    return dict(lo=m["lo"][idx], hi=m["hi"][idx], hashes=m["hashes"][idx], positions=pos, count=len(idx), xor_value=xr(m["lo"][idx]),
                aux=xr(m["hi"][idx]), xor_hash=xr(m["hashes"][idx]), xor_pos=xr(pos))
