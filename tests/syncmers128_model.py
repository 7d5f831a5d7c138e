"""Independent model of bl_scan_syncmers128 (syncmer_sampler with minimizer_position_extractor over kmer_view<KmerType>), in numpy.

TEST INFRASTRUCTURE: shares no code with the library.  The rule (include/biolib_amd.h), for a valid k-mer of value v:
  s-mer j     x_j = (v >> 2(k-s-j)) & (4^s - 1), j = 0 .. W-1, W = k - s + 1: the s-mer that starts at the k-mer's base j
  hash        h_j = MurmurHash3_x64_128 (first word) over the bytes of x_j AS A KmerType: `width` = 16 bytes for __uint128_t (the high
              word is zero), 8 for uint64_t (what bl_scan_syncmers hashes); 32-bit seed
  offset      the smallest j of minimal h_j
  record      offset == start_offset or offset == end_offset
The k-mers, their validity and canonical form come from kmers128_model.scan.

How it is evaluated: the s-mers of a forward k-mer at p are the text's s-mers at p .. p+W-1; those of a k-mer whose canonical value is
its reverse complement are the reverse complements of the text's s-mers at p+W-1 .. p (x_j <-> text position p+W-1-j).  So every text
s-mer and its reverse complement are hashed ONCE and the windows are strided views.  extractor_offset() evaluates the rule on one value
in Python integers, word for word; the tests hold the two against each other.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import kmers128_model as K

U = np.uint64


def _rotl(x, r):
    return (x << U(r)) | (x >> U(64 - r))


def _fmix(k):
    k = k ^ (k >> U(33))
    k = k * U(0xFF51AFD7ED558CCD)
    k = k ^ (k >> U(33))
    k = k * U(0xC4CEB9FE1A85EC53)
    return k ^ (k >> U(33))


def hash_keys(x, seed, width):
    """first word of MurmurHash3_x64_128 over the `width` (8 or 16) little-endian bytes of the values x (< 2^64), numpy uint64 array"""
    assert width in (8, 16)
    x = np.asarray(x, dtype=U)
    c1, c2 = U(0x87C37B91114253D5), U(0x4CF5AD432745937F)
    sd = U(seed & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        k1 = _rotl(x * c1, 31) * c2
        h1 = np.full(x.shape, sd, U) ^ k1
        h2 = np.full(x.shape, sd, U)
        if width == 16:  # one body block: the s-mer and a zero high word (k2 = 0), no tail
            h1 = _rotl(h1, 27) + h2
            h1 = h1 * U(5) + U(0x52DCE729)
            h2 = _rotl(h2, 31) + h1
            h2 = h2 * U(5) + U(0x38495AB5)
        # width 8: no body block, the tail builds k1 from the 8 bytes
        h1 = h1 ^ U(width)
        h2 = h2 ^ U(width)
        h1 = h1 + h2
        h2 = h2 + h1
        return _fmix(h1) + _fmix(h2)


def extractor_offset(v, k, s, seed=0, width=16):
    """the rule on ONE k-mer value (Python int): (offset, number of j at which the minimum is attained)"""
    mask = (1 << (2 * s)) - 1
    hs = [int(hash_keys(np.array([(v >> (2 * (k - s - j))) & mask], U), seed, width)[0]) for j in range(k - s + 1)]
    return hs.index(min(hs)), hs.count(min(hs))


def scan(seq, offsets, k, s, seed=0, canonical=False, drop_last=False, width=16):
    """dict over the whole batch: valid (uint8), offset (int64: the extractor's offset, -1 where no k-mer starts), tied (bool: the minimum
    is attained more than once), strand (uint8: 1 = the canonical value is the reverse complement)"""
    assert 1 <= s <= 32 and s <= k <= 64
    seq = bytes(seq)
    n, w = len(seq), k - s + 1
    can = K.scan(seq, offsets, k, seed, canonical, drop_last)
    fwd = can if not canonical else K.scan(seq, offsets, k, seed, False, drop_last)
    valid = can["valid"].astype(bool)
    strand = valid & ((can["lo"] != fwd["lo"]) | (can["hi"] != fwd["hi"]))
    # text s-mers and their reverse complements: wherever s bases of any kind follow (a k-mer that is valid holds good bases only)
    code = np.array([K.CODE.get(c, 0) for c in seq], U)
    ns = max(n - s + 1, 0)
    f = np.zeros(ns, U)
    r = np.zeros(ns, U)
    for i in range(s):
        f = (f << U(2)) | code[i:i + ns]
        r = r | ((U(3) - code[i:i + ns]) << U(2 * i))
    hf, hr = hash_keys(f, seed, width), hash_keys(r, seed, width)
    offset = np.full(n, -1, np.int64)
    tied = np.zeros(n, bool)
    nk = max(n - k + 1, 0)
    if nk:
        wf = sliding_window_view(hf, w)[:nk]           # row p: h_j = hf[p + j]
        wr = sliding_window_view(hr, w)[:nk, ::-1]     # row p: h_j = hr[p + w-1 - j]
        rows = np.where(strand[:nk, None], wr, wf)
        off = rows.argmin(axis=1)                      # numpy returns the first (leftmost) minimum
        ties = (rows == rows.min(axis=1)[:, None]).sum(axis=1) > 1
        ok = valid[:nk]
        offset[:nk][ok] = off[ok]
        tied[:nk][ok] = ties[ok]
    return dict(valid=can["valid"], offset=offset, tied=tied, strand=strand.astype(np.uint8), lo=can["lo"], hi=can["hi"])


def syncmers(m, start_offset, end_offset, first=0, end=None, origin=0):
    """records of bl_scan_syncmers128 over [first, end): positions (numpy uint64), count and xor_pos"""
    end = len(m["valid"]) if end is None else end
    off = m["offset"][first:end]
    idx = np.nonzero((off >= 0) & ((off == start_offset) | (off == end_offset)))[0] + first
    pos = (idx + origin).astype(U)
    return dict(positions=pos, count=len(idx), xor_pos=int(np.bitwise_xor.reduce(pos)) if len(pos) else 0)
