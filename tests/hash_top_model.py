"""A plain numpy model of the approximate hash dword pass 1 of the window scans decides on, written from the rule and not from
the kernel text, and (at the end) of what the exact kernels' own fast forms keep of a hash.  TEST INFRASTRUCTURE: imported by tests/ and by
tests/golden/make_approx_adversaries.py and make_tie_adversaries.py only.

The rule.  hash64(key, seed) = F1 + F2 (mod 2^64), the two finalised halves of MurmurHash3_x64_128 over the 8 key bytes.  Write
F = hi:lo in dwords.  Then

    T     = hash64 >> 32              = hi1 + hi2 + carry  (mod 2^32),   carry = (lo1 + lo2) >> 32   in {0, 1}
    S     = top(key, seed)            = hi1 + hi2          (mod 2^32)    -- what pass 1 compares (T or one BELOW it)
    S + 1 = top_plus_one(key, seed)                        (mod 2^32)    -- the other form (T or one ABOVE it)

Window keys are packed: prefix = dword >> 6 (26 bits) above a 6-bit position tag.  What follows from the rule, for two keys a, b
without a wrap (the same for both forms):

  * prefixes two or more apart: the hashes are ordered like the prefixes;
  * prefixes exactly one apart, prefix(a) + 1 == prefix(b): T(a) <= T(b) still, and T(a) == T(b) only for S(b) == S(a) + 1 with
    carry(a) = 1, carry(b) = 0 -- the low dwords of the hashes then decide, either way.  That is the ONE case in the band of
    width one where the approximate order can be wrong (`misordered`), a coincidence of 2^-32 per pair;
  * equal prefixes: anything goes.

A wrap: top:          S == 0xffffffff with carry 1 -- approximate prefix all ones, T == 0, the smallest hash there is;
        top_plus_one: S == 0xffffffff with carry 0 -- approximate value 0, T == 0xffffffff, the largest.
"""
import numpy as np

M = np.uint64
MASK32 = M(0xFFFFFFFF)
NEAR = 0xFFFFFFC0  # values from here on have every prefix bit set


def halves(keys, seed):
    """F1, F2: fmix64 of the two lanes of MurmurHash3_x64_128 for one 8-byte little-endian key and a 32-bit seed"""
    with np.errstate(over="ignore"):
        k = np.atleast_1d(np.asarray(keys, dtype=np.uint64)).copy()
        s = M(int(seed) & 0xFFFFFFFF)
        k = k * M(0x87C37B91114253D5)
        k = (k << M(31)) | (k >> M(33))
        k = k * M(0x4CF5AD432745937F)
        h1 = (s ^ k) ^ M(8)           # h1 ^= k1; h1 ^= len
        h2 = np.full_like(k, s ^ M(8))
        h1 = h1 + h2
        h2 = h2 + h1

        def fmix(x):
            x = x ^ (x >> M(33))
            x = x * M(0xFF51AFD7ED558CCD)
            x = x ^ (x >> M(33))
            x = x * M(0xC4CEB9FE1A85EC53)
            return x ^ (x >> M(33))

        return fmix(h1), fmix(h2)


def hash64(keys, seed):
    f1, f2 = halves(keys, seed)
    with np.errstate(over="ignore"):
        return f1 + f2


def top(keys, seed):
    """S: the sum of the two high dwords, without the carry of the low ones"""
    f1, f2 = halves(keys, seed)
    return ((f1 >> M(32)) + (f2 >> M(32))) & MASK32


def top_plus_one(keys, seed):
    return (top(keys, seed) + M(1)) & MASK32


def carry(keys, seed):
    f1, f2 = halves(keys, seed)
    return ((f1 & MASK32) + (f2 & MASK32)) >> M(32)


def true_top(keys, seed):
    """T, from the rule (S + carry); tests pin it against hash64 >> 32"""
    return (top(keys, seed) + carry(keys, seed)) & MASK32


def approx(keys, seed, form):
    """the dword a kernel family compares: form = 'top' or 'top_plus_one'"""
    if form == "top":
        return top(keys, seed)
    if form == "top_plus_one":
        return top_plus_one(keys, seed)
    raise ValueError(form)


def prefix(dword):
    return np.asarray(dword, dtype=np.uint64) >> M(6)


def wraps(keys, seed, form):
    """S + carry crosses 2^32 (top), or S + 1 == 0 with carry 0 (top_plus_one): the approximate dword is at the wrong END of the range"""
    s, c = top(keys, seed), carry(keys, seed)
    if form == "top":
        return (s == MASK32) & (c == M(1))
    return (s == MASK32) & (c == M(0))


def near_wrap(keys, seed, form):
    """the key is one a wrap guard must fire for although it did not wrap: every prefix bit set (top), prefix 0 (top_plus_one)"""
    a = approx(keys, seed, form)
    hit = (a >= M(NEAR)) if form == "top" else (a < M(64))
    return hit & ~wraps(keys, seed, form)


# ----------------------------------------------------------------------------- sequences and units

_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def codes(seq):
    if isinstance(seq, str):
        seq = seq.encode()
    c = _CODE[np.frombuffer(bytes(seq), np.uint8)]
    assert (c < 4).all(), "ACGT only"
    return c


def decode(values, length):
    """2-bit packed value(s), first base most significant -> str (scalar) """
    v = int(values)
    return "".join("ACGT"[(v >> (2 * (length - 1 - i))) & 3] for i in range(length))


def revcomp_value(v, length):
    v = np.asarray(v, dtype=np.uint64)
    out = np.zeros_like(v)
    x = v.copy()
    for _ in range(length):
        out = (out << M(2)) | (M(3) - (x & M(3)))
        x = x >> M(2)
    return out


def units(seq, unit, canonical):
    """the unit values of one sequence, in position order (first base most significant; canonical: the numeric minimum of both strands)"""
    c = codes(seq).astype(np.uint64)
    n = len(c) - unit + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    fw = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    for i in range(unit):
        fw = (fw << M(2)) | c[i:i + n]
        rc = rc | ((M(3) - c[i:i + n]) << M(2 * i))
    return np.minimum(fw, rc) if canonical else fw


# ----------------------------------------------------------------------------- windows

def _windows(x, w):
    return np.lib.stride_tricks.sliding_window_view(np.asarray(x), w)


def argmin_hash(h, w):
    """per window of w consecutive units: index of the smallest hash, leftmost of equals (the rule of every scan that packs approximate
    dwords into window keys; the closed-syncmer kernels, which mirror it on the reverse strand, compare values: closed_facts)"""
    return _windows(h, w).argmin(axis=1)


def argmin_prefix(a, w):
    """the same on the 26-bit prefixes of the approximate dwords: what a packed key (prefix above a position tag) elects"""
    return argmin_hash(prefix(a), w)


def two_smallest_prefixes(a, w):
    win = np.sort(_windows(prefix(a), w), axis=1)
    return win[:, 0], win[:, 1]


def equal_prefix(a, w):
    lo, nx = two_smallest_prefixes(a, w)
    return lo == nx


def one_apart(a, w):
    lo, nx = two_smallest_prefixes(a, w)
    return nx - lo == M(1)


def misordered(a, h, w):
    return argmin_prefix(a, w) != argmin_hash(h, w)


def must_redo(keys, seed, form, w):
    """per window: the rule cannot vouch for the prefix argmin -- the two smallest prefixes are less than two apart, or the window holds
    a key a wrap guard has to fire for (wrapped or not).  Windows of a sequence's units `keys`."""
    a = approx(keys, seed, form)
    lo, nx = two_smallest_prefixes(a, w)
    guard = near_wrap(keys, seed, form) | wraps(keys, seed, form)
    return (nx - lo < M(2)) | _windows(guard, w).any(axis=1)


# ----------------------------------------------------------------------------- closed syncmers (offsets {0, w - 1})

def revcomp_str(seq):
    return seq[::-1].translate(str.maketrans("ACGT", "TGCA"))


def closed_facts(kmer, s, seed):
    """One k-mer (a string) under the closed-syncmer rule: the s-mers of the CANONICAL k-mer (the numerically smaller strand), hashed as they
    stand; it is a syncmer when the leftmost smallest hash sits at the first or the last of them.  What a kernel sees on murmur64_top<true>:
    e = the smaller dword of the two end s-mers against mid = the smallest dword between them.
    Returns (true_hit, approx_hit, |e - mid|, smallest dword)."""
    rc = revcomp_str(kmer)
    c = kmer if units(kmer, len(kmer), False)[0] <= units(rc, len(rc), False)[0] else rc
    u = units(c, s, False)
    h = hash64(u, seed)
    a = top_plus_one(u, seed).astype(np.int64)
    am = int(h.argmin())
    e, mid = int(min(a[0], a[-1])), int(a[1:-1].min())
    return am in (0, len(u) - 1), e < mid, abs(e - mid), int(a.min())


def closed_syncmers(seq, k, s, seed, offsets):
    """positions of the k-mers of one ACGT sequence whose leftmost smallest s-mer hash, read along the canonical strand, sits at one of
    `offsets`: the syncmer rule for any seed (the oracle has the reference's seed 0 only; tests pin this against it there)"""
    w = k - s + 1
    u = units(seq, s, False)
    hf, hr = hash64(u, seed), hash64(revcomp_value(u, s), seed)
    kf = units(seq, k, False)
    rev = revcomp_value(kf, k) < kf
    off_f = _windows(hf, w).argmin(axis=1)
    off_r = _windows(hr, w)[:, ::-1].argmin(axis=1)  # the canonical strand reads the s-mers back to front
    off = np.where(rev, off_r, off_f)
    return np.flatnonzero(np.isin(off, list(offsets))).astype(np.uint64)


# ----------------------------------------------------------------------------- the exact kernels' own fast path (tie adversaries)

def syncmer_offsets(seq, k, s, seed, canonical):
    """per k-mer of one ACGT sequence: the offset, along the strand that counts, of its smallest s-mer hash (s-mers hashed as they stand on that
    strand; leftmost of equals along it) and whether that strand is the reverse one"""
    w = k - s + 1
    u = units(seq, s, False)
    hf = hash64(u, seed)
    off = _windows(hf, w).argmin(axis=1)
    kf = units(seq, k, False)
    rev = np.zeros(len(kf), bool)
    if canonical:
        hr = hash64(revcomp_value(u, s), seed)
        rev = revcomp_value(kf, k) < kf
        off = np.where(rev, _windows(hr, w)[:, ::-1].argmin(axis=1), off)
    return off, rev


def _argmin_last(x, w):
    return (w - 1) - _windows(x, w)[:, ::-1].argmin(axis=1)


def fast_argmins(h, w):
    """per window of w consecutive hashes, what each fast form ALONE would elect, beside the truth:
         p26_left / p26_right   26-bit prefix above a 6-bit tag (window_argmin_packed), leftmost / rightmost of equal prefixes
         p25_left / p25_right   25-bit prefix above a 7-bit tag (the run-time widths)
         hi32_left / hi32_right the high dword alone, ties to one side
         true_left / true_right the 64-bit hashes (the two differ only where equal units repeat)"""
    h = np.asarray(h, dtype=np.uint64)
    out = {}
    for name, x in (("p26", h >> M(38)), ("p25", h >> M(39)), ("hi32", h >> M(32)), ("true", h)):
        out[name + "_left"] = _windows(x, w).argmin(axis=1)
        out[name + "_right"] = _argmin_last(x, w)
    return out


def tie_class(ha, hb):
    """how two different hashes tie in the fast forms: 'hi32', 'p26', 'p25' or None"""
    ha, hb = int(ha), int(hb)
    if ha == hb:
        return None
    if ha >> 32 == hb >> 32:
        return "hi32"
    if ha >> 38 == hb >> 38:
        return "p26"
    if ha >> 39 == hb >> 39:
        return "p25"
    return None
