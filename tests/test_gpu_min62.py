"""The canonical form of units of at most 31 bases is one v_min_f64 on the GPU (min62, bl_scan_core.hpp).  test_min62_host.py states
why that equals the integer minimum; this file checks what the hardware does with the patterns the statement is about, by scanning
reads built so that the forward unit, its reverse complement or both fall on each of them, and holding value, position and hash of
every record against the oracle (which takes the integer minimum):

  poly-A                        forward +0, reverse complement 2^62 - 1, the largest pattern; poly-T the other way round
  k-mers that begin with 5, 6   patterns below 2^52, 2^50, 2^30: subnormal readings; with T's at the other end the reverse complement
  and 16 A's                    is subnormal too
  X y rc(X)                     forward and reverse complement equal in the 15 bases before and the 15 after the centre base, which is
                                y on one strand and its complement on the other: equal high dwords, low dwords that differ in their
                                top pair only.  (The closest two strands of an ODD unit length come: a reverse-complement palindrome,
                                i.e. equal operands, needs an even length, and equal low dwords would need a centre base that is its
                                own complement.  Equal operands are test_min62_host.py's.)
  A15 C T15                     ... with both readings subnormal
  R rc(R), (AT)n, (CG)n, (ACGT)n   even-length reverse-complement palindromes: every 31-mer window and its reverse complement
                                share a prefix of up to 30 bases, so the operands differ first in the high dword, the low dword or
                                the last pair as the window slides
  A75 T75                       one strand sweeps from +0 up, the other from the largest pattern down

Shapes: 32 reads of 150 bp are one tile of the read-tiled kernels, 33 cross a tile edge (the 33rd read is a crafted one); each with
the packed copy, through the ASCII path and with exact_windows; the same at 151 bp; a 2,000-base sequence through the position-tiled
kernels; the dense k-mer scan and the super-k-mer scan on the same texts; and k = 32, which keeps the integer form."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 42
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def cores(rng):
    x15, x10 = rand(rng, 15), rand(rng, 10)
    r32 = rand(rng, 32)
    out = ["A" * 151, "T" * 151, "A" * 75 + "T" * 76, "T" * 70 + "A" * 81]
    for n in (5, 6, 16):
        out.append("C" + "A" * n + "C" + rand(rng, 40) + "G" + "A" * n + "G")  # forward subnormal
        out.append("G" + rand(rng, 40) + "G" + "T" * n + "G" + rand(rng, 33))  # reverse complement subnormal
        out.append("C" + "A" * n + rand(rng, max(31 - 2 * n, 0)) + "T" * n + "G")  # both (n = 16: A16 T16, 31-mers A16 T15 and A15 T16)
    for y in "ACGT":
        out.append("G" + x15 + y + rc(x15) + "C" + "AAAAA" + x10 + y + rc(x10) + "TTTTT" + "G")
    out.append("G" + "A" * 15 + "C" + "T" * 15 + "G" + "A" * 15 + "G" + "T" * 15 + "C")
    out += [r32 + rc(r32) + r32 + rc(r32), "AT" * 76, "CG" * 76, "ACGT" * 38, "AATT" * 38]
    return out


def reads_text(n_reads, L):
    """n_reads reads of L bases: the crafted cores (padded with random bases) first, random reads after them, and a crafted read last"""
    rng = np.random.default_rng(7)
    cs = cores(rng)
    assert len(cs) < 32
    reads = [(c + rand(rng, L))[:L] for c in cs]
    while len(reads) < n_reads - 1:
        reads.append(rand(rng, L))
    reads.append(("A" * 40 + "C" + "T" * 40 + rand(rng, L))[:L])
    assert len(reads) == n_reads
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()


def long_text():
    rng = np.random.default_rng(8)
    s = "".join((c + rand(rng, 96))[:96] for c in cores(rng))
    assert len(s) >= 2000
    return np.frombuffer(s[:2000].encode(), dtype=np.uint8).copy()


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.set_option("packed_codes", 1)
    c.set_exact_windows(False)
    c.close()


def test_the_texts_hold_the_patterns():
    for seq, offs in ((reads_text(33, 150), O.fixed_offsets(33 * 150, 150)), (long_text(), np.array([0, 2000], np.uint64))):
        fw, ok = O.units(seq, offs, 31, False)
        cn, _ = O.units(seq, offs, 31, True)
        fw, cn = fw[ok != 0], cn[ok != 0]
        other = np.where(cn == fw, 0, 1)  # 1: the reverse complement was taken
        assert (fw == 0).any() and (fw == (1 << 62) - 1).any(), "poly-A on either strand"
        assert other.any() and not other.all()
        for bits in (52, 50, 30):
            assert ((cn < (1 << bits)) & (other == 0)).any() and ((cn < (1 << bits)) & (other == 1)).any(), bits
        # both strands subnormal: A5 ... T5
        both = [i for i in np.flatnonzero(fw < (1 << 52)) if (int(fw[i]) & 0x3FF) == 0x3FF]
        assert both, "a 31-mer that begins with five A's and ends in five T's"
        # X y rc(X): the forward unit with its centre base complemented is the reverse complement
        centre = np.uint64(3 << 30)
        hits = [i for i in range(len(fw) - 1) if fw[i] != cn[i] and (fw[i] ^ centre) == cn[i]]
        assert hits, "strands that differ in the centre base only, reverse strand smaller"
        assert any(fw[i] == cn[i] and (fw[i] >> np.uint64(32)) == 0 and ((int(fw[i]) >> 30) & 3) == 1 for i in range(len(fw))), "A15 C T15"


def check_minimizers(ctx, batch, seq, offs, unit, w, what):
    got = batch.minimizers(unit, w, seed=SEED, canonical=True, capacity=len(seq) + 1)
    v, p, h = O.minimizers(seq, offs, unit, w, SEED, True, brute=False)
    assert got["count"] == len(v) and len(v) > 0, (what, got["count"], len(v))
    assert np.array_equal(got["values"], v), what
    assert np.array_equal(got["positions"], p), what
    assert np.array_equal(got["hashes"], h), what
    assert got["xor_value"] == O.xor_reduce(v) and got["xor_hash"] == O.xor_reduce(h) and got["xor_pos"] == O.xor_reduce(p), what


@pytest.mark.parametrize("variant", ["packed", "ascii", "exact"])
@pytest.mark.parametrize("L", [150, 151])
@pytest.mark.parametrize("n_reads", [32, 33])
def test_read_tiled(ctx, n_reads, L, variant):
    seq = reads_text(n_reads, L)
    batch = ctx.upload(seq, read_len=L)
    ctx.set_option("packed_codes", 0 if variant == "ascii" else 1)
    ctx.set_exact_windows(variant == "exact")
    try:
        check_minimizers(ctx, batch, seq, O.fixed_offsets(len(seq), L), 31, 11, (n_reads, L, variant))
    finally:
        ctx.set_option("packed_codes", 1)
        ctx.set_exact_windows(False)
        batch.close()


@pytest.mark.parametrize("variant", ["packed", "ascii", "exact"])
@pytest.mark.parametrize("k", [21, 31, 32])
def test_position_tiled(ctx, k, variant):
    """one sequence: the position-tiled kernels (k = 31, w = 11: rolling registers and min62; k = 21: the run-time unit length,
    k = 32: all 64 bits — both the integer form)"""
    seq = long_text()
    batch = ctx.upload(seq)
    ctx.set_option("packed_codes", 0 if variant == "ascii" else 1)
    ctx.set_exact_windows(variant == "exact")
    try:
        check_minimizers(ctx, batch, seq, np.array([0, len(seq)], np.uint64), k, 11, (k, variant))
    finally:
        ctx.set_option("packed_codes", 1)
        ctx.set_exact_windows(False)
        batch.close()


@pytest.mark.parametrize("k", [31, 32])
def test_dense_kmers(ctx, k):
    for seq, offs, kw in ((long_text(), np.array([0, 2000], np.uint64), {}), (reads_text(33, 150), O.fixed_offsets(33 * 150, 150), {"read_len": 150})):
        batch = ctx.upload(seq, **kw)
        val, ok = O.units(seq, offs, k, True)
        got = batch.kmers(k, seed=SEED, canonical=True)
        assert np.array_equal(got["valid"], ok) and ok.any(), k
        assert np.array_equal(got["values"], val), k
        assert np.array_equal(got["hashes"][ok != 0], O.hash64_np(val[ok != 0], SEED)), k
        d = O.kmer_digest(seq, offs, k, True, SEED)
        assert (got["count"], got["xor_value"], got["xor_hash"], got["sum_hash"]) == (d["count"], d["xor_value"], d["xor_hash"], d["sum_hash"]), k
        batch.close()


def test_super_kmers(ctx):
    for seq, offs, kw in ((long_text(), np.array([0, 2000], np.uint64), {}), (reads_text(33, 150), O.fixed_offsets(33 * 150, 150), {"read_len": 150})):
        batch = ctx.upload(seq, **kw)
        got = batch.super_kmers(31, 17, seed=SEED, canonical=True, capacity=len(seq) + 1)
        mn, fp, mp, sz, hs = O.super_kmers(seq, offs, 31, 17, SEED, True)
        assert got["count"] == len(mn) and len(mn) > 0
        for key, want in (("minimizers", mn), ("first_pos", fp), ("mm_pos", mp), ("sizes", sz), ("hashes", hs)):
            assert np.array_equal(got[key], want), key
        batch.close()
