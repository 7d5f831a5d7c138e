"""A batch's packed copy (2-bit codes and one bad bit per 16-base chunk, made when the batch is) against the ASCII staging it replaces:
every case is scanned with the copy and again under set_option("packed_codes", 0), which makes the same batch go through the ASCII path,
and both results — every output array, the count, the digest words — are held against each other and against oracle_lib.

Shapes: the smallest that reach more than one tile of each layout (a read-tiled tile of 150-bp reads is 32 reads, a position-tiled
one 4032 positions), read lengths whose batch is and is not a multiple of 16, N's as the first and the last base of a chunk, in
the chunk on a tile border and in the last read, sub-ranges that start inside a chunk, one read, ten bases, and a borrowed buffer,
which never gets a copy."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 42


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.set_option("packed_codes", 1)
    c.close()


def random_bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()


def place_ns(seq, first, stride, read_len):
    """N as the first and as the last base of a chunk, in the chunk that holds the border between the first two tiles of the range that
    starts at `first`, and in the last read"""
    n = len(seq)
    for q in (first + 16 * 20, first + 16 * 40 + 15, (first + 700) | 15, (first + 900) & ~15, first + stride - 1, first + 2 * stride,
              n - 1 - read_len // 2, n - 1):
        if 0 <= q < n:
            seq[q] = ord("N")
    return seq


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), (what, key)
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


def both(ctx, scan, what):
    """the scan with the packed copy and through the ASCII path: equal in every word; returns the first"""
    ctx.set_option("packed_codes", 1)
    packed = scan()
    ctx.set_option("packed_codes", 0)
    try:
        ascii_ = scan()
    finally:
        ctx.set_option("packed_codes", 1)
    same(packed, ascii_, what)
    return packed


def check_minimizers(ctx, batch, seq, offsets, unit, w, what, first=0, n=0, canonical=True):
    """[first, first + n) must hold whole sequences of `offsets` (offsets relative to `first`)"""
    got = both(ctx, lambda: batch.minimizers(unit, w, seed=SEED, canonical=canonical, first=first, n=n, capacity=len(seq) + 1), what)
    part = seq[first:first + n] if n else seq[first:]
    v, p, h = O.minimizers(part, offsets, unit, w, SEED, canonical, brute=False)
    p = p + np.uint64(first)
    assert got["count"] == len(v), (what, got["count"], len(v))
    assert np.array_equal(got["values"], v) and np.array_equal(got["positions"], p) and np.array_equal(got["hashes"], h), what
    assert got["xor_value"] == O.xor_reduce(v) and got["xor_hash"] == O.xor_reduce(h) and got["xor_pos"] == O.xor_reduce(p), what


def check_super_kmers(ctx, batch, seq, offsets, k, m, what):
    got = both(ctx, lambda: batch.super_kmers(k, m, seed=SEED, canonical=True, capacity=len(seq) + 1), what)
    mn, fp, mp, sz, hs = O.super_kmers(seq, offsets, k, m, SEED, True)
    assert got["count"] == len(mn), (what, got["count"], len(mn))
    for key, want in (("minimizers", mn), ("first_pos", fp), ("mm_pos", mp), ("sizes", sz), ("hashes", hs)):
        assert np.array_equal(got[key], want), (what, key)
    # the digest words: minimizers, hashes, position of the minimizer (first k-mer + offset in it), number of group ends
    assert got["xor_value"] == O.xor_reduce(mn) and got["xor_hash"] == O.xor_reduce(hs), what
    assert got["xor_pos"] == O.xor_reduce(fp + mp.astype(np.uint64)) and got["aux"] == len(mn), what


def check_syncmers(ctx, batch, seq, offsets, k, s, soff, eoff, what):
    got = both(ctx, lambda: batch.syncmers(k, s, soff, eoff, seed=0, canonical=True, capacity=len(seq) + 1), what)
    n, p = O.syncmers(seq, offsets, k, s, soff, eoff, True)
    assert got["count"] == n, (what, got["count"], n)
    assert np.array_equal(got["positions"], p), what
    assert got["xor_pos"] == O.xor_reduce(p), what


# ---- read-tiled, 150 bp: 100 reads are three tiles of 32 reads and four reads; a tile is 4800 bases = 300 chunks
@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "N"])
def test_read_tiled_150(ctx, dirty):
    L, reads = 150, 100
    seq = random_bases(np.random.default_rng(1), L * reads)
    if dirty:
        place_ns(seq, 0, 32 * L, L)
    batch = ctx.upload(seq, read_len=L)
    check_minimizers(ctx, batch, seq, O.fixed_offsets(len(seq), L), 31, 11, "150 bp")
    # a range that starts at read 1: base 150, inside chunk 9
    sub = (reads - 1) * L
    check_minimizers(ctx, batch, seq, O.fixed_offsets(sub, L), 31, 11, "150 bp from read 1", first=L, n=sub)
    batch.close()


# ---- read-tiled, 151 bp: 67 reads = 10117 bases, no multiple of 16; two tiles of 32 reads (302 chunks each) and three reads
@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "N"])
def test_read_tiled_151(ctx, dirty):
    L, reads = 151, 67
    seq = random_bases(np.random.default_rng(2), L * reads)
    if dirty:
        place_ns(seq, L, 32 * L, L)
        seq[5] = ord("n")
    seq[200:260] |= 0x20  # lower case
    seq[300:400][seq[300:400] == ord("T")] = ord("U")
    batch = ctx.upload(seq, read_len=L)
    check_minimizers(ctx, batch, seq, O.fixed_offsets(len(seq), L), 31, 11, "151 bp")
    sub = 40 * L  # reads 1 .. 40: the range starts at base 151, inside chunk 9, and ends inside tile 1
    check_minimizers(ctx, batch, seq, O.fixed_offsets(sub, L), 31, 11, "151 bp, reads 1 .. 40", first=L, n=sub)
    batch.close()


# ---- position-tiled: a contig of three tiles (4032 positions each) with N's across a tile border, and ragged reads
def test_position_tiled(ctx):
    rng = np.random.default_rng(3)
    n = 16 * 750 + 7
    seq = random_bases(rng, n)
    place_ns(seq, 0, 4032, 120)
    seq[4032 - 20:4032 + 20] = ord("N")
    one = np.asarray([0, n], dtype=np.uint64)
    batch = ctx.upload(seq)
    check_minimizers(ctx, batch, seq, one, 31, 11, "contig")
    check_minimizers(ctx, batch, seq, one, 31, 11, "contig, not canonical", canonical=False)
    batch.close()
    clean = random_bases(rng, n)
    batch = ctx.upload(clean)
    check_minimizers(ctx, batch, clean, one, 31, 11, "clean contig")
    check_minimizers(ctx, batch, clean, one, 21, 25, "width 25: the shape the library keeps off the packed copy")
    batch.close()
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + int(rng.integers(100, 152))))
    offsets = np.asarray(cuts, dtype=np.uint64)
    for text, what in ((clean, "ragged reads"), (seq, "ragged reads with N")):
        batch = ctx.upload(text, offsets=offsets)
        check_minimizers(ctx, batch, text, offsets, 31, 11, what)
        batch.close()


# ---- the other shapes that stage through the same two functions, two tiles each
def test_super_kmers_31_15(ctx):
    rng = np.random.default_rng(4)
    L, reads = 150, 50  # read-tiled: 28 reads per tile
    seq = place_ns(random_bases(rng, L * reads), 0, 28 * L, L)
    batch = ctx.upload(seq, read_len=L)
    check_super_kmers(ctx, batch, seq, O.fixed_offsets(len(seq), L), 31, 15, "super-k-mers, reads")
    batch.close()
    n = 8000 + 5  # position-tiled: 4032 - 16 positions per tile
    seq = place_ns(random_bases(rng, n), 0, 4 * (1024 - 32), 120)
    batch = ctx.upload(seq)
    check_super_kmers(ctx, batch, seq, np.asarray([0, n], dtype=np.uint64), 31, 15, "super-k-mers, contig")
    batch.close()


def test_syncmers_31_11(ctx):
    rng = np.random.default_rng(5)
    n = 8000 + 5
    seq = place_ns(random_bases(rng, n), 0, 4 * (1024 - 32), 120)
    batch = ctx.upload(seq)
    check_syncmers(ctx, batch, seq, np.asarray([0, n], dtype=np.uint64), 31, 11, 0, 20, "syncmers, contig")
    batch.close()
    L, reads = 150, 60
    seq = random_bases(rng, L * reads)
    batch = ctx.upload(seq, read_len=L)
    check_syncmers(ctx, batch, seq, O.fixed_offsets(len(seq), L), 31, 11, 0, 20, "syncmers, reads")
    batch.close()


# ---- tiny batches, a batch made without a copy, and a borrowed buffer (bl_batch_from_device: never a copy)
def test_tiny_and_borrowed(ctx):
    import torch

    rng = np.random.default_rng(6)
    seq = random_bases(rng, 150)
    batch = ctx.upload(seq, read_len=150)
    check_minimizers(ctx, batch, seq, np.asarray([0, 150], dtype=np.uint64), 31, 11, "one read")
    batch.close()
    seq = random_bases(rng, 10)
    batch = ctx.upload(seq)
    check_minimizers(ctx, batch, seq, np.asarray([0, 10], dtype=np.uint64), 31, 11, "ten bases, no window")
    check_minimizers(ctx, batch, seq, np.asarray([0, 10], dtype=np.uint64), 4, 3, "ten bases")
    batch.close()

    L, reads = 150, 70
    seq = place_ns(random_bases(rng, L * reads), 0, 32 * L, L)
    offsets = O.fixed_offsets(len(seq), L)
    ctx.set_option("packed_codes", 0)
    try:
        batch = ctx.upload(seq, read_len=L)  # made without a copy: the ASCII path whatever the option says later
    finally:
        ctx.set_option("packed_codes", 1)
    check_minimizers(ctx, batch, seq, offsets, 31, 11, "a batch made without a copy")
    batch.close()
    t = torch.from_numpy(seq).to(ctx.torch_device)
    batch = ctx.from_tensor(t, read_len=L)
    check_minimizers(ctx, batch, seq, offsets, 31, 11, "borrowed, reads")
    batch.close()
    batch = ctx.from_tensor(t)
    check_minimizers(ctx, batch, seq, np.asarray([0, len(seq)], dtype=np.uint64), 31, 11, "borrowed, one sequence")
    batch.close()
