"""The read-tiled pass 1 does not stage a tile of a batch's packed copy that holds no bad chunk: its lanes read their four dwords from the
copy (frl_tile_clean, bl_scan_frl.hpp).  Every case is scanned that way and again under set_option("direct_codes", 0), which stages every
tile in LDS as before; both results -- every output array, the count, the digest words -- are held against each other and against oracle_lib.

Shapes: a tile of 150-bp reads is 32 reads (4800 bases, 304 staged chunks; 151 bp: 32 reads, 100 bp: 48).  A batch is three full tiles and
one read (97 reads of 150 bp), so the last tile has idle lanes and, ending with the batch, stages guard chunks: it is always staged.  Sub-ranges start at reads 1, 3 and 8 (150 mod 16 = 6:
the tile origin falls at offsets 6, 2 and 0 inside its chunk) and end with the batch or before it.  N's: none, one per tile, in the middle tile
only, on the border of tiles 0 and 1, and just behind tile 1's last read, where tile 1 still stages the chunk.  The per-wave redo flags are
reached with the planted reads of approx_plant.py, in turn in wave 0, 1, 2 and 3 of tile 1 of a batch without N."""
import numpy as np
import pytest

import approx_plant as P
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 42


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.set_option("direct_codes", 1)
    c.close()


def random_bases(seed, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].copy()


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), (what, key)
        else:
            assert a[key] == b[key], (what, key, a[key], b[key])


def both(ctx, scan, what):
    """the scan with clean tiles read from the packed copy, and with every tile staged: equal in every word; returns the first"""
    ctx.set_option("direct_codes", 1)
    direct = scan()
    ctx.set_option("direct_codes", 0)
    try:
        staged = scan()
    finally:
        ctx.set_option("direct_codes", 1)
    same(direct, staged, what)
    return direct


def check_minimizers(ctx, batch, seq, L, unit, w, what, first_read=0, end_read=None, kernel=None):
    reads = len(seq) // L
    end_read = reads if end_read is None else end_read
    first, n = first_read * L, (end_read - first_read) * L
    got = both(ctx, lambda: batch.minimizers(unit, w, seed=SEED, canonical=True, first=first, n=n, capacity=n + 1), what)
    if kernel:
        assert kernel in ctx.last_scan_kernels(), (what, ctx.last_scan_kernels())
    v, p, h = O.minimizers(seq[first:first + n], O.fixed_offsets(n, L), unit, w, SEED, True, brute=False)
    p = p + np.uint64(first)
    assert got["count"] == len(v), (what, got["count"], len(v))
    assert np.array_equal(got["values"], v) and np.array_equal(got["positions"], p) and np.array_equal(got["hashes"], h), what
    assert got["xor_value"] == O.xor_reduce(v) and got["xor_hash"] == O.xor_reduce(h) and got["xor_pos"] == O.xor_reduce(p), what


def with_ns(seq, where):
    seq = seq.copy()
    for q in where:
        seq[q] = ord("N")
    return seq


def n_cases(L, reads):
    """name -> positions of N, for a batch of `reads` reads of L bases that is scanned from read 0"""
    stride = 4 * P.frl_plan(L)["rpw"] * L
    tiles = (reads * L + stride - 1) // stride
    return {
        "no N": [],
        "one N per tile": [t * stride + stride // 3 for t in range(tiles - 1)] + [reads * L - 40],
        "N in the middle tile": [stride + stride // 2],
        "N on the border of tiles 0 and 1": [stride - 1, stride],
        "N behind tile 1": [2 * stride + 20],
    }


# ---- the headline kernel (compile-time geometry, 150 bp) and the run-time-geometry twins (151 bp: NS = 16, 100 bp: NS = 14)
@pytest.mark.parametrize("L,kernel", [(150, "frl<MM,W=11,NS=15,U=31,L=150,approx>"), (151, "frl<MM,W=11,NS=16,U=31,approx>"), (100, "frl<MM,W=11,NS=14,U=31,approx>")])
def test_bad_bases(ctx, L, kernel):
    reads = 3 * P.frl_plan(L)["reads_per_tile"] + 1  # 97 for 150 and 151 bp, 145 for 100 bp (48 reads per tile)
    clean = random_bases(10 + L, L * reads)
    for name, where in n_cases(L, reads).items():
        seq = with_ns(clean, where)
        batch = ctx.upload(seq, read_len=L)
        check_minimizers(ctx, batch, seq, L, 31, 11, f"{L} bp, {name}", kernel=kernel)
        batch.close()


@pytest.mark.parametrize("L", [150, 151, 100])
def test_sub_ranges(ctx, L):
    rpt = P.frl_plan(L)["reads_per_tile"]
    reads = 3 * rpt + 1
    clean = random_bases(20 + L, L * reads)
    dirty = with_ns(clean, n_cases(L, reads)["N in the middle tile"])
    for seq, name in ((clean, "no N"), (dirty, "N in the middle tile")):
        batch = ctx.upload(seq, read_len=L)
        for first_read in (1, 3, 8):
            check_minimizers(ctx, batch, seq, L, 31, 11, f"{L} bp, {name}, reads {first_read} .. end", first_read=first_read)  # ends with the batch: the last tile stages guard chunks
            check_minimizers(ctx, batch, seq, L, 31, 11, f"{L} bp, {name}, reads {first_read} .. {first_read + 2 * rpt}", first_read=first_read,
                             end_read=first_read + 2 * rpt)  # two full tiles that end inside the batch: both direct when clean
        check_minimizers(ctx, batch, seq, L, 31, 11, f"{L} bp, {name}, reads 0 .. {rpt + 8}", end_read=rpt + 8)  # a last tile with idle lanes that is not the batch's last
        batch.close()


# ---- one flag per wave: a planted window pass 1 cannot decide, in turn in wave 0, 1, 2 and 3 of tile 1; every other tile and wave is random
@pytest.mark.parametrize("wave", [0, 1, 2, 3])
def test_wave_redo_flags(ctx, wave):
    import biolib_amd as B

    L, reads = 150, 97
    g = P.frl_plan(L)
    entry = P.case_entries("top_plus_one", "equal_prefix")[0]
    seq = random_bases(30, L * reads)
    read = g["reads_per_tile"] + wave * g["rpw"] + 1
    P.plant(seq, read * L + g["ns"], entry["bases"])
    must, _ = P.redo_bounds(seq, L, "top_plus_one")
    assert 1 in must
    batch = ctx.upload(seq, read_len=L)
    check_minimizers(ctx, batch, seq, L, 31, 11, f"planted in wave {wave}", kernel="frl_redo<MM,W=11,NS=15,U=31,L=150>")
    for direct in (1, 0):
        ctx.set_option("direct_codes", direct)
        try:
            r = batch.minimizers_raw(31, 11, SEED, B.FLAG_CANONICAL | B.FLAG_SYNC)
        finally:
            ctx.set_option("direct_codes", 1)
        assert int(r.redone) >= len(must), (wave, direct, int(r.redone), must)
    batch.close()


# ---- the other read-tiled scans that take the same path: a width of the general minimizer kernels, and super-k-mers (31, 15)
def test_minimizers_w5(ctx):
    L, reads = 150, 70
    clean = random_bases(40, L * reads)
    for seq, name in ((clean, "no N"), (with_ns(clean, [L * 40 + 7]), "N in tile 1")):
        batch = ctx.upload(seq, read_len=L)
        check_minimizers(ctx, batch, seq, L, 31, 5, f"w = 5, {name}", kernel="frl<MM,W=5>")
        check_minimizers(ctx, batch, seq, L, 31, 5, f"w = 5, {name}, from read 3", first_read=3, end_read=67)
        batch.close()


def test_super_kmers_31_15(ctx):
    L, reads = 150, 60  # 28 reads per tile: two tiles and four reads
    clean = random_bases(50, L * reads)
    offsets = O.fixed_offsets(L * reads, L)
    for seq, name in ((clean, "no N"), (with_ns(clean, [28 * L + 100]), "N in tile 1")):
        batch = ctx.upload(seq, read_len=L)
        got = both(ctx, lambda: batch.super_kmers(31, 15, seed=SEED, canonical=True, capacity=len(seq) + 1), name)
        assert "frl<SK,W=17>" in ctx.last_scan_kernels(), ctx.last_scan_kernels()
        mn, fp, mp, sz, hs = O.super_kmers(seq, offsets, 31, 15, SEED, True)
        assert got["count"] == len(mn), (name, got["count"], len(mn))
        for key, want in (("minimizers", mn), ("first_pos", fp), ("mm_pos", mp), ("sizes", sz), ("hashes", hs)):
            assert np.array_equal(got[key], want), (name, key)
        assert got["xor_value"] == O.xor_reduce(mn) and got["xor_hash"] == O.xor_reduce(hs), name
        batch.close()
