"""The C3 shape (canonical 31-mers, w = 11, 150-bp reads: scan_count_frl_kernel<0,11,15,31,150,1,true>, scan_redo_frl_kernel and
scan_emit_kernel<0,31,1,1>) against the oracle on the inputs its two passes treat specially: units taken by direct extraction in
pass 1 and from two staged strands in pass 2, windows decided on murmur64_top<true> with a redo for a minimum at prefix 0."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

L = 150
K, W, SEED = 31, 11, 42
# canonical 31-mers whose hash (seed 42) has a high dword below 64 or above 0xffffffc0: prefix 0 and prefix all ones of the packed
# keys pass 1 compares (found by search with oracle_lib.hash64_np; checked below)
LOW_PREFIX = [2393889798664489993, 2793802494497477368, 995647800767030434, 1372974326945987553]
HIGH_PREFIX = [799355525284604741]


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def kmer_bases(v):
    return np.frombuffer(bytes(b"ACGT"[(v >> (2 * (K - 1 - i))) & 3] for i in range(K)), np.uint8)


def revcomp(a):
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[x] = y
    return comp[a[::-1]]


def check(ctx, seq, want_redo=False):
    import biolib_amd as B

    offs = O.fixed_offsets(len(seq), L)
    b = ctx.upload(seq, offs)
    try:
        v, p, h = O.minimizers(seq, offs, K, W, SEED, True, brute=False)
        got = b.minimizers(K, W, seed=SEED, canonical=True)
        assert got["count"] == len(v)
        assert np.array_equal(got["positions"], p) and np.array_equal(got["values"], v) and np.array_equal(got["hashes"], h)
        cap = max(len(v), 1)
        vv, pp, hh = ctx.empty_u64(cap), ctx.empty_u64(cap), ctx.empty_u64(cap)
        r = b.minimizers_raw(K, W, SEED, B.FLAG_CANONICAL | B.FLAG_SYNC, values=vv, positions=pp, hashes=hh, capacity=cap)
        assert int(r.count) == len(v)
        if want_redo:
            assert int(r.redone) > 0
        return int(r.redone)
    finally:
        b.close()


def test_special_keys_are_what_they_claim():
    hi = lambda v: int(O.hash64_np(np.array([v], np.uint64), SEED)[0]) >> 32
    for v in LOW_PREFIX:
        assert hi(v) < 64
    for v in HIGH_PREFIX:
        assert hi(v) >= 0xFFFFFFC0
    for v in LOW_PREFIX + HIGH_PREFIX:  # canonical: the smaller strand
        bases = kmer_bases(v)
        rc = revcomp(bases)
        rv = 0
        for c in rc:
            rv = (rv << 2) | b"ACGT".index(bytes([c]))
        assert v < rv


@pytest.mark.parametrize("edge", ["first", "last", "both", "inner_lane_borders"])
def test_c3_breaks_at_read_edges(ctx, edge):
    n_reads = 32 * 6 + 7
    seq = O.synth(11, n_reads * L).copy()
    rng = np.random.default_rng(3)
    for r in rng.choice(n_reads, n_reads // 3, replace=False):
        at = {"first": [0, 1], "last": [L - 1, L - 2], "both": [0, L - 1], "inner_lane_borders": [15, 30, 44, 45, 119, 120]}[edge]
        for o in at:
            seq[r * L + o] = ord("N") if rng.random() < 0.7 else ord("x")
    check(ctx, seq)


def test_c3_reverse_complement_palindromes(ctx):
    """reads whose second half is the reverse complement of the first: unit s and unit L - K - s are each other's reverse
    complement and have the same canonical value — equal keys in the same read, the tie pass 1 must hand to the redo kernel"""
    n_reads = 32 * 5 + 3
    seq = O.synth(12, n_reads * L).copy()
    for r in range(0, n_reads, 2):
        half = seq[r * L:r * L + L // 2]
        seq[r * L + L // 2:(r + 1) * L] = revcomp(half)
    check(ctx, seq)


def test_c3_reads_of_repeats_every_tile_redone(ctx):
    n_reads = 32 * 8
    motifs = [b"A", b"AC", b"ACG", b"AAAT", b"ACGTT", b"ACGTACGTAC"]
    seq = np.concatenate([np.resize(np.frombuffer(motifs[t % len(motifs)], np.uint8), 32 * L) for t in range(n_reads // 32)])
    check(ctx, seq, want_redo=True)  # (every window holds a key twice)


@pytest.mark.parametrize("which", ["low", "high", "both"])
def test_c3_keys_at_prefix_zero_and_all_ones(ctx, which):
    """31-mers whose hash prefix is 0 (murmur64_top<true> may have wrapped there: the tile is decided again) or all ones, planted at
    unit starts across the lane map (lane borders at multiples of 15, the last unit of a read at 119) in random reads"""
    n_reads = 32 * 6
    seq = O.synth(13, n_reads * L).copy()
    pick = {"low": LOW_PREFIX, "high": HIGH_PREFIX, "both": LOW_PREFIX + HIGH_PREFIX}[which]
    rng = np.random.default_rng(5)
    starts = [0, 1, 13, 14, 15, 16, 29, 30, 60, 104, 105, 118, 119]
    for r in range(n_reads):
        o = starts[r % len(starts)]
        v = pick[r % len(pick)]
        bases = kmer_bases(v)
        seq[r * L + o:r * L + o + K] = bases if rng.random() < 0.5 else revcomp(bases)
    check(ctx, seq, want_redo=(which != "high"))
