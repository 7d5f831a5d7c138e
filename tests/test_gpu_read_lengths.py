"""Every fixed read length, on the kernels.  plan_scan_frl_for decides from the read length alone whether a batch of fixed-length reads takes the
read-tiled layout and with which geometry (lanes per read, reads per wave — with its reciprocal division and its LDS cap —, units per lane, the halo
rule, a floating-point efficiency comparison against the position-tiled layout): each of these flips at lengths nobody chose.  So: every length from
one window per read to the largest the plan accepts, and 32 beyond it (the position-tiled fallback), for minimizers (31, 11) on both strands, (15, 5),
(15, 10), (20, 19) and super-k-mers (31, 15); two full tiles plus three reads with N's and one read of repeats; every array and the digest against
the oracle, and the layout the scan recorded against the plan's.  The same loop through the CPU emulation, and what the lengths reach in the
planner: test_kernel_cases.py."""
import pytest

import kernel_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("block", range(K.LENGTH_BLOCKS))
@pytest.mark.parametrize("shape", K.LENGTH_SHAPES, ids=K.P.ids)
def test_read_lengths_vs_oracle(ctx, shape, block):
    entry, unit, w, canonical = shape
    taken = 0
    for L in K.length_block(shape, block):
        r = K.length_row(shape, L)
        seq, offs, read_len, g = K.length_input(shape, L)
        b = ctx.upload(seq, read_len=read_len)
        try:
            cap = len(seq) + 1
            if entry == "minimizers":
                got = b.minimizers(unit, w, seed=K.SEED, canonical=bool(canonical), capacity=cap)
            else:
                got = b.super_kmers(unit + w - 1, unit, seed=K.SEED, canonical=bool(canonical), capacity=cap)
        finally:
            b.close()
        names = ctx.last_scan_kernels()
        assert names[0].startswith("frl<") == (g is not None), (shape, L, names)
        if g and (unit, w, canonical) == (31, 11, 1):
            assert f"NS={g['ns']}," in names[0] and names[-1] == "emit<MM,C3>", (shape, L, names)
        K.assert_same(entry, got, K.expected(r, seq, offs, read_len), (shape, L, names))
        taken += g is not None
    assert taken > 10
