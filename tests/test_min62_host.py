"""The claim min62 (bl_scan_core.hpp) rests on: for two 64-bit patterns below 2^62, the IEEE minimum of their readings as doubles is
the integer minimum, and it is one of the operands bit for bit.  Such patterns have sign 0 and an exponent field of at most 0x3ff:
+0, subnormal (below 2^52) or normal, never a NaN or an infinity; and non-negative finite doubles are ordered as their bit patterns.
numpy's float64 minimum on the host stands for the statement here; what the GPU's v_min_f64 does with the same patterns, subnormal
readings included, is test_gpu_min62.py's to check."""
import numpy as np

TOP = (1 << 62) - 1


def check(a, b):
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    assert a.shape == b.shape and int(a.max()) <= TOP and int(b.max()) <= TOP
    fa, fb = a.view(np.float64), b.view(np.float64)
    assert np.isfinite(fa).all() and np.isfinite(fb).all() and not np.signbit(fa).any() and not np.signbit(fb).any()
    got = np.minimum(fa, fb).view(np.uint64)
    want = np.minimum(a, b)
    assert np.array_equal(got, want)
    assert np.all((got == a) | (got == b)), "one operand's bits"
    assert np.array_equal(np.minimum(fb, fa).view(np.uint64), want), "either order"
    assert np.array_equal(fa < fb, a < b), "the order of the readings is the order of the patterns"


def others(rng):
    """values of every kind to set against a fixed one: 0, 1, the ends of the subnormal and of the whole range, random ones"""
    fixed = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, 1 << 61, (1 << 61) - 1, TOP - 1, TOP]
    return np.concatenate([np.array(fixed, np.uint64), rng.integers(0, 1 << 62, 500, dtype=np.uint64), rng.integers(0, 1 << 52, 500, dtype=np.uint64)])


def test_zero_and_the_largest_pattern_against_anything():
    o = others(np.random.default_rng(1))
    check(np.zeros_like(o), o)
    check(np.full_like(o, TOP), o)


def test_equal_operands():
    o = others(np.random.default_rng(2))
    check(o, o.copy())


def test_pairs_that_differ_in_one_part_only():
    rng = np.random.default_rng(3)
    hi = rng.integers(0, 1 << 30, 2000, dtype=np.uint64) << np.uint64(32)
    hi[:200] = 0  # subnormal readings, the high dword all zero
    hi[200:400] &= np.uint64((1 << 52) - 1)  # subnormal readings with bits in the high dword
    lo_a, lo_b = rng.integers(0, 1 << 32, 2000, dtype=np.uint64), rng.integers(0, 1 << 32, 2000, dtype=np.uint64)
    check(hi | lo_a, hi | lo_b)  # only the low dword differs
    check(hi | lo_a, hi | (lo_a ^ np.uint64(1)))  # ... in its lowest bit
    check(hi | lo_a, hi | (lo_a ^ np.uint64(1 << 31)))  # ... in its highest bit
    a = rng.integers(0, 1 << 62, 2000, dtype=np.uint64)
    check(a, a ^ np.uint64(1 << 61))  # only bit 61 differs
    check(a, a ^ np.uint64(1 << 52))  # only the lowest exponent bit differs
    check(a, a ^ np.uint64(1 << 32))  # only the lowest bit of the high dword differs


def test_subnormal_readings():
    rng = np.random.default_rng(4)
    sub_a, sub_b = rng.integers(0, 1 << 52, 3000, dtype=np.uint64), rng.integers(0, 1 << 52, 3000, dtype=np.uint64)
    normal = rng.integers(1 << 52, 1 << 62, 3000, dtype=np.uint64)
    assert (sub_a.view(np.float64) < np.finfo(np.float64).tiny).all() and (normal.view(np.float64) >= np.finfo(np.float64).tiny).all()
    check(sub_a, sub_b)
    check(sub_a, normal)
    check(normal, sub_b)
    small = rng.integers(0, 1 << 20, 3000, dtype=np.uint64)  # a few bits at the very bottom
    check(small, sub_a)
    check(small, small[::-1].copy())


def test_random_pairs():
    rng = np.random.default_rng(5)
    check(rng.integers(0, 1 << 62, 5000, dtype=np.uint64), rng.integers(0, 1 << 62, 5000, dtype=np.uint64))


def test_the_precondition_is_needed():
    """a unit of 32 bases uses all 64 bits: NaN patterns and the sign bit, which is why such units keep the integer form"""
    nan = np.array([0x7FF8000000000001], np.uint64)
    neg = np.array([0x8000000000000001], np.uint64)
    one = np.array([1], np.uint64)
    assert np.isnan(nan.view(np.float64)).all()
    assert np.minimum(neg.view(np.float64), one.view(np.float64)).view(np.uint64)[0] != np.minimum(neg, one)[0]
