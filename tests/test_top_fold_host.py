"""CPU-only: murmur64_top (bl_scan_core.hpp), reached through the host build of tests/emu/ as tests/test_emu_vs_oracle.py does, against
its definition written out here.  The function forms the low dword of the four cross products of its last multiply as
(a1 + a2)*chi + (b1 + b2)*clo; the test states S with the four products apart, a1*chi + b1*clo + a2*chi + b2*clo, and asks for the
same dword, on random keys and on keys built so that the two sums overflow 32 bits.  For both forms (S and S + 1)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hash_top_model as H
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")

M64, M32 = (1 << 64) - 1, (1 << 32) - 1
C1, C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F  # the key's two multiplies
F1, F2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53  # fmix64's
CLO, CHI = F2 & M32, F2 >> 32
SEEDS = (0, 42, 0xFFFFFFFF)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    L = C.CDLL(os.path.join(EMU_DIR, "_build", "libbl_emu.so"))
    L.emu_top_values.argtypes = [C.c_void_p, C.c_uint64, C.c_uint, C.c_int, C.c_void_p]
    L.emu_top_values.restype = None
    return L


def tops(emu, keys, seed, plus_one):
    keys = np.ascontiguousarray(keys, np.uint64)
    out = np.zeros(len(keys), np.uint32)
    emu.emu_top_values(O._ptr(keys), len(keys), seed, int(plus_one), O._ptr(out))
    return out.astype(np.uint64)


# ----------------------------------------------------------------------------- the definition, in Python integers

def before_last_multiply(key, seed):
    """the two 64-bit words the last multiply of each fmix64 takes (Python integers)"""
    k = key * C1 & M64
    k = (k << 31 | k >> 33) & M64
    k = k * C2 & M64
    h2 = seed ^ 8
    h1 = ((seed ^ k ^ 8) + h2) & M64
    h2 = (h2 + h1) & M64
    out = []
    for h in (h1, h2):
        h ^= h >> 33
        h = h * F1 & M64
        h ^= h >> 33
        out.append(h)
    return out


def four_products(key, seed, plus_one):
    """S (or S + 1): the two high products and the four cross products of the last multiplies, each on its own"""
    x1, x2 = before_last_multiply(key, seed)
    a1, b1, a2, b2 = x1 & M32, x1 >> 32, x2 & M32, x2 >> 32
    cross = a1 * CHI + b1 * CLO + a2 * CHI + b2 * CLO
    return ((a1 * CLO >> 32) + (a2 * CLO >> 32) + cross + int(plus_one)) & M32


def dwords_np(keys, seed):
    """a1, b1, a2, b2 of many keys at once (uint64 arrays holding dwords): before_last_multiply in numpy, pinned against it below"""
    U = np.uint64
    with np.errstate(over="ignore"):
        k = np.asarray(keys, np.uint64) * U(C1)
        k = (k << U(31)) | (k >> U(33))
        k = k * U(C2)
        h2 = np.full_like(k, U(seed ^ 8))
        h1 = (U(seed) ^ k ^ U(8)) + h2
        h2 = h2 + h1
        out = []
        for h in (h1, h2):
            h = h ^ (h >> U(33))
            h = h * U(F1)
            h = h ^ (h >> U(33))
            out += [h & U(M32), h >> U(32)]
    return out


def four_products_np(keys, seed, plus_one):
    """four_products for many keys: every product of two dwords fits 64 bits, their sum may wrap, and only its low dword is kept"""
    U = np.uint64
    a1, b1, a2, b2 = dwords_np(keys, seed)
    with np.errstate(over="ignore"):
        cross = a1 * U(CHI) + b1 * U(CLO) + a2 * U(CHI) + b2 * U(CLO)
        return (((a1 * U(CLO)) >> U(32)) + ((a2 * U(CLO)) >> U(32)) + cross + U(int(plus_one))) & U(M32)


# ----------------------------------------------------------------------------- keys whose sums overflow

def key_for(x1, seed):
    """the key whose h1 is x1 just before the last multiply: every step up to there undone (the multipliers are odd: inverses mod 2^64;
    y ^= y >> 33 is its own inverse; the seed's part is subtracted)"""
    h = x1 ^ (x1 >> 33)
    h = h * pow(F1, -1, 1 << 64) & M64
    h ^= h >> 33
    k = ((h - (seed ^ 8)) & M64) ^ seed ^ 8
    k = k * pow(C2, -1, 1 << 64) & M64
    k = (k >> 31 | k << 33) & M64
    return k * pow(C1, -1, 1 << 64) & M64


def overflow_keys(seed):
    """64 keys with a1 = 0xffffffff, 64 with b1 = 0xffffffff, one with both: a1 + a2 (b1 + b2) then overflows unless a2 (b2) is 0"""
    rng = np.random.default_rng(1000 + seed % 1000)
    r = [int(x) for x in rng.integers(0, 1 << 32, 128, dtype=np.uint64)]
    x1 = [r[i] << 32 | M32 for i in range(64)] + [M32 << 32 | r[i] for i in range(64, 128)] + [M64]
    keys = [key_for(x, seed) for x in x1]
    for k, x in zip(keys, x1):
        assert before_last_multiply(k, seed)[0] == x
    return keys


def test_inversion_and_numpy_restatement():
    rng = np.random.default_rng(2)
    keys = rng.integers(0, 1 << 62, 2000, dtype=np.uint64)
    for seed in SEEDS:
        a1, b1, a2, b2 = dwords_np(keys, seed)
        for i in range(0, 2000, 7):
            x1, x2 = before_last_multiply(int(keys[i]), seed)
            assert (x1, x2) == (int(b1[i]) << 32 | int(a1[i]), int(b2[i]) << 32 | int(a2[i]))
            assert key_for(x1, seed) == int(keys[i])
            for plus_one in (False, True):
                assert four_products(int(keys[i]), seed, plus_one) == int(four_products_np(keys[i:i + 1], seed, plus_one)[0])


@pytest.mark.parametrize("plus_one", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_top_is_the_four_product_sum_on_random_keys(emu, seed, plus_one):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 1 << 62, 1 << 20, dtype=np.uint64)
    keys[:4] = (0, 1, (1 << 62) - 1, (1 << 61) + 1)
    got = tops(emu, keys, seed, plus_one)
    assert np.array_equal(got, four_products_np(keys, seed, plus_one))
    for i in range(0, 1 << 20, 1 << 8):  # ... and the same in Python integers on every 256th
        assert int(got[i]) == four_products(int(keys[i]), seed, plus_one)
    # the hash's high dword T is S or S + 1 (the value or one below it for the S + 1 form)
    t = H.hash64(keys, seed) >> np.uint64(32)
    d = (t - got) & np.uint64(M32)
    assert np.isin(d, [M32, 0] if plus_one else [0, 1]).all()
    a1, b1, a2, b2 = dwords_np(keys, seed)  # about half of these overflow each sum, too
    assert int(((a1 + a2) >> np.uint64(32)).sum()) > 1 << 18 and int(((b1 + b2) >> np.uint64(32)).sum()) > 1 << 18


@pytest.mark.parametrize("plus_one", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_top_on_keys_built_to_overflow_both_sums(emu, seed, plus_one):
    keys = overflow_keys(seed)
    over_a = over_b = 0
    for k in keys:
        x1, x2 = before_last_multiply(k, seed)
        over_a += (x1 & M32) + (x2 & M32) > M32
        over_b += (x1 >> 32) + (x2 >> 32) > M32
    assert over_a >= 32 and over_b >= 32, (over_a, over_b)
    arr = np.array(keys, np.uint64)
    got = tops(emu, arr, seed, plus_one)
    for k, g in zip(keys, got):
        assert int(g) == four_products(k, seed, plus_one), hex(k)
    t = H.hash64(arr, seed) >> np.uint64(32)
    d = (t - got) & np.uint64(M32)
    assert np.isin(d, [M32, 0] if plus_one else [0, 1]).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_top_on_the_largest_sums_of_a_search(emu, seed):
    """the other way to the same keys: of 2^22 random 62-bit keys (which the scans can actually hold), the 64 with the largest a1 + a2 and
    the 64 with the largest b1 + b2"""
    rng = np.random.default_rng(77 + seed % 1000)
    keys = rng.integers(0, 1 << 62, 1 << 22, dtype=np.uint64)
    a1, b1, a2, b2 = dwords_np(keys, seed)
    pick = np.concatenate([np.argsort(a1 + a2)[-64:], np.argsort(b1 + b2)[-64:]])
    assert int(((a1 + a2)[pick[:64]] >> np.uint64(32)).sum()) >= 32 and int(((b1 + b2)[pick[64:]] >> np.uint64(32)).sum()) >= 32
    sel = keys[pick]
    for plus_one in (False, True):
        got = tops(emu, sel, seed, plus_one)
        for k, g in zip(sel, got):
            assert int(g) == four_products(int(k), seed, plus_one), hex(int(k))
        d = ((H.hash64(sel, seed) >> np.uint64(32)) - got) & np.uint64(M32)
        assert np.isin(d, [M32, 0] if plus_one else [0, 1]).all()
