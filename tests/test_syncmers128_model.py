"""CPU-only: the Python model of bl_scan_syncmers128 (tests/syncmers128_model.py) held against what is already pinned — with 8-byte
keys against the 64-bit syncmer oracle (rule and tie order), with 16-byte keys against the golden file whose forward strand was
checked against the reference, its hash against the reference's and the library's host hash — and the new symbol in header,
binding and library."""
import json
import os
import re

import numpy as np
import pytest

import biolib_amd
import kmers128_model as K
import oracle_lib as O
import syncmers128_model as M
from biolib_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "syncmers128.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def batch20k():
    """20 kbp, reads of many lengths, N and lower case, bytes >= 0x80"""
    rng = np.random.default_rng(20)
    n = 20_000
    seq = rng.choice(np.frombuffer(b"ACGTacgtUu", np.uint8), n)
    seq[rng.integers(0, n, 25)] = ord("N")
    seq[7000] = 0x80
    seq[[0, n - 1]] = ord("A")
    cuts = np.unique(np.concatenate([[0, 1, 32, 63, 95, 245, n], rng.integers(300, n - 300, 40)]))
    return seq, cuts.astype(np.uint64)


@pytest.mark.parametrize("k,s,offs", ((31, 11, (0, 20)), (21, 8, (2, 5)), (32, 32, (0, 0)), (15, 5, (0, 10))))
def test_width8_equals_the_64bit_oracle(batch20k, k, s, offs):
    seq, cuts = batch20k
    for canonical in (False, True):
        for drop_last in (False, True):
            m = M.scan(seq.tobytes(), cuts, k, s, 0, canonical, drop_last, width=8)
            got = M.syncmers(m, *offs)
            n, pos = O.syncmers(seq, cuts, k, s, offs[0], offs[1], canonical, drop_last)
            assert got["count"] == n > 0 and np.array_equal(got["positions"], pos), (k, s, canonical, drop_last)
    # ties exist in this batch for short s-mers: the tie order is exercised, not assumed
    if s <= 8:
        assert M.scan(seq.tobytes(), cuts, k, s, 0, True, False, width=8)["tied"].any()


def test_width16_equals_golden(golden):
    assert golden["reference_forward_checked"] is True, golden["reference_forward_note"]
    assert len(golden["strings"]["s200"]) == 200 and len(golden["strings"]["s600"]) == 600 and golden["strings"]["s200"].upper().count("N") == 2
    for name, text in golden["strings"].items():
        cuts = np.array([0, len(text)], np.uint64)
        for shape, entry in golden["cases"][name].items():
            k, s = (int(x) for x in shape.split(","))
            for strand, canonical in (("forward", False), ("canonical", True)):
                m = M.scan(text.encode(), cuts, k, s, golden["seed"], canonical, False, 16)
                idx = np.nonzero(m["valid"])[0]
                e = entry[strand]
                assert e["positions"] == idx.tolist() and e["offsets"] == m["offset"][idx].tolist() and len(idx) > 0, (name, shape, strand)
                for key in ("closed", "open"):
                    a, b = e[key]["offsets"]
                    assert e[key]["positions"] == M.syncmers(m, a, b)["positions"].tolist(), (name, shape, strand, key)
    assert set(golden["cases"]["s200"]) == {"33,11", "48,17", "64,32", "64,1"}


def test_strided_evaluation_equals_the_rule_word_for_word(batch20k):
    """every k-mer of a 2-kbp piece: offset and tie flag from the strided views against extractor_offset on the k-mer's value"""
    seq, _ = batch20k
    piece = seq[5000:7100].tobytes()  # holds N and the byte 0x80
    cuts = np.array([0, 700, len(piece)], np.uint64)
    for k, s, width in ((33, 11, 16), (64, 32, 16), (64, 1, 16), (40, 3, 16), (31, 4, 8)):
        m = M.scan(piece, cuts, k, s, 7, True, False, width)
        idx = np.nonzero(m["valid"])[0]
        assert len(idx) > 500 and m["strand"][idx].any() and not m["strand"][idx].all()
        for p in idx.tolist():
            v = int(m["lo"][p]) | (int(m["hi"][p]) << 64)
            off, times = M.extractor_offset(v, k, s, 7, width)
            assert (off, times > 1) == (int(m["offset"][p]), bool(m["tied"][p])), (k, s, p)
        if s <= 4:
            assert m["tied"][idx].any()


def test_key_hash_is_the_reference_hash_of_a_16_byte_value():
    rng = np.random.default_rng(16)
    x = rng.integers(0, 2**64 - 1, 3000, dtype=np.uint64, endpoint=True)
    x[:70] = [1 << i for i in range(64)] + [0, 2**64 - 1, 3, 2**62, 2**32, 2**32 - 1]
    ref = O.ref()
    for seed in (0, 42, 0xFFFFFFFF, 2**32 + 42):
        h16, h8 = M.hash_keys(x, seed, 16), M.hash_keys(x, seed, 8)
        for i, key in enumerate(x.tolist()):
            assert int(h16[i]) == biolib_amd.hash64_u128(key, 0, seed) == K.hash_u128(key, 0, seed)
            assert int(h8[i]) == biolib_amd.hash64(key, seed)
            if ref is not None and i < 1000:
                assert int(h16[i]) == ref.ref_hash64_u128(key, 0, seed)
        assert not np.array_equal(h16, h8)


def test_symbol_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "biolib_amd.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+bl_scan_syncmers128\s*\(", header) and "bl_scan_syncmers128" in capi.SYMBOLS
    L = capi.lib()
    assert L.bl_scan_syncmers128.argtypes is not None and len(L.bl_scan_syncmers128.argtypes) == 13
    assert hasattr(biolib_amd.scan.Batch, "syncmers128") and hasattr(biolib_amd.scan.Batch, "syncmers128_raw")
