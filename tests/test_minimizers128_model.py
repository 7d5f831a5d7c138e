"""CPU-only: the Python model of bl_scan_minimizers128 (tests/minimizers128_model.py) held against what is already pinned — with 8-byte
keys against the 64-bit minimizer oracle (record rule and tie order), with 16-byte keys against the golden hashes the reference
checked, against a word-for-word evaluation of single windows — and the new symbol in header, binding and library."""
import json
import os
import re

import numpy as np
import pytest

import biolib_amd
import minimizers128_model as M
import oracle_lib as O
from biolib_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.mark.parametrize("unit,w", ((31, 11), (15, 17), (32, 64), (5, 1)))
def test_width8_equals_the_64bit_oracle(batch20k, unit, w):
    seq, cuts = batch20k
    for canonical in (False, True):
        m = M.scan(seq.tobytes(), cuts, unit, w, 42, canonical, False, width=8)
        got = M.minimizers(m)
        v, p, h = O.minimizers(seq, cuts, unit, w, 42, canonical, brute=True)
        assert got["count"] == len(v) > 0, (unit, w, canonical)
        assert np.array_equal(got["lo"], v) and np.array_equal(got["positions"], p) and np.array_equal(got["hashes"], h) and not got["hi"].any()
    # short units repeat: tied minima exist in this batch, the tie order is exercised and not assumed
    if unit == 5:
        assert M.scan(seq.tobytes(), cuts, 5, 7, 42, True, False, width=8)["tied"].any()
        m = M.scan(seq.tobytes(), cuts, 5, 7, 42, True, False, width=8)
        v, p, h = O.minimizers(seq, cuts, 5, 7, 42, True, brute=True)
        got = M.minimizers(m)
        assert np.array_equal(got["positions"], p) and np.array_equal(got["lo"], v)


def test_width16_hashes_equal_golden():
    with open(os.path.join(ROOT, "tests", "golden", "kmers128.json")) as f:
        golden = json.load(f)
    assert golden["reference_forward_checked"] is True, golden["reference_forward_note"]
    text = golden["string"]
    cuts = np.array([0, len(text)], np.uint64)
    for k in (33, 48, 64):
        e = golden["scans"][str(k)]["forward"]
        m = M.scan(text.encode(), cuts, k, 5, golden["seed"], False, False, 16)
        idx = np.nonzero(m["valid"])[0]
        assert idx.tolist() == e["positions"] and len(idx) > 0
        assert m["hashes"][idx].tolist() == e["hashes"] and m["lo"][idx].tolist() == e["lo"] and m["hi"][idx].tolist() == e["hi"]
        # every record's hash is one of them, at its position
        r = M.minimizers(m)
        assert r["count"] > 0 and all(e["hashes"][e["positions"].index(int(p))] == int(h) for p, h in zip(r["positions"], r["hashes"]))


def test_vectorised_windows_equal_the_rule_word_for_word(batch20k):
    seq, cuts = batch20k
    rng = np.random.default_rng(3)
    seen_missing = seen_tied = 0
    for unit, w, canonical in ((33, 11, True), (64, 64, False), (40, 2, True), (3, 9, True)):
        m = M.scan(seq.tobytes(), cuts, unit, w, 7, canonical, True, 16)
        for p in rng.integers(0, len(seq), 50).tolist():
            exists, occ = M.window_by_hand(m, p, 7)
            assert (exists, occ) == (bool(m["exist"][p]), int(m["occ"][p])), (unit, w, p)
            seen_missing += not exists
            seen_tied += bool(m["tied"][p])
        rec = M.minimizers(m)
        # the record rule by hand on the first 300 windows
        last, want = None, []
        for p in range(300):
            exists, occ = M.window_by_hand(m, p, 7)
            if exists and occ != last:
                want.append(occ)
            last = occ if exists else None
        assert rec["positions"][rec["windows"] < 300].tolist() == want
    assert seen_missing > 0 and seen_tied > 0


def test_symbol_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "biolib_amd.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+bl_scan_minimizers128\s*\(", header) and "bl_scan_minimizers128" in capi.SYMBOLS
    L = capi.lib()
    assert L.bl_scan_minimizers128.argtypes is not None and len(L.bl_scan_minimizers128.argtypes) == 13
    assert hasattr(biolib_amd.scan.Batch, "minimizers128") and hasattr(biolib_amd.scan.Batch, "minimizers128_raw")
    with open(os.path.join(ROOT, "include", "compat", "minimizer_sampler.hpp")) as f:
        assert "is not provided" not in f.read()
