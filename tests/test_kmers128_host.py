"""CPU-only: the host side of the 128-bit k-mer scans — bl_hash64_u128 against reference KATs and the live reference, the Python
model (tests/kmers128_model.py) against the same and against the 64-bit oracle, and the three new symbols in header, binding and library."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import biolib_amd
import kmers128_model as M
import oracle_lib as O
from biolib_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bl_scan_kmers128", "bl_scan_hash_sample128", "bl_hash64_u128")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "kmers128.json")) as f:
        return json.load(f)


def test_host_hash_matches_reference_kats(golden, golden_kats):
    L = capi.lib()
    assert len(golden["hash_kats"]) >= 64
    for lo, hi, seed, h in golden["hash_kats"] + golden_kats["hash64_u128"]:
        assert L.bl_hash64_u128(lo, hi, seed) == h
        assert biolib_amd.hash64_u128(lo, hi, seed) == h
        assert M.hash_u128(lo, hi, seed) == h
    kinds = {(lo == 0, hi == 0) for lo, hi, _, _ in golden["hash_kats"]}
    assert {(True, False), (False, True), (True, True)} <= kinds
    assert any(lo == hi == 2**64 - 1 for lo, hi, _, _ in golden["hash_kats"]) and any(seed >= 2**32 for _, _, seed, _ in golden["hash_kats"])


def test_host_hash_matches_live_reference_on_random_keys():
    """20,000 random keys against hash::hash64::hash<__uint128_t> itself where the reference is built (oracle/_ref); everywhere, the first
    2,000 against the model, which the KATs above pin to the reference"""
    ref = O.ref()
    L = capi.lib()
    rng = np.random.default_rng(20_000)
    keys = rng.integers(0, 2**64 - 1, (20_000, 3), dtype=np.uint64, endpoint=True)
    keys[::7, 1] = 0  # k <= 32: high word 0
    keys[::11, 2] &= np.uint64(0xFFFFFFFF)
    for i, (lo, hi, seed) in enumerate(keys.tolist()):
        got = L.bl_hash64_u128(lo, hi, seed)
        if ref is not None:
            assert got == ref.ref_hash64_u128(lo, hi, seed)
        if i < 2_000:
            assert got == M.hash_u128(lo, hi, seed)
    assert L.bl_hash64_u128(5, 6, 42) == L.bl_hash64_u128(5, 6, 2**32 + 42)  # the seed is truncated to 32 bits


def test_model_equals_64bit_oracle_up_to_32():
    rng = np.random.default_rng(32)
    n = 3_000
    seq = rng.choice(np.frombuffer(b"ACGTacgtUu", np.uint8), n)
    seq[rng.integers(0, n, 12)] = ord("N")
    seq[1500] = 0x80
    seq[1501] = 0xFF
    offs = np.array([0, 1, 40, 72, 700, n], np.uint64)
    for k in (1, 16, 17, 31, 32):
        for canon in (False, True):
            m = M.scan(seq.tobytes(), offs, k, 7, canon, False)
            v, ok = O.units(seq, offs, k, canon)
            assert np.array_equal(m["valid"], ok), (k, canon)
            assert np.array_equal(m["lo"], np.where(ok == 1, v, 0)) and not m["hi"].any(), (k, canon)
            for drop in (False, True):
                d = O.kmer_digest(seq, offs, k, canon, 7, drop_last=drop)
                md = M.digest(M.scan(seq.tobytes(), offs, k, 7, canon, drop))
                assert (md["count"], md["xor_value"], md["aux"]) == (d["count"], d["xor_value"], 0), (k, canon, drop)


def test_golden_scans_are_the_models(golden):
    s = golden["string"].encode()
    assert len(s) == 200 and sum(c not in b"ACGT" for c in s) == 2
    offs = np.array([0, len(s)], np.uint64)
    for k in (33, 48, 64):
        for name, canon in (("forward", False), ("canonical", True)):
            m = M.scan(s, offs, k, golden["seed"], canon, False)
            g = golden["scans"][str(k)][name]
            idx = np.nonzero(m["valid"])[0]
            assert g["positions"] == idx.tolist() and g["lo"] == m["lo"][idx].tolist() and g["hi"] == m["hi"][idx].tolist() and g["hashes"] == m["hashes"][idx].tolist()
            if k > 32:
                assert any(g["hi"])
    assert golden["reference_forward_checked"] is True, golden["reference_forward_note"]


def test_header_binding_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "biolib_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(bl_[a-z0-9_]+)\s*\(", hdr))
    L = capi.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (bl_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in declared and name in capi.SYMBOLS and name in exported and hasattr(L, name), name
    assert "#define BL_VERSION 100" in open(os.path.join(ROOT, "include", "biolib_amd.h")).read()
    assert callable(biolib_amd.hash64_u128) and all(hasattr(biolib_amd.Batch, a) for a in ("kmers128", "kmers128_raw", "hash_sample128"))
