"""CPU-only: the read side of the 16-byte spill formats on files the REFERENCE wrote (tests/golden/spill128/, generator
make_spill128_golden.py): a run file of emem::external_memory_vector<__uint128_t> and an io::basic_store'd std::vector<__uint128_t>."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SP = os.path.join(HERE, "golden", "spill128")


def _sorted(keys):
    return keys[np.lexsort((keys[:, 0], keys[:, 1]))]  # numeric order of hi << 64 | lo


def test_fixture_is_what_the_issue_asks_for():
    keys = np.load(os.path.join(SP, "keys.npy"))
    assert keys.dtype == np.uint64 and keys.ndim == 2 and keys.shape[1] == 2 and 2500 <= len(keys) <= 3500
    assert len(np.unique(keys, axis=0)) < len(keys) and not np.array_equal(keys, _sorted(keys))  # duplicates, unsorted
    assert (keys[:, 1] >> np.uint64(2 * 41 - 64)).max() == 0 and keys[:, 1].max() > 0  # 41-mers: 82 bits
    for fn in ("tmp.run_first_0.bin", "vector.bin"):
        assert os.path.getsize(os.path.join(SP, fn)) < 100_000


def test_read_side_host(tmp_path):
    from biolib_amd import capi

    L = capi.lib()
    exp = _sorted(np.load(os.path.join(SP, "keys.npy")))
    for fn, with_count in (("tmp.run_first_0.bin", 0), ("vector.bin", 1)):
        path = os.path.join(SP, fn).encode()
        n = C.c_uint64()
        capi.check(L.bl_file_count_u128(path, with_count, C.byref(n)))
        assert n.value == len(exp)
        out = np.zeros((n.value, 2), np.uint64)
        capi.check(L.bl_read_file_u128_host(path, with_count, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        assert np.array_equal(out, exp)
        assert L.bl_read_file_u128_host(path, with_count, out.ctypes.data_as(C.c_void_p), n.value - 1, C.byref(n)) == capi.BL_ERR_CAPACITY
        assert n.value == len(exp)
    # the run file read as a stored vector and the other way round: sizes that do not fit are refused
    n = C.c_uint64()
    assert L.bl_file_count_u128(os.path.join(SP, "tmp.run_first_0.bin").encode(), 1, C.byref(n)) == capi.BL_ERR_INVALID
    assert L.bl_file_count_u128(os.path.join(SP, "vector.bin").encode(), 0, C.byref(n)) == capi.BL_ERR_INVALID
    bad = tmp_path / "odd.bin"
    bad.write_bytes(b"\x00" * 24)
    assert L.bl_file_count_u128(str(bad).encode(), 0, C.byref(n)) == capi.BL_ERR_INVALID
    assert L.bl_file_count_u128(str(bad).encode(), 1, C.byref(n)) == capi.BL_ERR_INVALID
    assert L.bl_file_count_u128(str(tmp_path / "missing.bin").encode(), 0, C.byref(n)) == capi.BL_ERR_INVALID
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    capi.check(L.bl_file_count_u128(str(empty).encode(), 0, C.byref(n)))
    assert n.value == 0
    capi.check(L.bl_read_file_u128_host(str(empty).encode(), 0, None, 0, C.byref(n)))


def test_count_word_whose_product_wraps_is_refused(tmp_path):
    """stored vectors whose count word times the element size wraps around 2^64 to the body's length: 2^61 + 1 over an 8-byte body (the
    case that passes a product check of 8-byte elements) and 2^60 + 1 over a 16-byte body (the same for 16-byte elements)"""
    from biolib_amd import capi

    L = capi.lib()
    n = C.c_uint64(5)
    out = np.zeros((4, 2), np.uint64)
    for name, words in (("wrap8.bin", [(1 << 61) + 1, 7]), ("wrap16.bin", [(1 << 60) + 1, 7, 9])):
        bad = tmp_path / name
        bad.write_bytes(np.array(words, np.uint64).tobytes())
        assert L.bl_file_count_u128(str(bad).encode(), 1, C.byref(n)) == capi.BL_ERR_INVALID and n.value == 0
        assert b"16-byte elements (count word and file size disagree)" in L.bl_last_error()
        assert L.bl_read_file_u128_host(str(bad).encode(), 1, out.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == capi.BL_ERR_INVALID
        assert not out.any()
    # a sound vector of one element next to them
    good = tmp_path / "one.bin"
    good.write_bytes(np.array([1, 7, 9], np.uint64).tobytes())
    capi.check(L.bl_read_file_u128_host(str(good).encode(), 1, out.ctypes.data_as(C.c_void_p), 4, C.byref(n)))
    assert n.value == 1 and out[0].tolist() == [7, 9]
