"""CPU-only: bl_scan_read_counts exists, its record is 48 bytes, and it refuses what it can refuse without a device.  (The reduction itself
runs under the sanitizers in test_emu_read_counts.py.)  The refusals below return before any HIP call."""
import ctypes as C

from biolib_amd import capi

INVALID = capi.BL_ERR_INVALID


def test_symbol_is_bound():
    L = capi.lib()
    assert "bl_scan_read_counts" in capi.SYMBOLS and L.bl_scan_read_counts.argtypes is not None and len(L.bl_scan_read_counts.argtypes) == 12


def test_record_is_48_bytes():
    R = capi.ReadCountsRecord
    assert C.sizeof(R) == 48
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [("n_kmers", 0), ("n_found", 4), ("n_solid", 8), ("min_count", 12), ("max_count", 16),
                                                                 ("reserved", 20), ("sum_counts", 24), ("weak_begin", 32), ("weak_end", 40)]
    assert (capi.READ_COUNTS_INIT, capi.READ_COUNTS_ACCUMULATE) == (0, 1)


def test_null_handles_are_refused_with_a_message():
    L = capi.lib()
    res = capi.Result()
    records = (capi.ReadCountsRecord * 2)()
    assert L.bl_scan_read_counts(None, None, 0, 0, 31, 0, None, 1, None, 0, records, C.byref(res)) == INVALID
    assert b"table" in L.bl_last_error()
    assert L.bl_scan_read_counts(None, None, 0, 0, 31, 0, None, 0, None, 0, None, C.byref(res)) == INVALID
    assert L.bl_last_error() != b""
