"""CPU-only: the count-table entry points exist and refuse what they can refuse without a device.  (That the library builds and exports
every symbol the header declares is test_capi_symbols.py's; the search itself runs under the sanitizers in test_emu_lookup.py.)
The refusals below return before any HIP call: NULL handles and NULL output pointers."""
import ctypes as C

import numpy as np

from biolib_amd import capi

INVALID = capi.BL_ERR_INVALID


def test_symbols_are_bound():
    L = capi.lib()
    for name in ("bl_table_build_u64", "bl_table_build_u128", "bl_table_destroy", "bl_table_info", "bl_table_arrays", "bl_table_lookup_u64",
                 "bl_table_lookup_u128", "bl_table_histogram", "bl_scan_kmer_counts"):
        assert name in capi.SYMBOLS and getattr(L, name).argtypes is not None


def test_null_arguments_are_refused_with_a_message():
    L = capi.lib()
    out = C.c_void_p()
    for build in (L.bl_table_build_u64, L.bl_table_build_u128):
        assert build(None, None, None, 0, 62, C.byref(out)) == INVALID and out.value is None
    n, kw = C.c_uint64(), C.c_uint32()
    assert L.bl_table_info(None, C.byref(n), C.byref(kw), None, None) == INVALID
    assert b"NULL" in L.bl_last_error()
    keys, counts = C.c_void_p(), C.c_void_p()
    assert L.bl_table_arrays(None, C.byref(keys), C.byref(counts)) == INVALID
    assert L.bl_table_lookup_u64(None, None, None, 0, None) == INVALID
    assert L.bl_table_lookup_u128(None, None, None, 0, None) == INVALID
    hist = np.zeros(4, np.uint64)
    assert L.bl_table_histogram(None, None, hist.ctypes.data_as(C.c_void_p), 4) == INVALID
    res = capi.Result()
    assert L.bl_scan_kmer_counts(None, None, 0, 0, 31, 0, None, None, None, C.byref(res)) == INVALID
    assert b"table" in L.bl_last_error()
    assert L.bl_table_destroy(None) == capi.BL_OK  # as free(NULL)
