"""CPU-only: the table of tests/kernel_cases.py (one scan per kernel the launchers can choose) against the library's own list of kernel names, and
its inputs — and every fixed read length of test_gpu_read_lengths.py — through the CPU emulation of the kernels, record for record against the
oracle.  The emulation runs the planner and the phase code of the kernels, so a disagreement here is a planner or phase bug; one that shows only
in test_gpu_kernel_census.py / test_gpu_read_lengths.py lies in what the emulation does not model: cross-lane and LDS code, and the launchers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kernel_cases as K
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    L = C.CDLL(os.path.join(EMU_DIR, "_build", "libbl_emu.so"))
    vp, u64, u = C.c_void_p, C.c_uint64, C.c_uint
    L.emu_batch.restype = vp
    L.emu_batch.argtypes = [vp, u64, vp, u64, u64]
    L.emu_batch_free.argtypes = [vp]
    L.emu_minimizers.argtypes = [vp, u64, u64, u, u, u64, u, vp, vp, vp, u64, vp]
    L.emu_hash_sample.argtypes = [vp, u64, u64, u, u64, u64, u, vp, vp, vp, u64, vp]
    L.emu_super_kmers.argtypes = [vp, u64, u64, u, u, u64, u, vp, vp, vp, vp, vp, u64, vp]
    L.emu_syncmers.argtypes = [vp, u64, u64, u, u, u, u, u64, u, vp, u64, vp]
    return L


def emu_scan(emu, r, seq, offs, read_len, first=0, n=0):
    """the row's scan through the emulated kernels: what kernel_cases.assert_same compares, and whether the read-tiled path was taken"""
    b = emu.emu_batch(O._ptr(seq), len(seq), None if read_len else O._ptr(offs), 0 if read_len else len(offs) - 1, read_len)
    cap = len(seq) + 1
    a = [np.zeros(cap, np.uint64) for _ in range(3)]
    res = np.zeros(8, np.uint64)
    frl = emu.emu_frl_scans()
    flags = 1 if r.canonical else 0
    try:
        if r.entry == "minimizers":
            emu.emu_minimizers(b, first, n, r.unit, r.w, K.SEED, flags, O._ptr(a[0]), O._ptr(a[1]), O._ptr(a[2]), cap, O._ptr(res))
        elif r.entry == "hash_sample":
            emu.emu_hash_sample(b, first, n, r.unit, K.SEED, K.THRESHOLD, flags, O._ptr(a[0]), O._ptr(a[1]), O._ptr(a[2]), cap, O._ptr(res))
        elif r.entry == "super_kmers":
            mp, sz = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
            emu.emu_super_kmers(b, first, n, r.unit + r.w - 1, r.unit, K.SEED, flags, O._ptr(a[0]), O._ptr(a[1]), O._ptr(mp), O._ptr(sz), O._ptr(a[2]), cap, O._ptr(res))
        else:
            emu.emu_syncmers(b, first, n, r.unit + r.w - 1, r.unit, r.offsets[0], r.offsets[1], 0, flags, O._ptr(a[0]), cap, O._ptr(res))
    finally:
        emu.emu_batch_free(b)
    c = int(res[0])
    got = dict(count=c, xor_value=int(res[1]), xor_hash=int(res[2]), xor_pos=int(res[3]), aux=int(res[4]))
    if r.entry in ("minimizers", "hash_sample"):
        got.update(values=a[0][:c], positions=a[1][:c], hashes=a[2][:c])
    elif r.entry == "super_kmers":
        got.update(minimizers=a[0][:c], first_pos=a[1][:c], mm_pos=mp[:c], sizes=sz[:c], hashes=a[2][:c])
    else:
        got.update(positions=a[0][:c])
    return got, emu.emu_frl_scans() - frl


# ----------------------------------------------------------------------------- the table

def test_one_row_for_every_name_the_library_lists():
    import biolib_amd

    listed = biolib_amd.Context.scan_kernel_names()
    assert len(listed) == len(set(listed)) > 100
    claimed = {n for r in K.ROWS for n in r.names}
    assert claimed == set(listed), (sorted(claimed - set(listed)), sorted(set(listed) - claimed))
    for w in range(2, 33):
        assert f"count<MM,W={w}>" in listed and f"count<SK,W={w}>" in listed
    assert len({K.row_id(r) for r in K.ROWS}) == len(K.ROWS)


def test_the_name_calls_report_the_bytes_they_need():
    from biolib_amd import capi

    L = capi.lib()
    need = C.c_uint64()
    assert L.bl_scan_kernel_names(None, 0, C.byref(need)) == capi.BL_ERR_CAPACITY and need.value > 1000
    buf = C.create_string_buffer(b"\x7f" * int(need.value), int(need.value))
    assert L.bl_scan_kernel_names(buf, need.value - 1, None) == capi.BL_ERR_CAPACITY and buf.raw == b"\x7f" * int(need.value)  # nothing written
    assert L.bl_scan_kernel_names(buf, need.value, None) == capi.BL_OK
    assert buf.raw[-2:] == b"\n\x00" and buf.raw.count(b"\n") == len(buf.value.split())


def test_the_inputs_reach_the_edges_they_are_for():
    for r in K.ROWS:
        if r.read_len:
            continue
        mode = K.MODE[r.entry]
        seq, offs, _, g = K.contig(mode, r.w)
        border = g["origin"] + 2 * g["stride"]
        text = bytes(seq).upper()
        assert text[border - 48:border + 48] == b"A" * 96 and text[border - 176:border - 48] == b"ACGTTACA" * 16
        assert 3 * g["stride"] < len(seq) - g["origin"] < 4 * g["stride"]
        _, offs_b, _, _ = K.ragged(mode, r.unit, r.w, False)
        seq_n, offs_n, _, _ = K.ragged(mode, r.unit, r.w, True)
        places = K.planted_places(g)
        assert set(places) <= set(offs_b.tolist()) and not set(places) & set(offs_n.tolist()) and all(seq_n[p] == ord("N") for p in places)
        lens = set(np.diff(offs_b.astype(np.int64)).tolist())
        assert 1 in lens and (r.unit + r.w - 1 in lens or r.w == 1) and any(x < r.unit for x in lens)
        assert (places[1] - g["origin"]) % g["stride"] == 0 and (places[4] - g["origin"]) % g["stride"] == g["stride"] // 4 == g["own"]


@pytest.mark.parametrize("fam", K.FAMILIES)
def test_minimizer_occurrences_are_the_oracles_groups(fam):
    """kernel_cases.expected takes the minimizers of a sub-range from the oracle's super-k-mer groups (range_minimizers): over the whole batch
    that view must be oracle_lib.minimizers itself"""
    for r in K.ROWS:
        if K.family(r) != fam or r.entry not in ("minimizers", "hash_sample"):
            continue
        for label, seq, offs, read_len in K.inputs(r):
            want = O.minimizers(seq, offs, r.unit, r.w, K.SEED, bool(r.canonical))
            got = K.range_minimizers(seq, offs, r.unit, r.w, r.canonical, 0, 0)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(want[0]) > 50, (K.row_id(r), label)


@pytest.mark.parametrize("fam", K.FAMILIES)
def test_emulation_of_every_row(emu, fam):
    for r in K.ROWS:
        if K.family(r) != fam or r.entry == "records128":  # (the 32-byte record's emulation: test_emu_records128.py)
            continue
        for label, seq, offs, read_len in K.inputs(r):
            got, frl = emu_scan(emu, r, seq, offs, read_len)
            want = K.expected(r, seq, offs, read_len)
            assert want["count"] > (20 if r.entry != "hash_sample" else 5), (K.row_id(r), label)
            K.assert_same(r.entry, got, want, (K.row_id(r), label))
            assert frl == (1 if r.read_len else 0)  # (the emulation has no position_tiled switch: that row runs read-tiled here)
        label, seq, offs, read_len, first, n = K.sub_range(r)
        got, _ = emu_scan(emu, r, seq, offs, read_len, first, n)
        K.assert_same(r.entry, got, K.expected(r, seq, offs, read_len, first, n), (K.row_id(r), label, first, n))


# ----------------------------------------------------------------------------- every fixed read length

def test_the_read_lengths_reach_every_plan():
    """every lanes-per-read count 1..64 in the planner's arithmetic (and the reciprocal lpr_inv exact for every lane at each accepted one), 14 / 15 / 16
    units per lane for canonical (31, 11) and 16 for the rest, a length where the LDS cap lowers the reads per wave, lengths on either side of the
    efficiency switch"""
    seen = K.assert_plan_coverage()
    assert seen["reached"] == 64
    print(seen)
    for shape in K.LENGTH_SHAPES:
        assert sorted(L for b in range(K.LENGTH_BLOCKS) for L in K.length_block(shape, b)) == K.lengths_of(shape)
        assert K.lengths_of(shape)[0] == shape[1] + shape[2] - 1
    assert K.lengths_of(K.LENGTH_SHAPES[0])[-1] == 1054 + K.BEYOND  # 31-mers: 1024 units on 64 lanes


@pytest.mark.parametrize("block", range(K.LENGTH_BLOCKS))
@pytest.mark.parametrize("shape", K.LENGTH_SHAPES, ids=K.P.ids)
def test_emulation_at_every_read_length(emu, shape, block):
    taken = 0
    for L in K.length_block(shape, block):
        r = K.length_row(shape, L)
        seq, offs, read_len, g = K.length_input(shape, L)
        got, frl = emu_scan(emu, r, seq, offs, read_len)
        K.assert_same(r.entry, got, K.expected(r, seq, offs, read_len), (shape, L))
        assert frl == (1 if g else 0), (shape, L)
        taken += frl
    assert taken > 10
