"""bl_pack_super_kmers128 / bl_partition_records128 / bl_expand_super_kmers128 / bl_count_super_kmers128 on the GPU, bit-exact against
the plain model of tests/superkmer128_model.py (checked on the CPU by tests/test_superkmer128_model.py and, for the kernels' own
per-thread bodies, by tests/test_emu_superkmer128.py).

The counter's directed cases are single buckets built ON the limits the model reads from the kernel sources, and every one asserts on
the model that it sits there before the GPU sees it.  All calls go through the C ABI, so that the capacity is the exact need (or one
less, or nothing) and the output pointers may be NULL; 4,096 sentinel entries behind every output array must stay as they were."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmers128_model as K
import oracle_lib as O
import superkmer128_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
KEY_SENT = 0xA5A5A5A5A5A5A5A5
CNT_SENT = 0x5A5A5A5A
SEED = 7
EDGE_BASES = (1, 32, 33, 64, 65, 96, 97, 122)


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lim():
    return M.limits()


def _to_device(a):
    import torch

    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


def _guarded(n, sentinel, dtype):
    """n + GUARD entries, all the sentinel: the first n are the output array, the rest must not be touched"""
    import torch

    bits = 64 if dtype == torch.int64 else 32
    signed = sentinel - (1 << bits) if sentinel >> (bits - 1) else sentinel
    return torch.full((int(n) + GUARD,), signed, dtype=dtype, device="cuda")


def _count_call(ctx, recs_t, n, k, m, canon, capacity, keys=True, counts=True):
    """one bl_count_super_kmers128: (rc, n_distinct, keys as Python ints [capacity], counts [capacity]) after the guards were checked"""
    import torch

    import biolib_amd as B
    from biolib_amd import capi

    kt, ct = _guarded(2 * capacity, KEY_SENT, torch.int64), _guarded(capacity, CNT_SENT, torch.int32)
    need = C.c_uint64(12345)
    rc = capi.lib().bl_count_super_kmers128(ctx._h, C.c_void_p(recs_t.data_ptr()) if n else None, n, k, m, SEED, B.FLAG_CANONICAL if canon else 0,
                                            C.c_void_p(kt.data_ptr()) if keys else None, C.c_void_p(ct.data_ptr()) if counts else None, capacity, C.byref(need))
    ctx.sync()
    torch.cuda.synchronize()
    hk, hc = kt.cpu().numpy().view(np.uint64), ct.cpu().numpy().view(np.uint32)
    assert np.all(hk[2 * capacity:] == np.uint64(KEY_SENT)) and np.all(hc[capacity:] == np.uint32(CNT_SENT)), "written behind the capacity"
    if not (keys and counts) or rc != capi.BL_OK:
        assert np.all(hk == np.uint64(KEY_SENT)) and np.all(hc == np.uint32(CNT_SENT)), "a call that does not deliver wrote k-mers"
    return rc, int(need.value), hk[:2 * capacity].reshape(-1, 2), hc[:capacity]


def _as_dict(hk, hc, need):
    keys = M.from_words(hk[:need])
    out = dict(zip(keys, hc[:need].tolist()))
    assert len(out) == need, "one k-mer delivered twice"
    return out, keys


def _check_counts(ctx, recs, k, m, canon, expected, what, tight=True):
    """the whole contract on one input: count-only, capacity == need (content), a generous capacity (content), need - 1, 0, one NULL"""
    from biolib_amd import capi

    need, n = len(expected), len(recs)
    recs_t = _to_device(recs) if n else None
    rc, got, _, _ = _count_call(ctx, recs_t, n, k, m, canon, 0, keys=False, counts=False)
    assert (rc, got) == ((capi.BL_ERR_CAPACITY if need else capi.BL_OK), need), (what, "count only", rc, got, need)
    keys = []
    for cap in (need, need + 1000):
        rc, got, hk, hc = _count_call(ctx, recs_t, n, k, m, canon, cap)
        assert (rc, got) == (capi.BL_OK, need), (what, "capacity", cap, rc, got, need)
        delivered, keys = _as_dict(hk, hc, need)
        assert delivered == expected, (what, "capacity", cap)
    if tight and need:
        for cap in sorted({need - 1, 0}):
            rc, got, _, _ = _count_call(ctx, recs_t, n, k, m, canon, cap)
            assert (rc, got) == (capi.BL_ERR_CAPACITY, need), (what, "capacity", cap, rc, got, need)
        for kk, cc in ((False, True), (True, False)):  # one pointer NULL is a count-only call as well
            rc, got, _, _ = _count_call(ctx, recs_t, n, k, m, canon, need, keys=kk, counts=cc)
            assert (rc, got) == (capi.BL_ERR_CAPACITY, need), (what, "one NULL pointer", rc, got, need)
    return keys  # as written with the generous capacity: the order tells which path wrote them


def _run_cases(ctx, lim, cases):
    for case in cases:
        fate = M.check_case(case, lim)  # the case sits where it says: asserted on the model, never skipped
        expected = M.expected_counts(case["records"], case["k"], case["canonical"])
        assert len(expected) == fate["distinct"]
        written = _check_counts(ctx, case["records"], case["k"], case["m"], case["canonical"], expected,
                                (case["name"], fate["path"], "rounds", fate["rounds"][:6], "held", fate["held"][-3:], "totals", fate["totals"][-3:]))
        # which path counted the bucket shows in the order of the output (both being exact, the edges would otherwise be invisible):
        # the sort path writes its keys ascending, a table in slot order, which for 16 or more keys is ascending with a chance < 1 / 16!
        if len(written) >= 16:
            assert (written == sorted(written)) == (fate["path"] == "fallback"), (case["name"], fate["path"])


# ----------------------------------------------------------------------------- pack

@pytest.mark.parametrize("n_bases,origin", [(1000, 0), (1000, 10**12 + 7), (5, 0), (5, 10**12 + 7)])
def test_pack_clipping_matrix(ctx, n_bases, origin):
    import torch

    from biolib_amd import capi

    rng = np.random.default_rng(n_bases + origin % 1000)
    seq = rng.choice(np.frombuffer(b"ACGTacgtUu", np.uint8), n_bases)
    batch = ctx.upload(seq).set_origin(origin)
    wrap = lambda p: (origin + p) & M.M64 if p < 2**62 else (origin - (2**64 - p)) & M.M64
    for k, m in ((1, 1), (31, 15), (33, 32), (59, 5), (64, 32)):
        pos = [0, 1, n_bases - 1, n_bases, n_bases + 1, max(n_bases - 130, 0), max(n_bases - 64, 0), 2**64 - 1, 2**64 - k, 2**64 - 122, 2**63]
        fps, sizes = [], []
        for b in EDGE_BASES:
            if k <= b <= k + 63:
                for p in pos + [max(n_bases - b, 0), max(n_bases - b + 1, 0)]:
                    fps.append(wrap(p)); sizes.append(b - k + 1)
        fp, sz = np.array(fps, np.uint64), np.array(sizes, np.uint8)
        mp = rng.integers(0, 64, len(fp)).astype(np.uint8)
        n = len(fp)
        out = _guarded(4 * n, KEY_SENT, torch.int64)
        assert out.data_ptr() % 32 == 0
        fp_t, sz_t, mp_t = _to_device(fp), _to_device(sz), _to_device(mp)  # named: all three must be alive while the kernel reads them
        rc = capi.lib().bl_pack_super_kmers128(ctx._h, batch._h, C.c_void_p(fp_t.data_ptr()), C.c_void_p(sz_t.data_ptr()),
                                               C.c_void_p(mp_t.data_ptr()), n, k, m, C.c_void_p(out.data_ptr()))
        assert rc == capi.BL_OK
        ctx.sync()
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        assert np.all(got[4 * n:] == np.uint64(KEY_SENT)), "written behind the records"
        want = M.pack_clipped(seq, fp.tolist(), sz.tolist(), k, mp.tolist(), origin)
        got = got[:4 * n].reshape(-1, 4)
        assert np.array_equal(got, want), (k, np.nonzero((got != want).any(1))[0][:5])
        inside = want[:, :3].any(1) | ((want[:, 3] >> np.uint64(12)) != 0)
        assert inside.any() or n_bases < k
        assert not inside.all()  # and some are empty records
    batch.close()


# ----------------------------------------------------------------------------- expand

@pytest.mark.parametrize("canon", [False, True])
@pytest.mark.parametrize("k", [1, 32, 33, 48, 64])
def test_expand_hand_built_records(ctx, k, canon):
    import torch

    import biolib_amd as B
    from biolib_amd import capi

    rng = np.random.default_rng(64 * k + canon)
    lens = sorted({b for b in EDGE_BASES if k <= b <= k + 63} | {k, k + 1, k + 15, k + 16, k + 17, min(k + 63, 122)})
    strings = ["".join("ACGT"[c] for c in rng.integers(0, 4, b)) for b in lens] + ["T" * min(k + 63, 122), "A" * k]
    recs = M.records_from_bases(strings, k, [int(x) for x in rng.integers(0, 64, len(strings))])
    want = M.expand(recs, k, canon)
    need = len(want)
    recs_t = _to_device(recs)
    flags = B.FLAG_CANONICAL if canon else 0
    for cap in (need, need + 7, need - 1, 0):
        out = _guarded(2 * cap, KEY_SENT, torch.int64)
        got_n = C.c_uint64(999)
        rc = capi.lib().bl_expand_super_kmers128(ctx._h, C.c_void_p(recs_t.data_ptr()), len(recs), k, flags, C.c_void_p(out.data_ptr()), cap, C.byref(got_n))
        ctx.sync()
        torch.cuda.synchronize()
        host = out.cpu().numpy().view(np.uint64)
        assert got_n.value == need
        assert np.all(host[2 * cap:] == np.uint64(KEY_SENT)), "written behind the capacity"
        if cap >= need:
            assert rc == capi.BL_OK and M.from_words(host[:2 * need]) == want
        else:
            assert rc == capi.BL_ERR_CAPACITY and np.all(host == np.uint64(KEY_SENT))
    got = ctx.expand_super_kmers128(recs_t, k, canonical=canon)
    assert M.from_words(got.cpu().numpy()) == want


# ----------------------------------------------------------------------------- count

def test_count_tiny_inputs(ctx):
    k, m = 40, 5
    s = "GATTC" + "ACGGTCATGCAAGTCTAGCATCGATCGGATCTAGCTAGGATCCATCGAT"
    cases = {
        "no record": np.zeros((0, 4), np.uint64),
        "one record, one k-mer": M.records_from_bases([s[:40]], k, 0),
        "one record": M.records_from_bases([s], k, 0),
        "one k-mer repeated": M.records_from_bases(["GATTC" + "A" * 98] + [s[:40]] * 5 + ["GATTC" + "A" * 35], k, 0),
        "two records sharing k-mers": M.records_from_bases([s[:50], s[:45]], k, 0),
    }
    for what, recs in cases.items():
        for canon in (False, True):
            M.assert_bucketable(recs, k, m, canon)
            _check_counts(ctx, recs, k, m, canon, M.expected_counts(recs, k, canon), what)


def test_count_round_limits(ctx, lim):
    _run_cases(ctx, lim, M.round_cases(lim))


def test_count_table_full_limits(ctx, lim):
    _run_cases(ctx, lim, M.full_cases(lim))


def test_count_probe_chains(ctx, lim):
    _run_cases(ctx, lim, M.probe_cases(lim))


def test_count_width_edge(ctx, lim):
    _run_cases(ctx, lim, M.count_width_cases(lim))


def test_count_poly_t_at_k_64_without_the_canonical_flag(ctx):
    recs = M.records_from_bases(["T" * 122, "T" * 64, "T" * 32 + "ACGT" * 8 + "T" * 32], 64, 0)
    M.assert_bucketable(recs, 64, 32, False)
    expected = M.expected_counts(recs, 64, False)
    assert expected[2**128 - 1] == 60 and len(expected) > 30
    for tables in (1, 0):
        ctx.set_option("count128_tables", tables)
        try:
            _check_counts(ctx, recs, 64, 32, False, expected, ("poly-T", tables))
        finally:
            ctx.set_option("count128_tables", 1)


def test_count_terminates_on_any_record_bits(ctx):
    """random words: size and mm_pos inconsistent with k and m, base bits where a record has none.  One k-mer may then sit under two
    minimizers (several partial counts), so only the total and the termination are checked, tables against the sort path"""
    rng = np.random.default_rng(11)
    recs = rng.integers(0, 1 << 64, (3000, 4), dtype=np.uint64, endpoint=False)
    recs_t = _to_device(recs)
    for k, m in ((64, 32), (33, 1)):
        n_kmers = sum(M.record_size(r) for r in recs)
        k1, c1 = ctx.count_super_kmers128(recs_t, k, m, seed=SEED, canonical=True)
        assert int(c1.sum().item()) == n_kmers
        ctx.set_option("count128_tables", 0)
        try:
            k0, c0 = ctx.count_super_kmers128(recs_t, k, m, seed=SEED, canonical=True)
        finally:
            ctx.set_option("count128_tables", 1)
        assert int(c0.sum().item()) == n_kmers and len(set(M.from_words(k0.cpu().numpy()))) == len(c0)
        assert set(M.from_words(k1.cpu().numpy())) == set(M.from_words(k0.cpu().numpy()))


# ----------------------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def reads():
    """~20 kbp of 150-bp reads with N's and a short read"""
    n = 150 * 134
    seq = O.synth(5, n)
    seq[np.random.default_rng(5).integers(0, n, 25)] = ord("N")
    offs = np.concatenate([np.arange(0, 150 * 60 + 1, 150), [150 * 60 + 40], np.arange(150 * 61 + 40, n, 150), [n]]).astype(np.uint64)
    return seq, np.unique(offs)


@pytest.mark.parametrize("k,m", [(33, 15), (51, 21), (64, 32)])
def test_end_to_end_counts_equal_a_counter_over_the_128_bit_scan(ctx, reads, k, m):
    import torch
    import torch.distributed as dist

    from biolib_amd import shard

    seq, offs = reads
    batch = ctx.upload(seq, offs)
    scan = batch.kmers128(k, seed=0, canonical=True)
    ok = scan["valid"] == 1
    want = collections.Counter(M.from_words(scan["values"][ok]))
    model = K.scan(seq.tobytes(), offs, k, 0, True)
    assert int(model["valid"].sum()) == int(ok.sum()) > 5000

    def as_counter(keys, cnts):
        out = dict(zip(M.from_words(keys.cpu().numpy()), cnts.cpu().tolist()))
        assert len(out) == len(cnts)
        return out

    keys, cnts = shard.count_kmers_via_super_kmers(ctx, batch, k, m, seed=SEED, canonical=True)
    assert keys.shape[1] == 2 and as_counter(keys, cnts) == want
    recs, hashes = batch.super_kmer_records128(k, m, seed=SEED, canonical=True)
    assert recs.shape[1] == 4 and len(recs) > 500
    if dist.is_available() and dist.is_initialized():
        keys, cnts = shard.count_kmers_via_super_kmers(ctx, batch, k, m, seed=SEED, canonical=True, force_exchange=True)
        assert as_counter(keys, cnts) == want
    # routing: three parts by minimizer hash, each holding its own records; the concatenation counts to the same
    bucketed, counts = ctx.partition_records128(hashes, recs, 3)
    assert sum(counts) == len(recs)
    h = hashes.cpu().numpy().view(np.uint64)
    assert counts == [int((h % np.uint64(3) == np.uint64(b)).sum()) for b in range(3)]
    rows = lambda t: sorted(map(tuple, t.cpu().numpy().view(np.uint64).tolist()))
    src = recs.cpu().numpy().view(np.uint64)
    at = 0
    for b in range(3):
        assert rows(bucketed[at:at + counts[b]]) == sorted(map(tuple, src[h % np.uint64(3) == np.uint64(b)].tolist()))
        at += counts[b]
    keys, cnts = ctx.count_super_kmers128(bucketed, k, m, seed=SEED, canonical=True)
    assert as_counter(keys, cnts) == want
    # the two paths against each other on the same records
    ctx.set_option("count128_tables", 0)
    try:
        k0, c0 = ctx.count_super_kmers128(recs, k, m, seed=SEED, canonical=True)
    finally:
        ctx.set_option("count128_tables", 1)
    k1, c1 = ctx.count_super_kmers128(recs, k, m, seed=SEED, canonical=True)
    assert sorted(as_counter(k0, c0).items()) == sorted(as_counter(k1, c1).items()) == sorted(want.items())
    assert M.from_words(k0.cpu().numpy()) == sorted(want)  # the sort path delivers ascending
    # the records themselves are the model's
    g = batch.super_kmers(k, m, seed=SEED, canonical=True)
    assert np.array_equal(src, M.pack(seq, g["first_pos"], g["sizes"], k, g["mm_pos"]))
    batch.close()
    torch.cuda.synchronize()


def test_small_shapes_keep_the_16_byte_path(ctx, reads):
    from biolib_amd import shard

    seq, offs = reads
    batch = ctx.upload(seq, offs)
    keys, cnts = shard.count_kmers_via_super_kmers(ctx, batch, 31, 15, seed=SEED, canonical=True)
    assert keys.dim() == 1 and len(keys) == len(cnts) > 5000
    keys, cnts = shard.count_kmers_via_super_kmers(ctx, batch, 32, 4, seed=SEED, canonical=True)  # 2k - m = 60: one base too many for 16 bytes
    assert keys.dim() == 2 and int((keys[:, 1] != 0).sum().item()) == 0
    batch.close()


# ----------------------------------------------------------------------------- argument errors

def test_argument_errors(ctx):
    import torch

    import biolib_amd as B
    from biolib_amd import capi

    L = capi.lib()
    recs = _to_device(M.records_from_bases(["ACGT" * 20], 40, 0).repeat(4, 0))
    out = torch.zeros(256, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(64, dtype=torch.int32, device="cuda")
    need = C.c_uint64()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    for k, m in ((65, 32), (64, 33), (40, 0), (20, 21), (64, 5), (0, 0)):  # k > 64, m > 32, m < 1, m > k, 2k - m > 122, k < 1
        rc = L.bl_count_super_kmers128(ctx._h, p(recs), 1, k, m, 0, 0, p(out), p(cnt), 8, C.byref(need))
        assert rc == capi.BL_ERR_INVALID, (k, m)
        assert b"2k - m <= 122" in L.bl_last_error() and b"k <= 64" in L.bl_last_error()
        batch = ctx.upload(np.frombuffer(b"ACGT" * 50, np.uint8))
        fp, sz = _to_device(np.zeros(1, np.uint64)), _to_device(np.ones(1, np.uint8))
        assert L.bl_pack_super_kmers128(ctx._h, batch._h, p(fp), p(sz), p(sz), 1, k, m, p(out)) == capi.BL_ERR_INVALID
        batch.close()
    assert L.bl_count_super_kmers128(ctx._h, p(recs), 1, 64, 6, 0, 0, p(out), p(cnt), 64, C.byref(need)) == capi.BL_OK  # 2k - m = 122, w = 59
    assert L.bl_expand_super_kmers128(ctx._h, p(recs), 1, 65, 0, p(out), 8, C.byref(need)) == capi.BL_ERR_INVALID
    assert L.bl_expand_super_kmers128(ctx._h, p(recs), 1, 0, 0, p(out), 8, C.byref(need)) == capi.BL_ERR_INVALID
    # misaligned arrays
    assert L.bl_count_super_kmers128(ctx._h, p(recs, 16), 1, 40, 5, 0, 0, p(out), p(cnt), 8, C.byref(need)) == capi.BL_ERR_INVALID
    assert L.bl_count_super_kmers128(ctx._h, p(recs), 1, 40, 5, 0, 0, p(out, 8), p(cnt), 8, C.byref(need)) == capi.BL_ERR_INVALID
    assert L.bl_expand_super_kmers128(ctx._h, p(recs, 8), 1, 40, 0, p(out), 8, C.byref(need)) == capi.BL_ERR_INVALID
    assert L.bl_expand_super_kmers128(ctx._h, p(recs), 1, 40, 0, p(out, 8), 8, C.byref(need)) == capi.BL_ERR_INVALID
    counts = (C.c_uint64 * 3)()
    assert L.bl_partition_records128(ctx._h, p(out), p(recs, 16), 1, 3, p(out), counts) == capi.BL_ERR_INVALID
    assert L.bl_partition_records128(ctx._h, p(out), p(recs), 1, 65, p(out), counts) == capi.BL_ERR_INVALID
    batch = ctx.upload(np.frombuffer(b"ACGT" * 50, np.uint8))
    fp, sz = _to_device(np.zeros(1, np.uint64)), _to_device(np.ones(1, np.uint8))
    assert L.bl_pack_super_kmers128(ctx._h, batch._h, p(fp), p(sz), p(sz), 1, 40, 5, p(out, 16)) == capi.BL_ERR_INVALID
    assert L.bl_pack_super_kmers128(ctx._h, batch._h, p(fp), p(sz), None, 1, 40, 5, p(out)) == capi.BL_ERR_INVALID
    batch.close()
    with pytest.raises(B.BiolibError):
        ctx.set_option("count128_tables", 2)
    # the 64-bit calls keep their limits
    assert L.bl_count_super_kmers(ctx._h, p(recs), 1, 33, 15, 0, 1, p(out), p(cnt), 8, C.byref(need)) == capi.BL_ERR_INVALID


# ----------------------------------------------------------------------------- drop-in

def test_hash_sampler_drop_in_over_a_wide_view():
    lib = os.path.join(ROOT, "biolib_amd", "lib")
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_compat_hashsample128")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-pthread", "-I" + os.path.join(ROOT, "include", "compat"),
                           os.path.join(ROOT, "tests", "cpp", "test_compat_hashsample128.cpp"), "-L" + lib, "-lbiolib_amd", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe], timeout=600)
    seq = bytes(O.synth(3, 400)).decode()
    seq = seq[:170] + "N" + seq[171:]
    for k, canon, rate in ((33, 1, 0.5), (64, 0, 0.5), (64, 1, 1.0), (21, 1, 0.25)):
        out = subprocess.run([exe, seq, str(k), str(canon), repr(rate), "42"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "test_compat_hashsample128: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        got = [int(a) | (int(b) << 64) for a, b in (ln.split() for ln in out.stdout.splitlines()[:-1])]
        model = K.scan(seq.encode(), np.array([0, len(seq)], np.uint64), k, 42, bool(canon), drop_last=True)  # quirk Q1: the last k-mer is outside the range
        threshold = 2**64 - 1 if rate >= 1.0 else int(rate * float(2**64 - 1))
        rec = K.sample(model, threshold)
        want = [int(lo) | (int(hi) << 64) for lo, hi in zip(rec["lo"].tolist(), rec["hi"].tolist())]
        assert got == want and len(want) > 20, (k, canon, rate, len(got), len(want))
