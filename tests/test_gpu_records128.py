"""bl_scan_super_kmer_records128 on the GPU: the 32-byte super-k-mer record built inside the scan's record pass.  By contract its output
is what bl_scan_super_kmers + bl_pack_super_kmers128 give (Batch.super_kmer_records128(fused=False): the two calls as they were before
the fused one existed), so every comparison is whole arrays, bit for bit, against that path, and against the Python model
(superkmer128_model.pack over the oracle's groups) for the first few thousand records.  Shapes, batches and the ranges aimed at tile
edges are those of the CPU emulation test (tests/records128_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import records128_cases as R

pytestmark = pytest.mark.gpu

GUARD = 1024
REC_SENT, HASH_SENT = 0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C3C3C3C3C
MODEL_RECORDS = 4000
IDS = [f"k{k}-m{m}" for k, m in R.SHAPES]


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def _upload(ctx, seq, offs, read_len):
    return ctx.upload(seq, offs, read_len)


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _both(batch, k, m, canonical, first=0, n=0):
    """(fused records, hashes), (scan + pack records, hashes) as host arrays"""
    out = []
    for fused in (True, False):
        recs, hs = batch.super_kmer_records128(k, m, seed=R.SEED, canonical=canonical, first=first, n=n, fused=fused)
        out.append((_host(recs).reshape(-1, 4), _host(hs)))
    return out


def _same(a, b, what):
    assert len(a[0]) == len(b[0]) and len(a[1]) == len(b[1]), (what, len(a[0]), len(b[0]))
    bad = np.nonzero((a[0] != b[0]).any(1))[0]
    assert len(bad) == 0, (what, "first differing records", bad[:5].tolist(), [hex(int(x)) for x in a[0][bad[0]]], [hex(int(x)) for x in b[0][bad[0]]])
    assert np.array_equal(a[1], b[1]), what


def _raw(ctx, batch, k, m, canonical, first, n, capacity, records=True, hashes=True, offset=0):
    """one call through the C ABI with guard entries behind both arrays: (rc, count, records[capacity, 4], hashes[capacity]); asserts that
    nothing at or beyond `capacity` was written"""
    import torch

    import biolib_amd as B
    from biolib_amd import capi

    rt = torch.full((4 * capacity + GUARD,), REC_SENT, dtype=torch.int64, device="cuda")
    ht = torch.full((capacity + GUARD,), HASH_SENT, dtype=torch.int64, device="cuda")
    res = capi.Result()
    rc = capi.lib().bl_scan_super_kmer_records128(ctx._h, batch._h, first, n, k, m, R.SEED, (B.FLAG_CANONICAL if canonical else 0) | B.FLAG_SYNC,
                                                  C.c_void_p(rt.data_ptr() + offset) if records else None, C.c_void_p(ht.data_ptr()) if hashes else None,
                                                  capacity, C.byref(res))
    ctx.sync()
    torch.cuda.synchronize()
    hr, hh = _host(rt), _host(ht)
    assert np.all(hr[4 * capacity:] == np.uint64(REC_SENT)) and np.all(hh[capacity:] == np.uint64(HASH_SENT)), "written at or beyond the capacity"
    if not records:
        assert np.all(hr == np.uint64(REC_SENT))
    if not hashes:
        assert np.all(hh == np.uint64(HASH_SENT))
    return rc, int(res.count), hr[:4 * capacity].reshape(-1, 4), hh[:capacity]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,m", R.SHAPES, ids=IDS)
def test_layouts(ctx, k, m, canonical):
    """whole batches (a contig of a few tiles, ragged reads with N's, 150-bp reads, a batch shorter than a tile) and sub-ranges"""
    for name, make in R.LAYOUTS.items():
        seq, offs, read_len = make(k)
        exp = R.Expect(seq, offs, read_len, k, m, canonical)
        batch = _upload(ctx, seq, offs, read_len)
        n = len(seq)
        jobs = [(0, 0)] + ([(1234, 5000), (n - 122, 0)] if name == "contig" else []) + ([(150 * 7, 150 * 200)] if name == "reads150" else [])
        for first, cnt in jobs:
            fused, plain = _both(batch, k, m, canonical, first, cnt)
            _same(fused, plain, (name, first, cnt, "fused against scan + pack"))
            want = exp.of_range(first, cnt)
            assert len(fused[0]) == len(want[0]) > (0 if name == "short" or first else 100)
            _same((fused[0][:MODEL_RECORDS], fused[1][:MODEL_RECORDS]), (want[0][:MODEL_RECORDS], want[1][:MODEL_RECORDS]), (name, first, cnt, "fused against the model"))
        batch.close()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,m", R.SHAPES, ids=IDS)
def test_full_size_groups_at_the_last_positions_a_tile_owns(ctx, k, m, canonical):
    seq = O.synth(77 + k, R.BIG)
    exp = R.Expect(seq, None, 0, k, m, canonical)
    jobs = R.edge_jobs(exp, k, m)  # asserts, on the oracle's groups, that every pick has size == w and sits at its tile's edge
    assert len(jobs) == 4 * R.EDGE_PICKS
    batch = ctx.upload(seq)
    for first, n, placement, g in jobs:
        fused, plain = _both(batch, k, m, canonical, first, n)
        _same(fused, plain, (placement, first, n, "fused against scan + pack"))
        _same(fused, exp.of_range(first, n), (placement, first, n, "fused against the model"))
    batch.close()


def test_the_batch_origin_does_not_change_the_records(ctx):
    k, m = 51, 21
    seq, offs, read_len = R.ragged(k)
    a, b = ctx.upload(seq, offs), ctx.upload(seq, offs).set_origin(10**12 + 7)
    for canonical in (False, True):
        fa, _ = _both(a, k, m, canonical)
        fb, pb = _both(b, k, m, canonical, 0, 0)
        _same(fa, fb, "origin 0 against origin 10^12 + 7")
        _same(fb, pb, "fused against scan + pack at origin 10^12 + 7")
        fb, pb = _both(b, k, m, canonical, 3000, 9000)  # `first` counts inside the batch, whatever its origin
        _same(fb, pb, "a sub-range at origin 10^12 + 7")
        _same(fb, R.Expect(seq, offs, read_len, k, m, canonical).of_range(3000, 9000), "a sub-range against the model")
    a.close()
    b.close()


@pytest.mark.parametrize("k,m", [(51, 21), (31, 15)], ids=["k51-m21", "k31-m15"])
def test_capacity_and_null_outputs(ctx, k, m):
    from biolib_amd import capi

    seq, offs, read_len = R.reads150(k) if k == 31 else R.contig(k)  # (31, 15) on 150-bp reads: the read-tiled layout
    want = R.Expect(seq, offs, read_len, k, m, True).of_range()
    need = len(want[0])
    batch = _upload(ctx, seq, offs, read_len)
    rc, cnt, recs, hs = _raw(ctx, batch, k, m, True, 0, 0, need)
    assert (rc, cnt) == (capi.BL_OK, need)
    _same((recs, hs), want, "capacity == need")
    rc, cnt, recs, hs = _raw(ctx, batch, k, m, True, 0, 0, need - 1)
    assert (rc, cnt) == (capi.BL_ERR_CAPACITY, need)
    _same((recs, hs), (want[0][:need - 1], want[1][:need - 1]), "capacity == need - 1: the records below the capacity")
    rc, cnt, _, _ = _raw(ctx, batch, k, m, True, 0, 0, 0)
    assert (rc, cnt) == (capi.BL_ERR_CAPACITY, need)
    rc, cnt, _, _ = _raw(ctx, batch, k, m, True, 0, 0, need, records=False, hashes=False)  # count only
    assert (rc, cnt) == (capi.BL_OK, need)
    rc, cnt, recs, _ = _raw(ctx, batch, k, m, True, 0, 0, need, hashes=False)
    assert (rc, cnt) == (capi.BL_OK, need) and np.array_equal(recs, want[0])
    rc, cnt, _, hs = _raw(ctx, batch, k, m, True, 0, 0, need, records=False)
    assert (rc, cnt) == (capi.BL_OK, need) and np.array_equal(hs, want[1])
    batch.close()


def test_argument_errors(ctx):
    from biolib_amd import capi

    batch = ctx.upload(O.synth(1, 2000))
    for off in (8, 16, 24):
        rc, _, _, _ = _raw(ctx, batch, 51, 21, True, 0, 0, 64, offset=off)
        assert rc == capi.BL_ERR_INVALID and b"32-byte aligned" in capi.lib().bl_last_error(), off
    for k, m in ((64, 5), (64, 33), (65, 32), (65, 1), (40, 0), (20, 21)):  # 123 bases, m = 33, k = 65, w = 65, m < 1, m > k
        rc, _, _, _ = _raw(ctx, batch, k, m, True, 0, 0, 64)
        assert rc == capi.BL_ERR_INVALID, (k, m)
        msg = capi.lib().bl_last_error()
        assert b"m <= 32" in msg and b"k <= 64" in msg and b"k - m + 1 <= 64" in msg and b"2k - m <= 122" in msg, (k, m, msg)
    rc, cnt, _, _ = _raw(ctx, batch, 64, 6, True, 0, 0, 2000)  # 122 bases, w = 59: the limits themselves are allowed
    assert rc == capi.BL_OK and cnt > 10
    rc, cnt, _, _ = _raw(ctx, batch, 32, 32, True, 0, 0, 2000)  # k <= 32 is allowed
    assert rc == capi.BL_OK and cnt > 10
    batch.close()


@pytest.mark.parametrize("k,m", [(51, 21), (64, 32)], ids=["k51-m21", "k64-m32"])
def test_end_to_end_counts_on_fused_records(ctx, k, m):
    """Context.count_super_kmers128 on the fused records of ~1 Mbp = np.unique of the oracle's canonical k-mers"""
    n = 1_000_000
    seq = O.synth(900 + k, n)
    batch = ctx.upload(seq)
    recs, _ = batch.super_kmer_records128(k, m, seed=R.SEED, canonical=True)
    keys, cnts = ctx.count_super_kmers128(recs, k, m, seed=R.SEED, canonical=True)
    got = _host(keys).reshape(-1, 2)[:, ::-1]  # (low, high) -> (high, low)
    order = np.lexsort((got[:, 1], got[:, 0]))
    want_keys, want_cnts = R.unique_counts128(R.canonical_kmers128(seq, k))
    assert int(want_cnts.sum()) == n - k + 1 and len(want_keys) > 900_000
    assert np.array_equal(got[order], want_keys) and np.array_equal(cnts.cpu().numpy()[order].astype(np.int64), want_cnts)
    batch.close()
