"""Pass 2 of the 64-bit scans against output arrays with guard words behind them.  emit_tile stores a tile's records without a per-record test when
the whole tile fits the capacity (`fits`) and with one when it does not; minimizer scans take four tiles per workgroup.  Through the C ABI, every
output array followed by sentinel words:
    entry points   bl_scan_minimizers, bl_scan_hash_sample, bl_scan_super_kmers (its two uint8 arrays included), bl_scan_super_kmer_records,
                   bl_scan_syncmers
    layouts        a contig of three tiles and a partial one (the generic pass 2); 150-bp reads, six tiles (canonical (31, 11) minimizers: the
                   C3 record kernel)
    capacities     need, need - 1, 0 with arrays, a value inside tile 1 (the second tile of a minimizer workgroup), the record offset of tile 2
                   (tile 1 fits to the last slot, tile 2 not at all) and one below it, and, on the reads, a value inside tile 5 (the second
                   tile of the second minimizer workgroup)
    checks         the return code (BL_ERR_CAPACITY when short) and the full count; the full digest; the first min(capacity, need) records are
                   the oracle's; every word behind them is still the sentinel; with any one array NULL the others hold the same"""
import ctypes as C

import numpy as np
import pytest

import kernel_cases as K
import oracle_lib as O
import superkmer_model as SM
import tie_plant as P

pytestmark = pytest.mark.gpu

GUARD = 1024
SENT64, SENT8 = 0x5A5A5A5A5A5A5A5A, 0xA5
# entry point -> [(array, words per record, bytes per word)]
ARRAYS = {
    "minimizers": [("values", 1, 8), ("positions", 1, 8), ("hashes", 1, 8)],
    "hash_sample": [("values", 1, 8), ("positions", 1, 8), ("hashes", 1, 8)],
    "super_kmers": [("minimizers", 1, 8), ("first_pos", 1, 8), ("mm_pos", 1, 1), ("sizes", 1, 1), ("hashes", 1, 8)],
    "super_kmer_records": [("records", 2, 8), ("hashes", 1, 8)],
    "syncmers": [("positions", 1, 8)],
}
# (entry, unit, w, canonical, syncmer offsets, layout, pass-2 kernel)
CASES = [
    ("minimizers", 21, 9, 1, None, "contig", "emit<MM>"),
    ("hash_sample", 27, 1, 0, None, "contig", "emit<MM>"),
    ("super_kmers", 19, 12, 1, None, "contig", "emit<SK>"),
    ("super_kmer_records", 19, 12, 0, None, "contig", "emit<SK>"),
    ("syncmers", 11, 21, 1, (0, 20), "contig", "emit<SY>"),
    ("minimizers", 31, 11, 1, None, "reads150", "emit<MM,C3>"),
    ("hash_sample", 27, 1, 1, None, "reads150", "emit<MM>"),
    ("super_kmers", 25, 17, 1, None, "reads150", "emit<SK>"),
    ("super_kmer_records", 15, 17, 0, None, "reads150", "emit<SK>"),  # k = 31 (a 16-byte record holds k <= 32), read-tiled like the case above
    ("syncmers", 11, 21, 1, (3, 9), "reads150", "emit<SY>"),
]


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def reads150():
    """six read-tiled tiles of the (31, 11) and the w = 17 plans: five full ones and three reads"""
    g = P.plan_frl(P.MODE_MINIMIZER, 150 * 1000, 150, 31, 11, 1)
    n = (5 * g["reads_per_tile"] + 3) * 150
    seq = O.synth(4150, n)
    seq[np.random.default_rng(150).integers(0, n, 9)] = ord("N")
    return seq, O.fixed_offsets(n, 150), 150


def want_of(case, seq, offs, read_len):
    """({array: expected}, digest, the window (k-mer) that starts each record)"""
    entry, unit, w, canonical, offsets, layout, _ = case
    row = K._row(("?",), "super_kmers" if entry == "super_kmer_records" else entry, unit, w, canonical, offsets=offsets)
    x = K.expected(row, seq, offs, read_len)
    if entry in ("minimizers", "hash_sample"):
        mn, fp, mp, _, hs = O.super_kmers(seq, offs, unit + w - 1, unit, K.SEED, bool(canonical))
        starts = fp[hs < np.uint64(K.THRESHOLD)] if entry == "hash_sample" else fp
        assert np.array_equal(x["positions"], (fp + mp)[hs < np.uint64(K.THRESHOLD)] if entry == "hash_sample" else fp + mp)
    elif entry == "syncmers":
        starts = x["positions"]
    else:
        starts = x["first_pos"]
    if entry == "super_kmer_records":
        recs = SM.pack(seq, x["first_pos"].astype(np.int64), x["sizes"].astype(np.int64), unit + w - 1, x["mm_pos"].astype(np.int64))
        x = dict(records=recs, hashes=x["hashes"], count=x["count"], xor_hash=x["xor_hash"], aux=x["aux"])
    return x, starts.astype(np.int64)


def tile_offsets(case, seq, read_len, starts):
    """record offset of every tile: the tile that builds a record is the one whose positions hold the owner of its first window (tie_plant's plans)"""
    entry, unit, w, canonical, offsets, layout, _ = case
    mode = K.MODE.get(entry, P.MODE_SUPERKMER)
    g = P.plan_frl(mode, len(seq), read_len, unit, w, canonical) if read_len and entry != "hash_sample" else None
    if g:
        tile = starts // g["stride"]
    else:
        g = P.plan_pos(mode, 0, len(seq), w)
        tile = (starts - (0 if mode == P.MODE_SYNCMER else 1) - g["origin"]) // g["stride"]
    assert tile.min() == 0 and tile.max() == g["n_tiles"] - 1 and np.all(np.diff(tile) >= 0)
    cnt = np.bincount(tile, minlength=g["n_tiles"])
    return np.concatenate([[0], np.cumsum(cnt)]), cnt


def raw(ctx, batch, case, capacity, null=None):
    """one call through the C ABI, sentinels in and behind every array: (rc, Result, {array: host copy of the WHOLE buffer})"""
    import torch

    import biolib_amd as B
    from biolib_amd import capi

    entry, unit, w, canonical, offsets, _, _ = case
    bufs = {}
    for name, words, size in ARRAYS[entry]:
        if size == 8:
            bufs[name] = torch.full((words * capacity + GUARD,), SENT64, dtype=torch.int64, device="cuda")
        else:
            bufs[name] = torch.full((capacity + GUARD,), SENT8, dtype=torch.uint8, device="cuda")
    ptr = [None if null in (name, "all") else C.c_void_p(bufs[name].data_ptr()) for name, _, _ in ARRAYS[entry]]
    flags = (B.FLAG_CANONICAL if canonical else 0) | B.FLAG_SYNC
    res = capi.Result()
    L, k = capi.lib(), unit + w - 1
    if entry == "minimizers":
        rc = L.bl_scan_minimizers(ctx._h, batch._h, 0, 0, unit, w, K.SEED, flags, *ptr, capacity, C.byref(res))
    elif entry == "hash_sample":
        rc = L.bl_scan_hash_sample(ctx._h, batch._h, 0, 0, unit, K.SEED, K.THRESHOLD, flags, *ptr, capacity, C.byref(res))
    elif entry == "super_kmers":
        rc = L.bl_scan_super_kmers(ctx._h, batch._h, 0, 0, k, unit, K.SEED, flags, *ptr, capacity, C.byref(res))
    elif entry == "super_kmer_records":
        rc = L.bl_scan_super_kmer_records(ctx._h, batch._h, 0, 0, k, unit, K.SEED, flags, *ptr, capacity, C.byref(res))
    else:
        rc = L.bl_scan_syncmers(ctx._h, batch._h, 0, 0, k, unit, offsets[0], offsets[1], 0, flags, *ptr, capacity, C.byref(res))
    ctx.sync()
    torch.cuda.synchronize()
    host = {name: (t.cpu().numpy().view(np.uint64) if t.dtype == torch.int64 else t.cpu().numpy()) for name, t in bufs.items()}
    return rc, res, host


def check(case, want, need, capacity, rc, res, host, null, what):
    from biolib_amd import capi

    entry = case[0]
    assert rc == (capi.BL_OK if capacity >= need else capi.BL_ERR_CAPACITY) and int(res.count) == need, (what, rc, int(res.count), need)
    for d in K.DIGEST["super_kmers" if entry == "super_kmer_records" else entry]:
        if d in want:
            assert int(getattr(res, d)) == int(want[d]), (what, d)  # the digest is that of every record, stored or not
    kept = min(capacity, need)
    for name, words, size in ARRAYS[entry]:
        a, sent = host[name], np.uint64(SENT64) if size == 8 else np.uint8(SENT8)
        if name == null:
            assert np.all(a == sent), (what, name, "written though NULL was passed")
            continue
        behind = np.nonzero(a[words * kept:] != sent)[0]
        assert len(behind) == 0, (what, name, "written behind the records the capacity allows: record", kept + int(behind[0]) // words)
        x = want[name].reshape(-1)[:words * kept]
        assert np.array_equal(a[:words * kept].astype(x.dtype), x), (what, name, "the records below the capacity")


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[5]}")
def test_capacity_guard(ctx, case):
    entry, unit, w, canonical, offsets, layout, emit = case
    seq, offs, read_len = reads150() if layout == "reads150" else K.contig(K.MODE.get(entry, P.MODE_SUPERKMER), w)[:3]
    want, starts = want_of(case, seq, offs, read_len)
    need = want["count"]
    base, cnt = tile_offsets(case, seq, read_len, starts)
    assert len(cnt) >= (6 if layout == "reads150" else 4) and cnt[1] > 8 and cnt[2] > 8
    caps = {need, need - 1, 0, int(base[1] + cnt[1] // 2), int(base[2]), int(base[2]) - 1}
    if len(cnt) >= 6:
        caps.add(int(base[5] + cnt[5] // 2))
    batch = ctx.upload(seq, read_len=read_len) if read_len else ctx.upload(seq, offsets=offs)
    try:
        for capacity in sorted(caps):
            rc, res, host = raw(ctx, batch, case, capacity)
            names = ctx.last_scan_kernels()
            assert names[-1] == emit, (case, names)
            check(case, want, need, capacity, rc, res, host, None, (case, "capacity", capacity, "of", need))
        for capacity in (need, int(base[1] + cnt[1] // 2)):
            for null, _, _ in ARRAYS[entry]:
                if len(ARRAYS[entry]) == 1:
                    continue  # (one array: without it the call is a count, below)
                rc, res, host = raw(ctx, batch, case, capacity, null=null)
                check(case, want, need, capacity, rc, res, host, null, (case, "capacity", capacity, "without", null))
        # no array at all: a count, whatever the capacity says
        from biolib_amd import capi

        rc, res, host = raw(ctx, batch, case, 0, null="all")
        assert rc == capi.BL_OK and int(res.count) == need
        assert all(np.all(a == (np.uint64(SENT64) if a.dtype == np.uint64 else np.uint8(SENT8))) for a in host.values())
    finally:
        batch.close()
