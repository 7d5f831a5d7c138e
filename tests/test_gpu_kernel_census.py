"""Every scan kernel the launchers of bl_kernels.hip can choose, launched at least once and held against the oracle.  One row of
tests/kernel_cases.py per kernel name the library lists (bl_scan_kernel_names); for every row:
    dispatch   after each call the context's recorded names (bl_ctx_last_scan_kernels) are exactly the row's
    records    every output array element for element, the count and the digest words, against oracle_lib
    inputs     (a) a contig with a repeat island across a tile border, (b) ragged reads with sequence starts planted at a tile and a wave border
               - 1, + 0, + 1, (b') N's at those places, or (c) two tiles and three reads of the row's read length; one sub-range whose first base
               is no multiple of 16 and whose end lies inside a tile
The last test of the module asserts that the names seen are the library's list, no more and no fewer: a launch site added without a row here, or
a row that stops reaching its kernel, fails there.  (The same rows and inputs through the CPU emulation: test_kernel_cases.py.)

Breaks tried on a scratch copy of the tree (library rebuilt, this module, test_gpu_read_lengths.py and test_gpu_capacity_guard.py run on an
MI355X; none committed) and the items that failed; without a break all 71 pass.
  the width-12 case launches the width-13 kernel and the reverse   test_kernel_census[MM_w9_16] and [SK_w9_16] (counts of the W = 12 rows), the
                                                                   closing test, test_capacity_guard's two w = 12 cases
  window_argmin's prefix minima take `<=` for `<` (leftmost tie)   9 of the 11 census families (all but MM_w2_8 and MM_w9_16, whose element-centric
                                                                   form does not come by there), the closing test, 22 of the 48 read-length items,
                                                                   2 capacity cases
  emit_store<MODE, true> refuses `g > capacity` only               all 10 test_capacity_guard cases ("written behind the records the capacity allows")"""
import ctypes as C

import numpy as np
import pytest

import kernel_cases as K

pytestmark = pytest.mark.gpu

SEEN = set()
FAMILIES_RUN = set()


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def scan(ctx, batch, r, first=0, n=0):
    """the row's scan through its entry point: what kernel_cases.assert_same compares"""
    import biolib_amd as B
    from biolib_amd import capi

    c, k = bool(r.canonical), r.unit + r.w - 1
    cap = batch.n_bases + 1  # (no second call for want of capacity: the names are those of the last scan)
    if r.entry == "minimizers":
        return batch.minimizers(r.unit, r.w, seed=K.SEED, canonical=c, first=first, n=n, capacity=cap)
    if r.entry == "hash_sample":
        return batch.hash_sample(r.unit, seed=K.SEED, threshold=K.THRESHOLD, canonical=c, first=first, n=n)
    if r.entry == "super_kmers":
        return batch.super_kmers(k, r.unit, seed=K.SEED, canonical=c, first=first, n=n, capacity=cap)
    if r.entry == "syncmers":
        return batch.syncmers(k, r.unit, r.offsets[0], r.offsets[1], seed=0, canonical=c, first=first, n=n, capacity=cap)
    recs, hs = ctx.empty_u64(4 * cap), ctx.empty_u64(cap)
    res = capi.Result()
    capi.check(capi.lib().bl_scan_super_kmer_records128(ctx._h, batch._h, first, n, k, r.unit, K.SEED, (B.FLAG_CANONICAL if c else 0) | B.FLAG_SYNC,
                                                        C.c_void_p(recs.data_ptr()), C.c_void_p(hs.data_ptr()), cap, C.byref(res)))
    cnt = int(res.count)
    out = res.as_dict()
    out.update(records=recs[:4 * cnt].cpu().numpy().view(np.uint64).reshape(-1, 4), hashes=hs[:cnt].cpu().numpy().view(np.uint64))
    return out


def run_row(ctx, r):
    jobs = [(label, seq, offs, read_len, 0, 0) for label, seq, offs, read_len in K.inputs(r)] + [K.sub_range(r)]
    try:
        ctx.set_exact_windows(r.exact)
        ctx.set_option("position_tiled", int(r.position_tiled))
        batches = {}
        for label, seq, offs, read_len, first, n in jobs:
            if label not in batches:
                batches[label] = ctx.upload(seq, read_len=read_len) if read_len else ctx.upload(seq, offsets=offs)
            got = scan(ctx, batches[label], r, first, n)
            names = tuple(ctx.last_scan_kernels())
            SEEN.update(names)
            what = (K.row_id(r), label, first, n)
            assert names == r.names, what
            want = K.expected(r, seq, offs, read_len, first, n)
            assert want["count"] > (20 if r.entry != "hash_sample" else 5), what
            K.assert_same(r.entry, got, want, what)
        for b in batches.values():
            b.close()
    finally:
        ctx.set_exact_windows(False)
        ctx.set_option("position_tiled", 0)


@pytest.mark.parametrize("fam", K.FAMILIES)
def test_kernel_census(ctx, fam):
    rows = [r for r in K.ROWS if K.family(r) == fam]
    assert rows
    for r in rows:
        run_row(ctx, r)
    FAMILIES_RUN.add(fam)


def test_kernel_census_an_empty_range_records_nothing(ctx):
    b = ctx.upload(K.contig(K.P.MODE_MINIMIZER, 7)[0])
    b.minimizers(21, 7, seed=K.SEED)
    assert ctx.last_scan_kernels() == ["count<MM,W=7>", "emit<MM>"]
    assert b.minimizers(21, 7, seed=K.SEED, first=100, n=0)["count"] > 0 and b.minimizers_raw(21, 7, K.SEED, 4, first=b.n_bases, n=0).count == 0
    assert ctx.last_scan_kernels() == []
    b.close()


def test_kernel_census_saw_every_name_the_library_lists(ctx):
    """runs last: needs every family of this module in the same session"""
    if FAMILIES_RUN != set(K.FAMILIES):
        pytest.fail(f"the census is whole only with every family run; missing {sorted(set(K.FAMILIES) - FAMILIES_RUN)}")
    listed = ctx.scan_kernel_names()
    assert len(listed) == len(set(listed))
    assert SEEN == set(listed), ("launched but not listed", sorted(SEEN - set(listed)), "listed but never launched", sorted(set(listed) - SEEN))
    print(f"\nkernel census: {len(SEEN)} kernels launched by {len(K.ROWS)} rows:", " ".join(sorted(SEEN)))
