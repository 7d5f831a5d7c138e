"""bl_pack_super_kmers / bl_expand_super_kmers / bl_count_super_kmers at their internal limits, bit-exact against the plain
model of tests/superkmer_model.py (checked on the CPU by tests/test_superkmer_model.py).

The counter's cases are single buckets built ON the limits the model reads from the kernel source — records and k-mers per
round, distinct k-mers per table, records per bucket, the 16 bits of a count, the wrap of the probe sequence — and every one
asserts on the model that it sits there before the GPU sees it.  All calls go through the C ABI, so that the capacity is the
exact need (or one less, or nothing) and the output pointers may be NULL; 4,096 sentinel entries behind both output arrays
must stay as they were.

What would go red (argued from bl_superkmer.hip, not run):

* pack_kernel's guards adding to the wrapped position again (`p + nb > n_bases`, `at + 8 <= n_bases`): for a position d bases in
  front of the origin with 1 <= d <= nb both sums wrap to small values, nb is kept and the 8-byte load starts d bytes in front
  of the batch — here the 'C's of the enclosing tensor, code 1.  test_pack_positions_... expects zero base bits at origin - 1
  (every shape), origin - k, origin - 59 (the 59-base shape) and at position 0 of a batch with an origin.
* `held + total >= CT_FULL` for `>`: the full_*_table cases (held + total == CT_FULL exactly) and chain_of_CT_FULL_wraps would
  take the sort path; their counts stay right, their keys come out ascending: the order assertion of _run_cases.
* CT_MAXREC raised by one: 2,041 x 32 still fits 16 bits, so no output changes (the static_assert stops 2,048);
  *_one_record_more and *_neighbour_makes_it_one_more are built from the constant and move with it.  The value itself is
  pinned by tests/test_superkmer_model.py::test_limits_are_all_found_and_as_documented.
* no `& (CT_SLOTS - 1)` in the probe loop: chain_of_CT_FULL_wraps and the cluster cases walk past slot 1,023 into the counts
  that follow the keys in LDS: wrong keys and counts.
* a round counting its 65th record (or dropping its 64th): recs_limit_plus_1, full_3_rounds_*, the probe chains (rounds of 64
  records of one k-mer each): a k-mer counted twice or not at all.
* put_counted ignoring `capacity`: every table case at capacity = need - 1 and 0 writes into the guard behind the arrays.
* fill_holes_kernel reading o.keys for ext_keys: the mixed reads at capacity == need fill their holes from behind the
  array (the guard's sentinel) instead of from the side buffer: wrong keys.
* append_counted_kernel without `base + i < capacity`: full_2_rounds_fallback (and every other fallback case) at need - 1 and 0.
* the count-only path forgetting the fallback's runs: the count-only call of every fallback case and of the mixed reads
  returns too small a need.
"""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib as O
import superkmer_model as M

pytestmark = pytest.mark.gpu

GUARD = 4096
KEY_SENT = 0xA5A5A5A5A5A5A5A5
CNT_SENT = 0x5A5A5A5A
SEED = 7


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

    signed = sentinel - (1 << (64 if dtype == torch.int64 else 32)) if sentinel >> (63 if dtype == torch.int64 else 31) else sentinel
    return torch.full((int(n) + GUARD,), signed, dtype=dtype, device="cuda")


def _count_call(ctx, recs_t, n, k, m, canon, capacity, keys=True, counts=True):
    """one bl_count_super_kmers: (rc, n_distinct, keys uint64 [capacity], counts [capacity]) after the guards were checked"""
    import torch

    import biolib_amd as B
    from biolib_amd import capi

    kt, ct = _guarded(capacity, KEY_SENT, torch.int64), _guarded(capacity, CNT_SENT, torch.int32)
    need = C.c_uint64(12345)
    rc = capi.lib().bl_count_super_kmers(ctx._h, C.c_void_p(recs_t.data_ptr()) if n else None, n, k, m, SEED, B.FLAG_CANONICAL if canon else 0,
                                         C.c_void_p(kt.data_ptr()) if keys else None, C.c_void_p(ct.data_ptr()) if counts else None, capacity, C.byref(need))
    ctx.sync()
    torch.cuda.synchronize()
    hk, hc = kt.cpu().numpy().view(np.uint64), ct.cpu().numpy().view(np.uint32)
    assert np.all(hk[capacity:] == np.uint64(KEY_SENT)) and np.all(hc[capacity:] == np.uint32(CNT_SENT)), "written behind the capacity"
    if not (keys and counts):
        assert np.all(hk == np.uint64(KEY_SENT)) and np.all(hc == np.uint32(CNT_SENT)), "a count-only call wrote k-mers"
    return rc, int(need.value), hk[:capacity], hc[:capacity]


def _sorted_pairs(keys, counts):
    order = np.argsort(keys, kind="stable")
    return keys[order], counts[order].astype(np.int64)


def _check_counts(ctx, recs, k, m, canon, expected, what, tight=True):
    """the whole contract on one input: count-only, capacity == need (content), a generous capacity (content), need - 1, 0"""
    from biolib_amd import capi

    eu, ec = expected
    need = len(eu)
    n = len(recs)
    recs_t = _to_device(recs) if n else None
    rc, got, _, _ = _count_call(ctx, recs_t, n, k, m, canon, 0, keys=False, counts=False)
    assert (rc, got) == ((capi.BL_ERR_CAPACITY if need else capi.BL_OK), need), (what, "count only", rc, got, need)
    for cap in (need, need + 1000):
        rc, got, hk, hc = _count_call(ctx, recs_t, n, k, m, canon, cap)
        assert (rc, got) == (capi.BL_OK, need), (what, "capacity", cap, rc, got, need)
        gu, gc = _sorted_pairs(hk[:need], hc[:need])
        assert np.array_equal(gu, eu), (what, "keys at capacity", cap)
        assert np.array_equal(gc, ec), (what, "counts at capacity", cap, gu[gc != ec][:4], gc[gc != ec][:4], ec[gc != ec][:4])
    if tight and need:
        for cap in sorted({need - 1, 0}):
            rc, got, _, _ = _count_call(ctx, recs_t, n, k, m, canon, cap)
            assert (rc, got) == (capi.BL_ERR_CAPACITY, need), (what, "capacity", cap, rc, got, need)
        for keys, counts in ((False, True), (True, False)):  # one pointer NULL is a count-only call as well
            rc, got, _, _ = _count_call(ctx, recs_t, n, k, m, canon, need, keys=keys, counts=counts)
            assert (rc, got) == (capi.BL_ERR_CAPACITY, need), (what, "one NULL pointer", rc, got, need)
    return hk[:need]  # as written with the generous capacity: the order tells which path wrote them


def _run_cases(ctx, lim, cases):
    for case in cases:
        fate = M.check_case(case, lim)  # the case sits where it says: asserted on the model, never skipped
        expected = M.expected_counts(case["records"], case["k"], case["canonical"])
        assert len(expected[0]) == fate["distinct"]
        t0 = time.time()
        written = _check_counts(ctx, case["records"], case["k"], case["m"], case["canonical"], expected,
                                (case["name"], fate["path"], "rounds", fate["rounds"][:6], "held", fate["held"][-3:], "totals", fate["totals"][-3:]))
        # Which path counted the bucket shows in the order of the output (an internal, pinned here on purpose: the edges would
        # otherwise be invisible, both paths being exact): the sort path writes its keys ascending, a table writes them in slot
        # order, which for 16 or more keys is ascending with a chance below 1 / 16!.
        if fate["distinct"] >= 16:
            ascending = bool(np.all(written[1:] > written[:-1]))
            assert ascending == (fate["path"] == "fallback"), (case["name"], "expected the", fate["path"], "path; keys ascending:", ascending)
        print(f"{case['name']}: {len(case['records'])} records, {len(fate['rounds'])} rounds, {fate['distinct']} distinct, {fate['path']}, "
              f"{M.n_buckets(len(case['records']), lim)} buckets, {time.time() - t0:.2f} s")


# ----------------------------------------------------------------------------- pack

PACK_SHAPES = [(1, 1, 1), (5, 4, 3), (31, 1, 15), (32, 1, 5), (28, 6, 5), (28, 32, 5)]  # (k, size, m): 1, 8, 31, 32, 33, 59 bases


@pytest.mark.parametrize("origin", [0, 10**12 + 7])
@pytest.mark.parametrize("n_bases", [1000, 5])
def test_pack_positions_in_front_of_behind_and_across_the_batch(ctx, origin, n_bases):
    """The batch is a SLICE of a larger device tensor of 'C's, so that a read in front of it (what the kernel did for a position
    1 .. nb bases in front of the origin while its guards added to the wrapped position) stays inside one allocation and shows
    as non-zero base bits.  Empty = all base bits zero with mm_pos and size - 1 kept; a record across the end is cut there."""
    import torch

    from biolib_amd import capi

    rng = np.random.default_rng(n_bases + (origin & 0xFF))
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_bases)]
    if n_bases >= 8:
        seq[:8] = np.frombuffer(b"GTCAGTCA", np.uint8)  # no code-0 base where a shifted read would land
    big = torch.full((4096 + n_bases + 4096,), ord("C"), dtype=torch.uint8, device="cuda")
    big[4096:4096 + n_bases] = torch.from_numpy(seq.copy()).cuda()
    batch = ctx.from_tensor(big[4096:4096 + n_bases])
    if origin:
        batch.set_origin(origin)
    assert sorted(s + k - 1 for k, s, _ in PACK_SHAPES) == [1, 8, 31, 32, 33, 59]
    for k, size, m in PACK_SHAPES:
        nb = size + k - 1
        empty = [-1, -k, -59, -60, n_bases] + ([-origin] if origin else [])
        cut = [n_bases - 1, n_bases - (nb - 1)]
        whole = [n_bases - nb]
        edges = empty + cut + whole
        rel, sizes = [], []
        for rep in range(40):  # ordinary groups between the edge ones: neighbouring threads take different exits
            for e in edges:
                s = int(rng.integers(1, min(32, 60 - k) + 1))
                if n_bases >= s + k - 1:
                    rel.append(int(rng.integers(0, n_bases - (s + k - 1) + 1)))
                    sizes.append(s)
                rel.append(e)
                sizes.append(size)
        first_pos = np.array([(origin + r) & M.M64 for r in rel], np.uint64)
        sizes = np.array(sizes, np.uint8)
        mm_pos = rng.integers(0, 32, len(rel)).astype(np.uint8)
        out = torch.full((len(rel), 2), -1, dtype=torch.int64, device="cuda")
        fp_t, sz_t, mp_t = _to_device(first_pos), _to_device(sizes), _to_device(mm_pos)
        capi.check(capi.lib().bl_pack_super_kmers(ctx._h, batch._h, C.c_void_p(fp_t.data_ptr()), C.c_void_p(sz_t.data_ptr()), C.c_void_p(mp_t.data_ptr()),
                                                  len(rel), k, m, C.c_void_p(out.data_ptr())))
        ctx.sync()
        got = out.cpu().numpy().view(np.uint64)
        exp = M.pack_clipped(seq, first_pos, sizes, k, mm_pos, origin)
        rel = np.array(rel, dtype=object)
        for g in np.nonzero((got != exp).any(axis=1))[0][:5]:
            print("k", k, "rel", rel[g], "size", sizes[g], "got", [hex(int(v)) for v in got[g]], "expected", [hex(int(v)) for v in exp[g]])
        assert np.array_equal(got, exp), (k, size, origin, n_bases)
        # the same, spelled out: the low ten bits always as given; nothing but zero bases in an empty record; whole records = pack()
        assert np.array_equal(got[:, 1] & np.uint64(0x3FF), (mm_pos.astype(np.uint64) << np.uint64(5)) | (sizes.astype(np.uint64) - np.uint64(1)))
        outside = np.array([r < 0 or r >= n_bases for r in rel])
        assert outside.sum() >= 40 * len(empty)
        assert np.all(got[outside, 0] == 0) and np.all(got[outside, 1] >> np.uint64(10) == 0)
        inside = np.array([0 <= r and r + int(s) + k - 1 <= n_bases for r, s in zip(rel, sizes)])
        if n_bases >= nb:
            assert inside.sum() >= 40 and (n_bases - nb) in set(rel[inside].tolist())
        if inside.any():
            idx = np.nonzero(inside)[0]
            assert np.array_equal(got[idx], M.pack(seq, np.array([rel[i] for i in idx], np.int64), sizes[idx], k, mm_pos[idx]))
        if n_bases >= nb > 1:  # cut records exist and are neither empty nor whole
            straddle = np.array([0 <= r < n_bases and r + int(s) + k - 1 > n_bases for r, s in zip(rel, sizes)])
            assert straddle.sum() >= 40
    batch.close()


# ----------------------------------------------------------------------------- expand

@pytest.mark.parametrize("k", [1, 5, 28, 32])
@pytest.mark.parametrize("canon", [False, True])
def test_expand_hand_built_records_with_a_tight_capacity(ctx, k, canon):
    import torch

    import biolib_amd as B
    from biolib_amd import capi

    rng = np.random.default_rng(k)
    top = min(32, M.MAX_BASES - k + 1)
    sizes = [1, top] * 150 + [int(s) for s in rng.integers(1, top + 1, 300)] + [top, 1]
    strings = ["".join("ACGT"[c] for c in rng.integers(0, 4, s + k - 1)) for s in sizes]
    strings[3], strings[4] = "T" * (top + k - 1), "A" * k
    recs = M.records_from_bases(strings, k, rng.integers(0, 32, len(strings)).tolist())
    exp = M.expand(recs, k, canon)
    need = len(exp)
    assert need == sum(sizes) and M.record_size(recs[1]) == top
    recs_t = _to_device(recs)
    flags = B.FLAG_CANONICAL if canon else 0
    for cap, want in ((need, capi.BL_OK), (need + 77, capi.BL_OK), (need - 1, capi.BL_ERR_CAPACITY), (0, capi.BL_ERR_CAPACITY)):
        out = _guarded(cap, KEY_SENT, torch.int64)
        got = C.c_uint64(1)
        rc = capi.lib().bl_expand_super_kmers(ctx._h, C.c_void_p(recs_t.data_ptr()), len(recs), k, flags, C.c_void_p(out.data_ptr()), cap, C.byref(got))
        ctx.sync()
        host = out.cpu().numpy().view(np.uint64)
        assert (rc, got.value) == (want, need), (k, canon, cap)
        assert np.all(host[cap:] == np.uint64(KEY_SENT)), "written behind the capacity"
        if want == capi.BL_OK:
            assert np.array_equal(host[:need], exp), (k, canon, cap)
            assert np.all(host[need:cap] == np.uint64(KEY_SENT))
        else:
            assert np.all(host == np.uint64(KEY_SENT)), "a refused call wrote k-mers"
    got = C.c_uint64(1)
    assert capi.lib().bl_expand_super_kmers(ctx._h, C.c_void_p(recs_t.data_ptr()), len(recs), k, flags, None, need, C.byref(got)) == capi.BL_ERR_CAPACITY and got.value == need
    assert capi.lib().bl_expand_super_kmers(ctx._h, None, 0, k, flags, None, 0, C.byref(got)) == capi.BL_OK and got.value == 0


# ----------------------------------------------------------------------------- count: tiny inputs

def _tiny_records(rng, n_rec, k, m, shared):
    """random records of sizes 1 and k - m + 1 (every fifth a copy of an earlier one); their minimizer at a random mm_pos of the
    first k-mer — one m-mer for all (`shared`: one bucket, the others empty) or whatever bases lie there"""
    top = k - m + 1
    strings, mps = [], []
    for i in range(n_rec):
        if i % 5 == 4:
            j = int(rng.integers(0, i))
            strings.append(strings[j])
            mps.append(mps[j])
            continue
        size = 1 if rng.integers(0, 2) else top
        s = "".join("ACGT"[c] for c in rng.integers(0, 4, size + k - 1))
        mp = int(rng.integers(0, k - m + 1))
        if shared:
            s = s[:mp] + M.CASE_MMER[:m].ljust(m, "G") + s[mp + m:]
        strings.append(s)
        mps.append(mp)
    return M.records_from_bases(strings, k, mps)


@pytest.mark.parametrize("k,m,canon,shared", [(5, 5, True, False), (5, 2, False, True), (21, 11, True, False), (31, 15, False, False), (31, 3, True, True),
                                              (32, 5, True, False)])
def test_count_tiny_inputs(ctx, lim, k, m, canon, shared):
    """one bucket and no sort up to 36 records, two buckets and one sort bit from 37, three from 73"""
    B = lim["BUCKET_RECS"]
    sizes = [1, 2, B, B + 1, 2 * B, 2 * B + 1]
    assert sizes == [1, 2, 36, 37, 72, 73] and [M.n_buckets(r, lim) for r in sizes] == [1, 1, 1, 2, 2, 3]
    for n_rec in sizes:
        recs = _tiny_records(np.random.default_rng(1000 * k + n_rec), n_rec, k, m, shared)
        M.assert_bucketable(recs, k, m, canon)
        assert {M.record_size(r) for r in recs} <= {1, k - m + 1}
        _check_counts(ctx, recs, k, m, canon, M.expected_counts(recs, k, canon), ("tiny", n_rec, k, m, canon))
    from biolib_amd import capi

    assert _count_call(ctx, None, 0, k, m, canon, 0, keys=False, counts=False)[:2] == (capi.BL_OK, 0)  # no records: nothing to ask for
    assert _count_call(ctx, None, 0, k, m, canon, 10)[:2] == (capi.BL_OK, 0)


# ----------------------------------------------------------------------------- count: directed buckets

def test_count_round_limits(ctx, lim):
    _run_cases(ctx, lim, M.round_cases(lim))


def test_count_table_full_limit(ctx, lim):
    _run_cases(ctx, lim, M.full_cases(lim))


def test_count_sixteen_bit_edge(ctx, lim):
    _run_cases(ctx, lim, M.sixteen_bit_cases(lim))


def test_count_probe_chains(ctx, lim):
    _run_cases(ctx, lim, M.probe_cases(lim))


# ----------------------------------------------------------------------------- count: capacity, NULL outputs, scratch reuse

def _mixed_reads():
    """~2 * 10^5 records: nine reads of ten are plain (their buckets stay in the tables), every tenth is of low complexity
    (thousands of records under one minimizer: the fallback runs beside the tables)"""
    k, m, L, n_reads = 31, 15, 150, 10_000
    seq = O.synth(97, n_reads * L)
    reads = seq.reshape(n_reads, L)
    low = [b"A", b"AC", b"T", b"ACG", b"A", b"T"]
    for i in range(0, n_reads, 10):
        unit = low[(i // 10) % len(low)]
        reads[i] = np.frombuffer((unit * L)[:L], np.uint8)
    return seq, O.fixed_offsets(seq.size, L), k, m


def test_count_capacity_and_null_outputs(ctx, lim):
    seq, offs, k, m = _mixed_reads()
    batch = ctx.upload(seq, offs)
    recs_t, _ = batch.super_kmer_records(k, m, seed=SEED, canonical=True)
    recs = recs_t.cpu().numpy().view(np.uint64)
    assert 150_000 < len(recs) < 250_000 and len(recs) == len(O.super_kmers(seq, offs, k, m, SEED, True)[0])
    vals, ok = O.units(seq, offs, k, True)
    eu, ec = np.unique(vals[ok != 0], return_counts=True)
    assert ec.max() > 0xFFFF, "no k-mer that only the fallback can count"
    assert (ec == 1).sum() > len(eu) // 2 and len(eu) > 64 * lim["CT_CHUNK"], "too few k-mers for holes and a side buffer"
    t0 = time.time()
    _check_counts(ctx, recs, k, m, True, (eu, ec.astype(np.int64)), "mixed reads")
    print(f"mixed reads: {len(recs)} records, {len(eu)} distinct, {time.time() - t0:.2f} s")
    # a large call, then a tiny one on the same context: the scratch arena is reused and must not leak into the answer
    tiny = _tiny_records(np.random.default_rng(5), 3, 21, 11, False)
    _check_counts(ctx, tiny, 21, 11, True, M.expected_counts(tiny, 21, True), "tiny after large")
    # and the directed buckets of both paths with every capacity
    names = {c["name"]: c for c in M.full_cases(lim)}
    for name in ("full_2_rounds_fallback", "full_2_rounds_table"):
        case = names[name]
        assert M.check_case(case, lim)["path"] == name.rsplit("_", 1)[1]
        _check_counts(ctx, case["records"], case["k"], case["m"], case["canonical"], M.expected_counts(case["records"], case["k"], case["canonical"]), name)
    batch.close()
