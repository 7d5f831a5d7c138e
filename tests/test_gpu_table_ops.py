"""GPU tests of the count-table algebra (bl_table_combine / bl_table_filter and CountTable.union, intersect, subtract, subtract_counts,
filter, compare) against the dict model of table_ops_cases.py.  The cases are those of the host emulation (test_emu_table_ops.py),
where every index path ran under the sanitizers; nothing here is larger than a few tiles except one case of 2^20 + 2^20 keys."""
import ctypes as C

import numpy as np
import pytest

import lookup_cases as LC
import table_ops_cases as TC

pytestmark = pytest.mark.gpu
U32 = TC.U32
STATS = ("n_a_only", "n_b_only", "n_both", "n_out", "sum_min", "sum_max", "sum_out")
MODE_NAMES = {TC.SUM: "sum", TC.MIN: "min", TC.MAX: "max", TC.LEFT: "left", TC.RIGHT: "right"}


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.fixture()
def auto_prefix(ctx):
    yield
    ctx.set_option("table_prefix_bits", -1)


def dev_keys(keys, key_words):
    import torch

    return torch.from_numpy(LC.words(keys, key_words).view(np.int64)).cuda()


def dev_counts(counts):
    import torch

    return torch.from_numpy(np.array(counts, np.uint32).view(np.int32)).cuda()


def host_keys(t, key_words):
    a = t.cpu().numpy().view(np.uint64)
    return [int(x) for x in a] if key_words == 1 else [(int(hi) << 64) | int(lo) for lo, hi in a.reshape(-1, 2).tolist()]


def host_u32(t):
    return [int(c) for c in t.cpu().numpy().view(np.uint32)]


def build(ctx, table, key_words, key_bits):
    keys = sorted(table)
    return ctx.count_table(dev_keys(keys, key_words), dev_counts([table[k] for k in keys]), key_bits=key_bits)


def as_dict(t):
    keys = host_keys(t.keys, t.key_words)
    assert keys == sorted(set(keys)), "sorted distinct keys"
    return dict(zip(keys, host_u32(t.counts)))


def fails(call, code):
    import biolib_amd

    with pytest.raises(biolib_amd.BiolibError) as e:
        call()
    assert e.value.code == code and len(str(e.value).split(": ", 1)[1]) > 5, e.value
    return str(e.value)


def by_method(ta, tb, op, mode, lo, hi):
    if op == TC.UNION:
        return ta.union(tb, count=MODE_NAMES[mode], min_count=lo, max_count=hi)
    if op == TC.INTERSECT:
        return ta.intersect(tb, count=MODE_NAMES[mode], min_count=lo, max_count=hi)
    return (ta.subtract if op == TC.SUBTRACT else ta.subtract_counts)(tb, min_count=lo, max_count=hi)


@pytest.mark.parametrize("key_words", (1, 2))
def test_cases_match_the_model(ctx, key_words):
    ran = 0
    for case in TC.cases():
        if case["key_words"] != key_words:
            continue
        kw, kb = case["key_words"], case["key_bits"]
        ta = build(ctx, case["a"], kw, kb)
        tb = ta if case["same"] else (build(ctx, case["b"], kw, kb) if case["b"] is not None else None)
        a, b = case["a"], (case["a"] if case["same"] else case["b"])
        before = [t.clone() for t in (ta.keys, ta.counts)] + ([tb.keys.clone(), tb.counts.clone()] if tb is not None else [])
        for op, mode, lo, hi in case["rules"]:
            want, stats = TC.model(a, b, op, mode, lo, hi)
            out, got_stats = ta.combine_raw(tb, op, mode, lo, hi)
            assert {s: got_stats[s] for s in STATS} == stats, (case["name"], op, mode, lo, hi)
            assert (out.n_distinct, out.key_words, out.key_bits) == (len(want), kw, kb), (case["name"], op, mode, lo, hi)
            assert as_dict(out) == want, (case["name"], op, mode, lo, hi)
            out.close()
            # stats only: no table, the same numbers
            none, only = ta.combine_raw(tb, op, mode, lo, hi, table=False)
            assert none is None and only == got_stats
            ran += 1
        # the named methods are the same calls (None stands for the empty table only in the raw call)
        if tb is not None:
            for op, mode, lo, hi in case["rules"][:: max(len(case["rules"]) // 4, 1)]:
                out = by_method(ta, tb, op, mode, lo, hi)
                assert as_dict(out) == TC.model(a, b, op, mode, lo, hi)[0], (case["name"], op, mode)
                out.close()
            cmp = ta.compare(tb)
            _, stats = TC.model(a, b, TC.UNION, TC.SUM)
            j, wj = TC.jaccards(stats)
            assert {s: cmp[s] for s in STATS} == stats and cmp["jaccard"] == j and cmp["weighted_jaccard"] == wj, case["name"]
        after = [ta.keys, ta.counts] + ([tb.keys, tb.counts] if tb is not None else [])
        assert all((x == y).all() for x, y in zip(before, after)), (case["name"], "an input changed")
        ta.close()
        if tb is not None and tb is not ta:
            tb.close()
    assert ran > 200


@pytest.mark.parametrize("key_words", (1, 2))
def test_filter(ctx, key_words):
    for case in TC.cases():
        if case["key_words"] != key_words or case["kind"] not in ("counts", "random", "size"):
            continue
        a = case["a"]
        ta = build(ctx, a, key_words, case["key_bits"])
        for lo, hi in ((0, U32), (2, U32), (0, 1), (3, 3), (U32, U32), (0, 0)):
            out = ta.filter(min_count=lo, max_count=hi)
            assert as_dict(out) == {x: c for x, c in a.items() if lo <= c <= hi}, (case["name"], lo, hi)
            assert (out.key_words, out.key_bits) == (key_words, case["key_bits"])
            out.close()
        assert as_dict(ta.filter()) == a
        ta.close()


@pytest.mark.parametrize("key_words,key_bits", [(1, 62), (2, 102)])
def test_the_result_is_a_real_table(ctx, auto_prefix, key_words, key_bits):
    case = [c for c in TC.cases() if c["name"] == f"planted-diagonals-w{key_words}-b{key_bits}"][0]
    a, b = case["a"], case["b"]
    ta, tb = build(ctx, a, key_words, key_bits), build(ctx, b, key_words, key_bits)
    rng = np.random.default_rng(3)
    absent = [x for x in (LC._rand_key(rng, key_bits) for _ in range(300)) if x not in a and x not in b] + [1 << key_bits if key_bits < 64 * key_words else 5]
    queries = sorted(set(a) | set(b)) + absent
    rng.shuffle(queries)
    dq = dev_keys(queries, key_words)
    for op, mode in TC.OP_MODES:
        want, _ = TC.model(a, b, op, mode)
        widths = set()
        for option in (0, 1, 24, -1):
            ctx.set_option("table_prefix_bits", option)
            out = ta.combine_raw(tb, op, mode)[0]
            assert out.prefix_bits == min(option, key_bits, 24) if option >= 0 else 0 <= out.prefix_bits <= min(key_bits, 24)
            widths.add(out.prefix_bits)
            assert host_u32(out.lookup(dq)) == [want.get(q, 0) for q in queries], (op, mode, option)
            hist = np.bincount(np.minimum(np.array(list(want.values()), np.int64), 7), minlength=8).astype(np.uint64)
            assert np.array_equal(out.histogram(8), hist), (op, mode, option)
            out.close()
        assert {0, 1, 24} <= widths
    # an empty result is the n = 0 table
    empty = ta.intersect(tb, min_count=U32, max_count=U32)
    assert empty.n_distinct == 0 and empty.keys.shape[0] == 0 and (empty.lookup(dq) == 0).all() and empty.histogram(3).tolist() == [0, 0, 0]
    again = empty.union(empty)
    assert again.n_distinct == 0 and ta.union(empty).n_distinct == len(a) and as_dict(empty.union(tb)) == b
    for t in (empty, again, ta, tb):
        t.close()


@pytest.mark.parametrize("k", (31, 33))
def test_scans_read_a_union_like_a_built_table(ctx, k):
    k_, canonical, drop_last, seq, offs, m, tables = next(iter(LC.scan_cases((k,))))
    whole = [t for t in tables if len(t) > 2][0]
    keys = sorted(whole)
    a = {x: whole[x] for x in keys[::2] + keys[::3]}
    b = {x: whole[x] + 1 for x in keys[1::2] + keys[::3]}
    want, _ = TC.model(a, b, TC.UNION, TC.SUM)
    kw = 1 if k <= 32 else 2
    ta, tb, built = build(ctx, a, kw, 2 * k), build(ctx, b, kw, 2 * k), build(ctx, want, kw, 2 * k)
    union = ta.union(tb)
    batch = ctx.upload(seq, offs)
    c1, v1, r1 = batch.kmer_counts(union, k, canonical=canonical, drop_last=drop_last, valid=True)
    c2, v2, r2 = batch.kmer_counts(built, k, canonical=canonical, drop_last=drop_last, valid=True)
    assert (c1 == c2).all() and (v1 == v2).all() and r1 == r2 and r1["found"] > 0
    rc1, d1 = batch.read_counts(union, k, min_count=2, canonical=canonical, drop_last=drop_last)
    rc2, d2 = batch.read_counts(built, k, min_count=2, canonical=canonical, drop_last=drop_last)
    assert (rc1.records == rc2.records).all() and d1 == d2
    for t in (ta, tb, built, union, batch):
        t.close()


def test_a_million_keys_each(ctx):
    import torch

    ka, ca, kb, cb = TC.big_case()
    ta = ctx.count_table(torch.from_numpy(ka).cuda(), torch.from_numpy(ca.astype(np.uint32).view(np.int32)).cuda(), key_bits=62)
    tb = ctx.count_table(torch.from_numpy(kb).cuda(), torch.from_numpy(cb.astype(np.uint32).view(np.int32)).cuda(), key_bits=62)
    assert ta.n_distinct == ka.size == 1 << 20 and tb.n_distinct == kb.size
    # numpy model: positions of the common keys in both arrays
    common, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    assert 0.4 * ka.size < common.size < 0.6 * ka.size
    keys = np.union1d(ka, kb)
    total = np.zeros(keys.size, np.int64)
    total[np.searchsorted(keys, ka)] += ca
    total[np.searchsorted(keys, kb)] += cb
    union, st = ta.combine_raw(tb, TC.UNION, TC.SUM)
    assert np.array_equal(union.keys.cpu().numpy(), keys) and np.array_equal(union.counts.cpu().numpy().view(np.uint32), total.astype(np.uint32))
    mx = np.zeros(keys.size, np.int64)
    mx[np.searchsorted(keys, ka)] = ca
    pb = np.searchsorted(keys, kb)
    mx[pb] = np.maximum(mx[pb], cb)
    assert st == dict(n_a_only=ka.size - common.size, n_b_only=kb.size - common.size, n_both=common.size, n_out=keys.size,
                      sum_min=int(np.minimum(ca[ia], cb[ib]).sum()), sum_max=int(mx.sum()), sum_out=int(total.sum()))
    again = ta.union(tb)
    assert torch.equal(again.keys, union.keys) and torch.equal(again.counts, union.counts), "bit-reproducible"
    inter = ta.intersect(tb, count="min", min_count=500)
    mn = np.minimum(ca[ia], cb[ib])
    assert np.array_equal(inter.keys.cpu().numpy(), common[mn >= 500]) and np.array_equal(inter.counts.cpu().numpy(), mn[mn >= 500].astype(np.int32))
    sub = ta.subtract_counts(tb)
    diff = ca.copy()
    diff[ia] -= cb[ib]
    assert np.array_equal(sub.keys.cpu().numpy(), ka[diff > 0]) and np.array_equal(sub.counts.cpu().numpy(), diff[diff > 0].astype(np.int32))
    assert 1 << 19 <= sub.n_distinct < 1 << 20 and sub.prefix_bits == 19 + 4, "the automatic width of the result's own size"
    assert (sub.lookup(torch.from_numpy(ka).cuda()).cpu().numpy() == np.maximum(diff, 0)).all()
    for t in (ta, tb, union, again, inter, sub):
        t.close()


def test_refusals(ctx):
    import biolib_amd
    from biolib_amd import capi

    INVALID = capi.BL_ERR_INVALID
    L = ctx._lib
    t1, t1b = build(ctx, {1: 1, 2: 2}, 1, 62), build(ctx, {2: 5}, 1, 64)
    t2, t2b = build(ctx, {1: 1, 2: 2}, 2, 102), build(ctx, {2: 5}, 2, 128)
    h, st = C.c_void_p(), capi.TableStats()

    def raw(c, a, b, op=0, mode=0, lo=0, hi=U32, out=True):
        h.value = 0x1234
        rc = L.bl_table_combine(c, a, b, op, mode, lo, hi, C.byref(h) if out else None, C.byref(st))
        if rc != 0 and out:
            assert h.value is None, "a refused call leaves *out NULL"
        return capi.check(rc)

    fails(lambda: raw(None, t1._h, None), INVALID)                  # NULL ctx
    fails(lambda: raw(ctx._h, None, t1._h), INVALID)               # NULL a
    fails(lambda: raw(ctx._h, t1._h, t2._h), INVALID)              # key_words differ
    fails(lambda: raw(ctx._h, t1._h, t1b._h), INVALID)             # key_bits differ
    fails(lambda: raw(ctx._h, t2._h, t2b._h), INVALID)
    fails(lambda: raw(ctx._h, t1._h, t1._h, op=4, mode=TC.LEFT), INVALID)   # unknown op
    fails(lambda: raw(ctx._h, t1._h, t1._h, mode=5), INVALID)      # unknown mode
    for mode in (TC.SUM, TC.MIN, TC.MAX, TC.RIGHT):                # a mode the op does not take
        fails(lambda: raw(ctx._h, t1._h, t1._h, op=TC.SUBTRACT, mode=mode), INVALID)
        fails(lambda: raw(ctx._h, t1._h, t1._h, op=TC.COUNT_SUBTRACT, mode=mode, out=False), INVALID)
    fails(lambda: raw(ctx._h, t1._h, t1._h, lo=3, hi=2), INVALID)  # crossed bounds
    fails(lambda: t1.filter(min_count=3, max_count=2), INVALID)
    fails(lambda: capi.check(L.bl_table_filter(ctx._h, None, 0, U32, C.byref(h))), INVALID)
    fails(lambda: capi.check(L.bl_table_filter(ctx._h, t1._h, 0, U32, None)), INVALID)
    other = biolib_amd.Context(0)
    foreign = build(other, {1: 1}, 1, 62)
    fails(lambda: t1.union(foreign), INVALID)                      # a table of another context, on either side
    fails(lambda: foreign.union(t1), INVALID)
    fails(lambda: raw(other._h, t1._h, None), INVALID)
    foreign.close()
    other.close()
    with pytest.raises(ValueError):
        t1.union(t1, count="product")
    # the tables still work
    assert as_dict(t1.union(t1)) == {1: 2, 2: 4} and as_dict(t2.intersect(t2, count="left")) == {1: 1, 2: 2}
    for t in (t1, t1b, t2, t2b):
        t.close()
