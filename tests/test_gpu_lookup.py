"""GPU tests of the count table (bl_table_build_* / bl_table_lookup_* / bl_scan_kmer_counts / bl_table_histogram and their Python
binding): against Python dicts, numpy and the Python model of the 128-bit scan (kmers128_model.py).  The tables, queries and batches
are those of the host emulation (lookup_cases.py): the shapes are small, every index path was run under the sanitizers there."""
import ctypes as C

import numpy as np
import pytest

import kmers128_model as M
import lookup_cases as LC

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
U32 = (1 << 32) - 1
CANARY32, CANARY8 = 0x5CA1AB1E, 0xA5


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
    return t.cpu().numpy().view(np.uint32)


def build(ctx, table, key_words, key_bits):
    keys = list(table)
    return ctx.count_table(dev_keys(keys, key_words), dev_counts([table[k] for k in keys]), key_bits=key_bits)


def invalid(call):
    import biolib_amd

    with pytest.raises(biolib_amd.BiolibError) as e:
        call()
    assert e.value.code == biolib_amd.capi.BL_ERR_INVALID, e.value
    return str(e.value)


# ---- build

@pytest.mark.parametrize("key_words,key_bits", [(1, 62), (1, 64), (2, 102), (2, 128)])
def test_build_merges_shuffled_input_with_duplicates(ctx, key_words, key_bits):
    rng = np.random.default_rng(key_bits)
    distinct = sorted({LC._rand_key(rng, key_bits) for _ in range(3000)} | {0, (1 << key_bits) - 1})
    picks = rng.integers(0, len(distinct), 20_000)
    keys = [distinct[i] for i in picks]
    counts = [int(c) for c in rng.integers(0, 1000, len(keys))]
    want = {}
    for k, c in zip(keys, counts):
        want[k] = want.get(k, 0) + c
    dk, dc = dev_keys(keys, key_words), dev_counts(counts)
    before_k, before_c = dk.clone(), dc.clone()
    t = ctx.count_table(dk, dc, key_bits=key_bits)
    assert (dk == before_k).all() and (dc == before_c).all(), "the build changed its input"
    del dk, dc  # the table has its own copy
    assert (t.n_distinct, t.key_words, t.key_bits) == (len(want), key_words, key_bits) and 0 <= t.prefix_bits <= min(key_bits, 24)
    got = host_keys(t.keys, key_words)
    assert got == sorted(want), "sorted, duplicate-free, 128-bit order"
    assert [int(c) for c in host_u32(t.counts)] == [want[k] for k in got]
    # counts = None: the multiplicities of the raw list
    raw = ctx.count_table(dev_keys(keys, key_words), None, key_bits=key_bits)
    mult = {}
    for k in keys:
        mult[k] = mult.get(k, 0) + 1
    assert host_keys(raw.keys, key_words) == sorted(mult) and [int(c) for c in host_u32(raw.counts)] == [mult[k] for k in sorted(mult)]
    t.close()
    raw.close()


@pytest.mark.parametrize("key_words", (1, 2))
def test_counts_saturate(ctx, key_words):
    keys = [5, 9, 5, 9, 9, 7]
    counts = [U32, U32 - 1, 5, 1, 1, 3]
    t = ctx.count_table(dev_keys(keys, key_words), dev_counts(counts), key_bits=8)
    assert host_keys(t.keys, key_words) == [5, 7, 9] and [int(c) for c in host_u32(t.counts)] == [U32, 3, U32]
    assert [int(c) for c in host_u32(t.lookup(dev_keys([9, 6, 5, 7], key_words)))] == [U32, 0, U32, 3]
    t.close()


def test_build_and_lookup_refusals(ctx):
    import torch

    # a key above key_bits
    for kw, kb, bad in ((1, 62, 1 << 62), (1, 10, 1 << 63), (2, 102, 1 << 102), (2, 102, 1 << 127), (2, 40, 1 << 64), (2, 64, 1 << 64)):
        invalid(lambda: ctx.count_table(dev_keys([1, 2, bad, 3], kw), None, key_bits=kb))
    for kw, kb in ((1, 0), (1, 65), (2, 0), (2, 129)):
        invalid(lambda: ctx.count_table(dev_keys([1], kw), None, key_bits=kb))
    # a misaligned 128-bit array
    odd = torch.zeros(9, dtype=torch.int64, device="cuda")[1:].view(4, 2)
    assert odd.data_ptr() % 16 == 8 and odd.is_contiguous()
    invalid(lambda: ctx.count_table(odd, None, key_bits=128))
    # width mismatch between table and lookup
    t1, t2 = ctx.count_table(dev_keys([1, 2], 1), None), ctx.count_table(dev_keys([1, 2], 2), None)
    q, out = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    L = ctx._lib
    for call, t in ((L.bl_table_lookup_u64, t2), (L.bl_table_lookup_u128, t1)):
        assert call(ctx._h, t._h, C.c_void_p(q.data_ptr()), 2, C.c_void_p(out.data_ptr())) == -1
    assert (out == 0).all()
    invalid(lambda: t2.lookup(odd))
    invalid(lambda: ctx.set_option("table_prefix_bits", 25))
    invalid(lambda: ctx.set_option("table_prefix_bits", -2))
    t1.close()
    t2.close()


@pytest.mark.parametrize("key_words", (1, 2))
def test_empty_table(ctx, key_words):
    import torch

    empty = torch.empty((0, 2) if key_words == 2 else (0,), dtype=torch.int64, device="cuda")
    t = ctx.count_table(empty, None, key_bits=62)
    assert t.n_distinct == 0 and t.keys.shape[0] == 0 and t.counts.shape[0] == 0
    assert (t.lookup(dev_keys([0, 1, (1 << 62) - 1, 1 << 63], key_words)) == 0).all()
    assert t.lookup(empty).numel() == 0
    assert t.histogram(4).tolist() == [0, 0, 0, 0]
    seq, offs = LC.make_batch(31, np.random.default_rng(5))
    b = ctx.upload(seq, offs)
    counts, r = b.kmer_counts(t, 31)
    assert (counts == 0).all() and r["found"] == 0 and r["sum_counts"] == 0 and r["count"] == M.digest(M.scan(seq.tobytes(), offs, 31))["count"]
    t.close()


# ---- lookup

@pytest.mark.parametrize("key_words", (1, 2))
def test_lookup_families_at_every_prefix_width(ctx, auto_prefix, key_words):
    for name, kw, kb, table, queries, options in LC.table_cases():
        if kw != key_words:
            continue
        want = [table.get(q, 0) for q in queries]
        dq = dev_keys(queries, kw)
        widths = set()
        for option in options:
            ctx.set_option("table_prefix_bits", option)
            t = build(ctx, table, kw, kb)
            assert t.prefix_bits == min(option, kb, 24) if option >= 0 else 0 <= t.prefix_bits <= min(kb, 24), (name, option)
            widths.add(t.prefix_bits)
            assert [int(c) for c in host_u32(t.lookup(dq))] == want, (name, option)
            t.close()
        assert {0, 1, min(kb, 24)} <= widths


@pytest.mark.parametrize("key_words,key_bits", [(1, 62), (2, 102)])
def test_lookup_many_workgroups_automatic_prefix(ctx, key_words, key_bits):
    """2^20 + 1 random keys, 2^20 queries in random order, half of them absent: the table's keys are even, the absent queries odd"""
    import torch

    n = (1 << 20) + 1
    rng = np.random.default_rng(key_bits)
    w = rng.integers(0, 1 << 63, (n, 2), dtype=np.uint64)
    w[:, 0] &= np.uint64(M64 - 1) if key_words == 2 else np.uint64((1 << key_bits) - 2)
    w[:, 1] &= np.uint64((1 << (key_bits - 64)) - 1) if key_words == 2 else np.uint64(0)
    _, first = np.unique(w, axis=0, return_index=True)
    w = w[np.sort(first)]
    counts = rng.integers(1, 1 << 32, len(w), dtype=np.uint64).astype(np.uint32)
    arr = w if key_words == 2 else np.ascontiguousarray(w[:, 0])
    t = ctx.count_table(torch.from_numpy(arr.view(np.int64)).cuda(), torch.from_numpy(counts.view(np.int32)).cuda(), key_bits=key_bits)
    assert t.n_distinct == len(w) and t.prefix_bits > 1
    nq = 1 << 20
    pick = rng.integers(0, len(w), nq)
    q = w[pick].copy()
    absent = rng.random(nq) < 0.5
    q[absent, 0] |= np.uint64(1)
    want = np.where(absent, 0, counts[pick]).astype(np.uint32)
    qa = q if key_words == 2 else np.ascontiguousarray(q[:, 0])
    got = host_u32(t.lookup(torch.from_numpy(qa.view(np.int64)).cuda()))
    assert np.array_equal(got, want) and 0.4 < absent.mean() < 0.6
    t.close()


# ---- the fused scan

def scan_with_canaries(b, table, k, canonical, drop_last, first, n, span, counts=True):
    import torch

    from biolib_amd.scan import _flags

    c = torch.full((span + 4,), CANARY32, dtype=torch.int32, device="cuda") if counts else None
    v = torch.full((span + 4,), CANARY8, dtype=torch.uint8, device="cuda")
    r = b.kmer_counts_raw(table, k, _flags(canonical, drop_last, True), first, n, c, v)
    if counts:
        assert (c[span:] == CANARY32).all(), "canary behind d_counts"
    assert (v[span:] == CANARY8).all(), "canary behind d_valid"
    return (host_u32(c[:span]) if counts else None), v[:span].cpu().numpy(), r.as_dict()


@pytest.mark.parametrize("k", (1, 31, 32, 33, 64))
def test_scan_vs_model(ctx, k):
    for k_, canonical, drop_last, seq, offs, m, tables in LC.scan_cases((k,)):
        b = ctx.upload(seq, offs)
        n_bases = len(seq)
        for table in tables:
            for kw in ((1, 2) if k <= 32 else (2,)):
                t = build(ctx, table, kw, 2 * k)
                whole = None
                for first, n in LC.RANGES:
                    end = n_bases if n == 0 else first + n
                    w_counts, w_valid, d = LC.expected_scan(m, table, first, end)
                    counts, valid, r = scan_with_canaries(b, t, k, canonical, drop_last, first, n, end - first)
                    assert np.array_equal(counts, w_counts) and np.array_equal(valid, w_valid), (k, canonical, drop_last, kw, first)
                    assert {x: r[x] for x in d} == d and r["status"] == 0, (k, canonical, drop_last, kw, first)
                    # d_counts = NULL: the same digest
                    _, valid2, r2 = scan_with_canaries(b, t, k, canonical, drop_last, first, n, end - first, counts=False)
                    assert r2 == r and np.array_equal(valid2, w_valid)
                    whole = whole or (counts, valid, r)
                # three consecutive ranges concatenate to the whole, and their sums add up
                parts = [scan_with_canaries(b, t, k, canonical, drop_last, f, n, n) for f, n in ((0, 4099), (4099, 13), (4112, n_bases - 4112))]
                assert np.array_equal(np.concatenate([p[0] for p in parts]), whole[0]) and np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
                for word in ("count", "xor_hash", "xor_pos"):
                    assert sum(p[2][word] for p in parts) & M64 == whole[2][word]
                for word in ("xor_value", "aux"):
                    assert parts[0][2][word] ^ parts[1][2][word] ^ parts[2][2][word] == whole[2][word]
                t.close()
        b.close()


def test_scan_against_another_batchs_table(ctx):
    k = 31
    seq, offs = LC.make_batch(k, np.random.default_rng(77))
    other = seq.copy()
    other[2000:6000] = LC.make_batch(k, np.random.default_rng(78))[0][2000:6000]  # shares the k-mers outside [2000 - k, 6000)
    for canonical in (False, True):
        m_other = M.scan(other.tobytes(), offs, k, 0, canonical, False)
        table = LC.own_table(m_other, drop=False)
        m = M.scan(seq.tobytes(), offs, k, 0, canonical, False)
        w_counts, w_valid, d = LC.expected_scan(m, table, 0, len(seq))
        assert 100 < d["xor_hash"] < d["count"] - 100
        b = ctx.upload(seq, offs)
        t = build(ctx, table, 2, 2 * k)
        counts, valid, r = scan_with_canaries(b, t, k, canonical, False, 0, 0, len(seq))
        assert np.array_equal(counts, w_counts) and np.array_equal(valid, w_valid) and {x: r[x] for x in d} == d
        t.close()
        b.close()


def test_scan_refusals_and_empty_range(ctx):
    import torch

    import biolib_amd

    seq, offs = LC.make_batch(31, np.random.default_rng(3))
    b = ctx.upload(seq, offs)
    t1, t2 = ctx.count_table(dev_keys([1, 2], 1), None, key_bits=62), ctx.count_table(dev_keys([1, 2], 2), None, key_bits=102)
    assert "key_bits" in invalid(lambda: b.kmer_counts(t1, 32))   # 2k = 64 > 62
    assert "key_bits" in invalid(lambda: b.kmer_counts(t2, 52))   # 2k = 104 > 102
    t64 = ctx.count_table(dev_keys([1, 2], 1), None, key_bits=64)
    invalid(lambda: b.kmer_counts(t64, 33))                       # a one-word table takes k <= 32
    invalid(lambda: b.kmer_counts(t2, 0))
    invalid(lambda: b.kmer_counts(t2, 65))
    other = biolib_amd.Context(0)
    foreign = other.count_table(dev_keys([1, 2], 2), None, key_bits=102)
    invalid(lambda: b.kmer_counts(foreign, 31))
    hist = np.zeros(4, np.uint64)
    assert ctx._lib.bl_table_histogram(ctx._h, foreign._h, hist.ctypes.data_as(C.c_void_p), 4) == biolib_amd.capi.BL_ERR_INVALID
    foreign.close()
    other.close()
    # an empty range succeeds and writes nothing
    c = torch.full((8,), CANARY32, dtype=torch.int32, device="cuda")
    v = torch.full((8,), CANARY8, dtype=torch.uint8, device="cuda")
    r = b.kmer_counts_raw(t2, 31, biolib_amd.FLAG_SYNC, len(seq), 0, c, v)
    assert r.count == 0 and r.xor_hash == 0 and r.xor_pos == 0 and (c == CANARY32).all() and (v == CANARY8).all()
    invalid(lambda: b.kmer_counts_raw(t2, 31, biolib_amd.FLAG_SYNC, len(seq) + 1, 0, c, v))
    for t in (t1, t2, t64):
        t.close()
    b.close()


# ---- equivalence with the unfused chain

@pytest.mark.parametrize("k", (31, 51))
def test_scan_equals_kmers128_then_lookup(ctx, k):
    import torch

    from biolib_amd.scan import _flags

    n = 150 * 7000  # about 1 Mbp of 150-bp reads
    b = ctx.synth(11, n, 150)
    ref = ctx.synth(12, n, 150)
    # the table: this batch's canonical k-mers of the first half and another batch's, counted by the library itself
    vals = torch.empty((2 * n, 2), dtype=torch.int64, device="cuda")
    ok = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    b.kmers128_raw(k, 0, _flags(True, False, True), 0, n // 2, vals, None, ok)
    ref.kmers128_raw(k, 0, _flags(True, False, True), 0, 0, vals[n // 2:], None, ok[n // 2:])
    keys = vals[: n // 2 + n][ok[: n // 2 + n] == 1].contiguous()
    uniq, mult = ctx.sort_count128(keys, key_bits=2 * k)
    tables = [ctx.count_table(uniq, mult, key_bits=2 * k)]
    if k <= 32:
        tables.append(ctx.count_table(uniq[:, 0].contiguous(), mult, key_bits=2 * k))
    for canonical in (True, False):
        v = torch.empty((n, 2), dtype=torch.int64, device="cuda")
        valid = torch.empty(n, dtype=torch.uint8, device="cuda")
        b.kmers128_raw(k, 0, _flags(canonical, False, True), 0, 0, v, None, valid)
        for t in tables:
            chain = t.lookup(v if t.key_words == 2 else v[:, 0].contiguous())
            chain = torch.where(valid == 1, chain, torch.zeros_like(chain))
            counts, got_valid, r = b.kmer_counts(t, k, canonical=canonical, valid=True)
            assert torch.equal(counts, chain) and torch.equal(got_valid, valid)
            assert r["found"] == int((chain != 0).sum()) and r["sum_counts"] == int(chain.to(torch.int64).bitwise_and(U32).sum()) & M64
            if canonical:
                assert r["found"] > n // 3
    for t in tables:
        t.close()


# ---- histogram

@pytest.mark.parametrize("n_bins", (1, 2, 256, 65536))
def test_histogram_vs_bincount(ctx, n_bins):
    rng = np.random.default_rng(n_bins)
    edge = [0, 1, max(n_bins - 2, 0), n_bins - 1, n_bins, U32]
    counts = np.concatenate([np.array(edge, np.uint64), rng.integers(0, 2 * n_bins + 2, 70_000, dtype=np.uint64),
                             rng.integers(0, 1 << 32, 1000, dtype=np.uint64)]).astype(np.uint32)
    keys = [int(x) for x in rng.permutation(len(counts))]
    for kw in (1, 2):
        t = ctx.count_table(dev_keys(keys, kw), dev_counts(counts), key_bits=40)
        assert t.n_distinct == len(counts)
        want = np.bincount(np.minimum(counts.astype(np.int64), n_bins - 1), minlength=n_bins).astype(np.uint64)
        got = t.histogram(n_bins)
        assert np.array_equal(got, want) and int(got.sum()) == len(counts)
        t.close()
    t = ctx.count_table(dev_keys([1], 1), None)
    invalid(lambda: t.histogram(0))
    invalid(lambda: t.histogram(65537))
    t.close()


# ---- end to end, Python

@pytest.mark.parametrize("k,m", [(31, 15), (51, 21)])
def test_count_then_table_then_kmer_counts(ctx, k, m):
    from biolib_amd import shard

    rng = np.random.default_rng(k)
    n_reads, L = 60, 150
    base = rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000)
    starts = rng.integers(0, len(base) - L, n_reads)
    seq = np.concatenate([base[s:s + L] for s in starts])  # overlapping reads of one short genome: multiplicities above 1
    seq[[100, 4000]] = ord("N")
    offs = np.arange(0, len(seq) + 1, L, dtype=np.uint64)
    b = ctx.upload(seq, offs)
    keys, mult = shard.count_kmers_via_super_kmers(ctx, b, k, m, canonical=True)
    t = ctx.count_table(keys, mult, key_bits=2 * k)
    model = M.scan(seq.tobytes(), offs, k, 0, True, False)
    valid = model["valid"] == 1
    pairs = np.stack([model["lo"][valid], model["hi"][valid]], axis=1)
    uniq, inverse, cnt = np.unique(pairs, axis=0, return_inverse=True, return_counts=True)
    assert t.n_distinct == len(uniq) and t.key_words == (2 if keys.dim() == 2 else 1) and cnt.max() > 1
    counts, got_valid, r = b.kmer_counts(t, k, canonical=True, valid=True)
    counts = host_u32(counts)
    assert np.array_equal(got_valid.cpu().numpy() == 1, valid)
    assert np.array_equal(counts[valid], cnt[inverse.reshape(-1)].astype(np.uint32)) and (counts[~valid] == 0).all()
    assert r["found"] == r["count"] == int(valid.sum()) and r["sum_counts"] == int(counts.sum(dtype=np.uint64))
    hist = t.histogram(256)
    assert int(hist.sum()) == len(uniq) and np.array_equal(hist, np.bincount(cnt, minlength=256).astype(np.uint64)) and hist[0] == 0
    t.close()
    b.close()


# ---- past the grid caps (scale_cases.py): the stride loops of lookup_kernel, histogram_lds_kernel and histogram_global_kernel

def closed_form_table(ctx, key_words):
    """8,392,705 keys in closed form (a bijection of the index: distinct), counts from a seeded generator with every histogram edge"""
    import torch

    import scale_cases as S

    n = S.table_size()
    keys = S.keys_of(np.arange(n, dtype=np.uint64), key_words)
    t = ctx.count_table(torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(S.table_counts().copy().view(np.int32)).cuda(),
                        key_bits=S.KEY_BITS_1 if key_words == 1 else S.KEY_BITS_2)
    assert t.n_distinct == n, "the keys are distinct"
    return t


@pytest.fixture(scope="module")
def big_table(ctx):
    t = closed_form_table(ctx, 1)
    yield t
    t.close()


def check_lookup_past_the_grid_cap(t, key_words):
    import torch

    import scale_cases as S

    idx = S.query_indices()
    nq = len(idx)
    assert nq > S.CAPS["LOOKUP_GRID_MAX"] * S.CAPS["LTPB"] * S.CAPS["G"]
    q = torch.from_numpy(S.keys_of(idx, key_words).view(np.int64)).cuda()
    got = host_u32(t.lookup(q))
    want = S.expected_lookup()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, ("first wrong queries", bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist(), "of", nq)


def test_lookup_past_the_grid_cap_one_word(big_table):
    check_lookup_past_the_grid_cap(big_table, 1)


def test_lookup_past_the_grid_cap_two_words(ctx):
    t = closed_form_table(ctx, 2)
    check_lookup_past_the_grid_cap(t, 2)
    t.close()


@pytest.mark.parametrize("n_bins", (1, 2, 4096, 8192, 8193, 65536))
def test_histogram_past_the_grid_caps(big_table, n_bins):
    """n_bins up to 4,096: the LDS kernel at its grid cap; 8,192: its largest; above: the global kernel at its grid cap"""
    import scale_cases as S

    assert n_bins in S.HIST_BINS
    want = S.expected_histogram(n_bins)
    got = big_table.histogram(n_bins)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0 and int(got.sum()) == S.table_size(), ("first wrong bins", bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
