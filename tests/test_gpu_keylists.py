"""GPU tests of the host side the key-list calls share for 8- and 16-byte keys (bl_keylist.hpp, blh::with_workspace, blpart::partition on
the context's scratch): what one context's grow-only scratch slots go through when calls of different sizes follow each other — a slot
that is empty, one that grows between the two primitives of a call or while it holds earlier contents, one that is already large — each
result against numpy."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
WIDTHS = pytest.mark.parametrize("words", [1, 2], ids=["u64", "u128"])


@pytest.fixture()
def ctx():
    """a NEW context per test: every scratch slot starts empty"""
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def dev(arr):
    """uint64[n] / uint64[n, w] -> int64 device tensor of the same shape"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def draw(rng, n, words, distinct):
    """n keys drawn with replacement from `distinct` values; two-word keys (low, high) differ in both words"""
    if words == 1:
        pool = rng.integers(0, 1 << 63, distinct, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, distinct, dtype=np.uint64)
    else:
        pool = np.stack([rng.integers(0, 1 << 63, distinct, dtype=np.uint64) * np.uint64(2), rng.integers(0, 1 << 40, distinct, dtype=np.uint64)], axis=1)
        pool[::3, 0] = pool[0, 0]  # equal low words: the high word decides
    return pool[rng.integers(0, distinct, n)]


def in_order(arr):
    """numeric order of the keys (hi << 64 | lo for two-word keys); rows of records in lexicographic order"""
    if arr.ndim == 1:
        return np.sort(arr)
    return arr[np.lexsort(arr.T)]  # (the last column is the primary key)


def unique_counts(arr):
    if arr.ndim == 1:
        return np.unique(arr, return_counts=True)
    u, c = np.unique(arr, axis=0, return_counts=True)
    order = np.lexsort(u.T)
    return u[order], c[order]


def methods(ctx, words):
    if words == 1:
        return ctx.sort_unique, ctx.sort_count, ctx.merge_runs, ctx.partition
    return ctx.sort_unique128, ctx.sort_count128, ctx.merge_runs128, ctx.partition128


@WIDTHS
@pytest.mark.parametrize("op", ["sort_unique", "sort_count"])
def test_fresh_context_small_large_small(ctx, words, op):
    """3 keys on empty slots, 200,000 keys (about half of them duplicates: slot 5 grows between the sort and the second primitive), 3 keys
    on slots that are large by then"""
    sort_unique, sort_count, _, _ = methods(ctx, words)
    rng = np.random.default_rng(31 + words)
    for n in (3, 200_000, 3):
        keys = draw(rng, n, words, max(2, n // 2))
        eu, ec = unique_counts(keys)
        t = dev(keys)
        if op == "sort_unique":
            nu = sort_unique(t)
            assert nu == len(eu) and np.array_equal(host(t)[:nu], eu), (words, n)
        else:
            u, c = sort_count(t)
            assert np.array_equal(host(u), eu) and np.array_equal(c.cpu().numpy().astype(np.int64), ec), (words, n)
            assert np.array_equal(host(t), in_order(keys)), (words, n)
        if n > 3:
            assert len(eu) < n * 3 // 4 and ec.max() > 1


def write_runs(tmp_path, tag, keys, sizes):
    paths, at = [], 0
    for i, size in enumerate(sizes):
        p = tmp_path / f"tmp.run_{tag}_{i}.bin"
        in_order(keys[at:at + size]).tofile(p)
        paths.append(p)
        at += size
    assert at == len(keys)
    return paths


@WIDTHS
def test_merge_after_merge_on_one_context(ctx, words, tmp_path):
    """3 runs (one empty), sort + unique of their merge, 8 larger runs (slots 4 and 5 grow while they hold the earlier contents), the
    first 3 again"""
    sort_unique, _, merge_runs, _ = methods(ctx, words)
    rng = np.random.default_rng(77 + words)
    small_sizes = [5000, 0, 4999]
    small = draw(rng, sum(small_sizes), words, 4000)  # duplicates inside and across runs
    small_paths = write_runs(tmp_path, "small", small, small_sizes)
    large_sizes = [40_000 + 13 * i for i in range(8)]
    large = draw(rng, sum(large_sizes), words, 150_000)
    large_paths = write_runs(tmp_path, "large", large, large_sizes)

    merged = merge_runs(small_paths)
    assert np.array_equal(host(merged), in_order(small))
    nu = sort_unique(merged)
    eu, _ = unique_counts(small)
    assert nu == len(eu) and np.array_equal(host(merged)[:nu], eu)
    assert np.array_equal(host(merge_runs(large_paths)), in_order(large))
    assert np.array_equal(host(merge_runs(small_paths)), in_order(small))


@WIDTHS
def test_merge_of_1_2_5_and_8_runs(ctx, words, tmp_path):
    """the run counts of test_spill_format.py::test_merge_runs_on_device for both widths: one run (nothing to merge), a pair, an odd run
    copied through a level (5, one of them empty), a full tree (8)"""
    merge_runs = methods(ctx, words)[2]
    rng = np.random.default_rng(5 + words)
    keys = draw(rng, 30_000, words, 8000)
    for n_runs in (1, 2, 5, 8):
        cuts = np.sort(rng.integers(0, len(keys), n_runs - 1))
        edges = np.concatenate([[0], cuts, [len(keys)]]).astype(np.int64)
        if n_runs == 5:
            edges[2] = edges[1]  # an empty run
        used = np.concatenate([keys[edges[i]:edges[i + 1]] for i in range(n_runs)])
        paths = write_runs(tmp_path, f"r{n_runs}", used, [int(e1 - e0) for e0, e1 in zip(edges[:-1], edges[1:])])
        assert np.array_equal(host(merge_runs(paths)), in_order(used)), (words, n_runs)


def owners_of(kind, keys, hashes, parts, seed):
    import biolib_amd

    if kind == "u64":
        h = O.hash64_np(keys, seed)
    elif kind == "u128":
        h = np.array([biolib_amd.hash64_u128(int(lo), int(hi), seed) for lo, hi in keys.tolist()], dtype=np.uint64)
    else:
        h = hashes
    return (h % np.uint64(parts)).astype(np.int64)


@pytest.mark.parametrize("kind", ["u64", "u128", "records", "records128"])
def test_partitions_of_different_shapes_on_one_context(ctx, kind):
    """n = 1; 5,000 items into 64 buckets (two blocks of 4096); a sort + unique in between (it shares slot 4); 70,000 items into 3 buckets
    (18 blocks); the second shape again.  Buckets contiguous and in bucket order, sizes as counted on the host; inside a bucket the items of
    a block come in no particular order, so buckets compare as sorted lists."""
    seed = 5
    width = {"u64": 1, "u128": 2, "records": 2, "records128": 4}[kind]
    rng = np.random.default_rng(len(kind))

    def one(n, parts):
        if kind in ("u64", "u128"):
            items = draw(rng, n, width, max(1, n - n // 5))
            hashes = None
            out, counts = (ctx.partition if kind == "u64" else ctx.partition128)(dev(items), parts, seed=seed)
        else:
            items = rng.integers(0, 1 << 63, (n, width), dtype=np.uint64)
            hashes = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
            hashes[::7] = hashes[0]  # one heavy bucket
            out, counts = (ctx.partition_records if kind == "records" else ctx.partition_records128)(dev(hashes), dev(items), parts)
        got = host(out)
        owner = owners_of(kind, items, hashes, parts, seed)
        assert got.shape == items.shape and counts == np.bincount(owner, minlength=parts).tolist(), (kind, n, parts)
        edges = np.concatenate([[0], np.cumsum(counts)])
        for b in range(parts):
            assert np.array_equal(in_order(got[edges[b]:edges[b + 1]]), in_order(items[owner == b])), (kind, n, parts, b)

    one(1, 5)
    one(5000, 64)
    keys = draw(rng, 30_000, 1, 9000)
    t = dev(keys)
    nu = ctx.sort_unique(t)
    assert np.array_equal(host(t)[:nu], np.unique(keys))
    one(70_000, 3)
    one(5000, 64)
