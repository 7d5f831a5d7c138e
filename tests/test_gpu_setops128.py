"""GPU tests of the consumer side for 16-byte keys (k-mers of kmer_view<__uint128_t>, k up to 64): sort, sort + unique, run-length
count, the two intersection kernels of bl_jaccard_sorted_u128, the owner split, the run files and the drop-in headers — against
numpy / Python-int sets, the Python model of the 128-bit scan (kmers128_model.py) and files the reference wrote (golden/spill128)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmers128_model as M
import setops128_cases as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SP = os.path.join(HERE, "golden", "spill128")
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def dev(arr):
    """uint64[n, 2] -> int64[n, 2] device tensor"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1, 2)).cuda()


def host(t, n=None):
    a = t.cpu().numpy().view(np.uint64).reshape(-1, 2)
    return a if n is None else a[:n]


def ints(arr):
    return [(int(hi) << 64) | int(lo) for lo, hi in arr.tolist()]


def lexsorted(arr):
    return arr[np.lexsort((arr[:, 0], arr[:, 1]))]


@pytest.fixture(scope="module")
def pool():
    """Python-int keys of every class of setops128_cases (any, high word only, low word only, top bits set), and small ones"""
    rng = np.random.default_rng(2024)
    keys = []
    for kind in ("any", "high_only", "low_only", "top_bits"):
        keys += S._distinct(rng, 3000, kind)
    keys += [0, 1, 2, 3, M64, 1 << 64, (1 << 64) + 1, (1 << 128) - 1, (1 << 127), (1 << 63)]
    return keys


@pytest.mark.parametrize("key_bits", [2, 64, 66, 126, 128])
def test_sort_and_sort_unique(ctx, pool, key_bits):
    rng = np.random.default_rng(key_bits)
    mask = (1 << key_bits) - 1
    for n in (0, 1, 2, 4097, 40_000):
        keys = [pool[i] & mask for i in rng.integers(0, len(pool), n)]  # drawn with replacement: duplicates
        arr = S.to_array(keys)
        t = dev(arr)
        ctx.sort128(t, key_bits=key_bits, n=n)
        assert np.array_equal(host(t, n), lexsorted(arr)), (key_bits, n)
        t = dev(arr)
        nu = ctx.sort_unique128(t, key_bits=key_bits, n=n)
        exp = sorted(set(keys))
        assert nu == len(exp) and ints(host(t, nu)) == exp, (key_bits, n)
        if n == 40_000 and key_bits >= 64:
            assert nu < n  # the pool gave duplicates
    # the default key_bits (128) is valid whatever the keys hold
    t = dev(S.to_array([5, 3, 3]))
    assert ctx.sort_unique128(t) == 2 and ints(host(t, 2)) == [3, 5]


@pytest.fixture(scope="module")
def jaccard_cases():
    return [(name, dev(S.to_array(a)), len(a), dev(S.to_array(b)), len(b), len(set(a) & set(b))) for name, a, b in S.cases()]


@pytest.mark.parametrize("path", [1, 2])
def test_jaccard_each_kernel_on_the_emulation_shapes(ctx, jaccard_cases, path):
    ctx.set_option("jaccard128_path", path)
    try:
        for name, ta, na, tb, nb, both in jaccard_cases:
            assert ctx.jaccard128(ta, na, tb, nb) == (both, na + nb - both), (name, path)
            assert ctx.jaccard128(tb, nb, ta, na) == (both, na + nb - both), (name, path, "swapped")
            assert ctx.jaccard128(ta, na, ta, na) == (na, na), (name, path, "self")
    finally:
        ctx.set_option("jaccard128_path", 0)


def test_jaccard_chooses_for_sets_of_very_different_size(ctx):
    rng = np.random.default_rng(40)
    big = S._distinct(rng, 100_000, "any")
    small = sorted(set(big[i] for i in rng.integers(0, len(big), 25)) | set(S._distinct(rng, 40, "top_bits")))[:40]
    both = len(set(small) & set(big))
    assert 0 < both < 40
    ts, tb = dev(S.to_array(small)), dev(S.to_array(big))
    ctx.set_option("jaccard128_path", 0)
    assert ctx.jaccard128(ts, 40, tb, 100_000) == (both, 100_040 - both)
    assert ctx.jaccard128(tb, 100_000, ts, 40) == (both, 100_040 - both)
    assert ctx.jaccard128(tb, 100_000, tb, 100_000) == (100_000, 100_000)
    for path in (1, 2):  # and both kernels agree on it
        ctx.set_option("jaccard128_path", path)
        try:
            assert ctx.jaccard128(ts, 40, tb, 100_000) == (both, 100_040 - both)
            assert ctx.jaccard128(tb, 100_000, ts, 40) == (both, 100_040 - both)
        finally:
            ctx.set_option("jaccard128_path", 0)


def test_arguments_are_checked(ctx):
    import biolib_amd as B
    from biolib_amd import capi

    L = capi.lib()
    t = dev(S.to_array([9, 8, 7, 6]))
    n = C.c_uint64()
    odd = C.c_void_p(t.data_ptr() + 8)  # 8-byte aligned only
    assert L.bl_sort_u128(ctx._h, odd, 2, 128) == capi.BL_ERR_INVALID
    assert L.bl_sort_unique_u128(ctx._h, odd, 2, 128, C.byref(n)) == capi.BL_ERR_INVALID
    assert L.bl_jaccard_sorted_u128(ctx._h, odd, 1, C.c_void_p(t.data_ptr()), 1, C.byref(n), C.byref(n)) == capi.BL_ERR_INVALID
    for bits in (0, 129):
        assert L.bl_sort_u128(ctx._h, C.c_void_p(t.data_ptr()), 4, bits) == capi.BL_ERR_INVALID
    assert ints(host(t)) == [9, 8, 7, 6]  # nothing was touched
    counts = (C.c_uint64 * 65)()
    for parts in (0, 65):
        assert L.bl_partition_u128(ctx._h, C.c_void_p(t.data_ptr()), 4, parts, 0, C.c_void_p(t.data_ptr()), counts) == capi.BL_ERR_INVALID
    for value in (-1, 3):
        with pytest.raises(B.BiolibError):
            ctx.set_option("jaccard128_path", value)
    # n = 0 succeeds and touches nothing, NULL arrays included
    assert L.bl_sort_u128(ctx._h, None, 0, 128) == 0 and L.bl_sort_unique_u128(ctx._h, None, 0, 128, C.byref(n)) == 0 and n.value == 0
    i, u = C.c_uint64(7), C.c_uint64(7)
    assert L.bl_jaccard_sorted_u128(ctx._h, None, 0, None, 0, C.byref(i), C.byref(u)) == 0 and (i.value, u.value) == (0, 0)
    assert ctx.jaccard128(t, 0, t, 4) == (0, 4)


@pytest.mark.parametrize("k,canonical", [(41, True), (64, True), (33, False)])
def test_scan_sort_unique_jaccard_end_to_end(ctx, k, canonical):
    """the route of the reference's Jaccard tool with kmer_t = __uint128_t: k-mers of the idiom loop (drop_last) -> sort + unique -> Jaccard"""
    n = 50_000
    first = np.random.default_rng(500).choice(np.frombuffer(b"ACGT", np.uint8), n)
    second = first.copy()
    second[::97] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), first[::97])]  # every 97th base changed
    second[910::911] = ord("N")
    offs = np.array([0, n], np.uint64)
    sets, models = [], []
    for seq in (first, second):
        b = ctx.upload(seq, offs)
        r = b.hash_sample128(k, canonical=canonical, drop_last=True, device=True)
        keys = r["values_device"][: r["n"]].contiguous()
        nu = ctx.sort_unique128(keys, key_bits=2 * k)
        m = M.scan(seq.tobytes(), offs, k, 0, canonical, True)
        idx = np.nonzero(m["valid"])[0]
        exp = sorted(set(ints(np.stack([m["lo"][idx], m["hi"][idx]], axis=1))))
        assert r["n"] == len(idx) and nu == len(exp) and ints(host(keys, nu)) == exp
        sets.append((keys, nu))
        models.append(set(exp))
        b.close()
    both = len(models[0] & models[1])
    assert 0 < both < min(len(models[0]), len(models[1]))
    assert ctx.jaccard128(sets[0][0], sets[0][1], sets[1][0], sets[1][1]) == (both, len(models[0] | models[1]))


@pytest.fixture(scope="module")
def owner_keys(pool):
    """50,000 keys with duplicates and their owner hashes at seed 5 (bl_hash64_u128 on the host)"""
    import biolib_amd

    rng = np.random.default_rng(50)
    arr = S.to_array([pool[i] for i in rng.integers(0, len(pool), 50_000)])
    arr[::7] = arr[0]  # heavy duplicates land in one bucket
    hashes = np.array([biolib_amd.hash64_u128(int(lo), int(hi), 5) for lo, hi in arr.tolist()], dtype=np.uint64)
    return arr, hashes


@pytest.mark.parametrize("parts", [1, 3, 64])
def test_partition128(ctx, owner_keys, parts):
    arr, hashes = owner_keys
    out, counts = ctx.partition128(dev(arr), parts, seed=5)
    got = host(out)
    owner = (hashes % np.uint64(parts)).astype(np.int64)
    assert sum(counts) == len(arr) and counts == np.bincount(owner, minlength=parts).tolist()
    edges = np.concatenate([[0], np.cumsum(counts)])
    for b in range(parts):
        assert np.array_equal(lexsorted(got[edges[b]:edges[b + 1]]), lexsorted(arr[owner == b])), (parts, b)


def test_sort_count128(ctx, pool):
    rng = np.random.default_rng(8)
    keys = [pool[i] for i in rng.integers(0, 3000, 40_000)] + [pool[-1]] * 5 + [0] * 3
    t = dev(S.to_array(keys))
    u, c = ctx.sort_count128(t)
    obj = np.empty(len(keys), dtype=object)
    obj[:] = keys
    eu, ec = np.unique(obj, return_counts=True)
    assert ints(host(u)) == eu.tolist() and np.array_equal(c.cpu().numpy().astype(np.int64), ec) and ec.max() > 1
    assert ints(host(t)) == sorted(keys)
    e = ctx.sort_count128(ctx.empty_u128(0), n=0)
    assert e[0].shape[0] == 0 and e[1].numel() == 0


def test_spill_files(ctx, tmp_path):
    from biolib_amd import capi

    L = capi.lib()
    keys = np.load(os.path.join(SP, "keys.npy"))
    exp = lexsorted(keys)
    # the files the reference wrote, read on the device
    assert np.array_equal(host(ctx.read_file_u128(os.path.join(SP, "tmp.run_first_0.bin"))), exp)
    assert np.array_equal(host(ctx.read_file_u128(os.path.join(SP, "vector.bin"), with_count=True)), exp)
    assert np.array_equal(host(ctx.merge_runs128([os.path.join(SP, "tmp.run_first_0.bin")])), exp)
    # written from the device: byte-identical to them
    t = dev(keys)
    ctx.sort128(t, key_bits=82)
    run, vec = str(tmp_path / "run.bin"), str(tmp_path / "vec.bin")
    capi.check(L.bl_write_run_u128(ctx._h, C.c_void_p(t.data_ptr()), len(keys), run.encode()))
    capi.check(L.bl_write_vector_u128(ctx._h, C.c_void_p(t.data_ptr()), len(keys), vec.encode()))
    assert open(run, "rb").read() == open(os.path.join(SP, "tmp.run_first_0.bin"), "rb").read()
    assert open(vec, "rb").read() == open(os.path.join(SP, "vector.bin"), "rb").read()
    # three runs cut from the keys (one of them short, duplicates across runs) merge to the sorted whole
    paths = []
    for i, (lo, hi) in enumerate(((0, 1000), (1000, 1003), (1003, len(keys)))):
        part = dev(keys[lo:hi])
        ctx.sort128(part, key_bits=82)
        p = str(tmp_path / f"tmp.run_x_{i}.bin")
        capi.check(L.bl_write_run_u128(ctx._h, C.c_void_p(part.data_ptr()), hi - lo, p.encode()))
        paths.append(p)
    assert np.array_equal(host(ctx.merge_runs128(paths)), exp)
    empty = tmp_path / "tmp.run_x_3.bin"
    empty.write_bytes(b"")
    assert np.array_equal(host(ctx.merge_runs128(paths[:2] + [str(empty)] + paths[2:])), exp)  # an empty run among them


def test_cpp_compat_jaccard128(tmp_path):
    """tests/cpp/test_compat_jaccard128.cpp with its own compile line (the flags of tests/cpp/Makefile): the Jaccard workflow over the
    drop-in headers with kmer_t = __uint128_t at k = 41"""
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_compat_jaccard128")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "biolib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-pthread", "-I" + os.path.join(ROOT, "include", "compat"),
                           os.path.join(ROOT, "tests", "cpp", "test_compat_jaccard128.cpp"), "-L" + lib, "-lbiolib_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe], timeout=600)
    ing = os.path.join(HERE, "golden", "ingest")
    out = subprocess.run([exe, os.path.join(ing, "many.fa"), os.path.join(ing, "many.fa.gz"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test_compat_jaccard128: OK" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stdout.count(" = 1.000000\n") == 2  # the same sequences, plain and gzip: every set equals itself
    out = subprocess.run([exe, os.path.join(ing, "many.fa"), os.path.join(ing, "mixed.fa"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "test_compat_jaccard128: OK" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
    assert not [f for f in os.listdir(tmp_path) if f.startswith("tmp.run")]  # the vectors removed their run files
