"""GPU tests of the 128-bit k-mer scans (bl_scan_kmers128, bl_scan_hash_sample128, kmer_view<__uint128_t>) against the independent
Python model (tests/kmers128_model.py) and the golden file tests/golden/kmers128.json.

Shapes: one batch of 3 tiles + 1,007 bases (13,295; not a multiple of 16) whose offsets hold reads of length 1, k-1, k, k+1, 150 and one
of 5,000 that crosses a tile edge, an N every 911 bases and one run of bytes 0x80-0xff."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import kmers128_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4096
N = 3 * H + 1007
SEED = 42
FULL = 2**64 - 1


@functools.lru_cache(maxsize=None)
def batch_for(k, variant=0):
    rng = np.random.default_rng(7 + variant)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), N)
    seq[np.arange(300, N, 1300)] = ord("t")
    seq[np.arange(301, N, 1300)] = ord("u")
    seq[911::911] = ord("N")
    seq[6000:6010] = np.arange(0x80, 0x100, 13, dtype=np.uint8)[:10]
    offs = [0]
    for length in (1, max(k - 1, 1), k, k + 1, 150):
        offs.append(offs[-1] + length)
    offs += [3000, 8000, 8000 + k, N]  # [3000, 8000) crosses the edge of tile 0
    return seq, np.array(offs, np.uint64)


@functools.lru_cache(maxsize=None)
def model(k, canonical, drop_last, variant=0):
    seq, offs = batch_for(k, variant)
    return M.scan(seq.tobytes(), offs, k, SEED, canonical, drop_last)


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "kmers128.json")) as f:
        return json.load(f)


def check_dense(got, m, first, end):
    d = M.digest(m, first, end)
    for key in ("count", "xor_value", "aux", "xor_hash", "sum_hash"):
        assert got[key] == d[key], key
    assert got["values"].shape == (end - first, 2) and got["values"].dtype == np.uint64
    assert np.array_equal(got["values"][:, 0], m["lo"][first:end]) and np.array_equal(got["values"][:, 1], m["hi"][first:end])
    assert np.array_equal(got["hashes"], m["hashes"][first:end]) and np.array_equal(got["valid"], m["valid"][first:end])


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 32, 33, 48, 49, 63, 64))
def test_dense_scan_vs_model(ctx, k):
    seq, offs = batch_for(k)
    b = ctx.upload(seq, offs)
    for canonical in (False, True):
        for drop_last in (False, True):
            m = model(k, canonical, drop_last)
            kw = dict(seed=SEED, canonical=canonical, drop_last=drop_last)
            whole = b.kmers128(k, **kw)
            check_dense(whole, m, 0, N)
            assert whole["count"] > 0
            check_dense(b.kmers128(k, first=37, n=8200, **kw), m, 37, 37 + 8200)  # not 16-aligned, ends inside a tile
            left, right = b.kmers128(k, first=0, n=4101, **kw), b.kmers128(k, first=4101, n=0, **kw)
            for key in ("values", "hashes", "valid"):
                assert np.array_equal(np.concatenate([left[key], right[key]]), whole[key]), key
            assert left["count"] + right["count"] == whole["count"] and left["xor_hash"] ^ right["xor_hash"] == whole["xor_hash"]
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 31, 32))
def test_agrees_with_the_64bit_scan_up_to_32(ctx, k):
    import biolib_amd

    seq, offs = batch_for(k)
    b = ctx.upload(seq, offs)
    for canonical in (False, True):
        narrow = b.kmers(k, seed=SEED, canonical=canonical, drop_last=True)
        wide = b.kmers128(k, seed=SEED, canonical=canonical, drop_last=True)
        assert np.array_equal(wide["valid"], narrow["valid"]) and narrow["count"] == wide["count"] > 0
        assert np.array_equal(wide["values"][:, 0], narrow["values"]) and not wide["values"][:, 1].any()
        want = np.array([biolib_amd.hash64_u128(v, 0, SEED) if ok else 0 for v, ok in zip(narrow["values"].tolist(), narrow["valid"].tolist())], np.uint64)
        assert np.array_equal(wide["hashes"], want)
        assert not np.array_equal(wide["hashes"], narrow["hashes"])  # 16 key bytes against 8: the reference's hash depends on KmerType
    b.close()


@pytest.mark.gpu
def test_digest_only_call(ctx):
    clean_seq = np.random.default_rng(3).choice(np.frombuffer(b"ACGT", np.uint8), 3000)  # one sequence, no break: wave 0 takes the unmasked path
    for k in (33, 64):
        seq, offs = batch_for(k)
        b = ctx.upload(seq, offs)
        clean = ctx.upload(clean_seq)
        for batch, first, n in ((b, 0, 0), (b, 37, 8200), (clean, 0, 0)):
            for canonical in (False, True):
                with_arrays = batch.kmers128(k, seed=SEED, canonical=canonical, first=first, n=n)
                without = batch.kmers128(k, seed=SEED, canonical=canonical, first=first, n=n, arrays=False)
                assert "values" not in without
                for key in ("count", "xor_value", "aux", "xor_hash", "sum_hash"):
                    assert without[key] == with_arrays[key], (k, key)
                if batch is clean:
                    d = M.digest(M.scan(clean_seq.tobytes(), [0, len(clean_seq)], k, SEED, canonical, False))
                    assert all(without[key] == d[key] for key in d) and d["count"] == len(clean_seq) - k + 1
        b.close()
        clean.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", (33, 51, 64))
def test_sampler_vs_model(ctx, k):
    import biolib_amd as B

    seq, offs = batch_for(k)
    b = ctx.upload(seq, offs)

    def same(got, want):
        for key in ("count", "xor_value", "aux", "xor_hash", "xor_pos"):
            assert got[key] == want[key], key
        assert got["values"].shape == (want["count"], 2)
        assert np.array_equal(got["values"][:, 0], want["lo"]) and np.array_equal(got["values"][:, 1], want["hi"])
        assert np.array_equal(got["positions"], want["positions"]) and np.array_equal(got["hashes"], want["hashes"])

    for canonical in (False, True):
        # everything below the largest threshold, with drop_last: the records of the dense scan where valid
        m = model(k, canonical, True)
        dense = b.kmers128(k, seed=SEED, canonical=canonical, drop_last=True)
        full = b.hash_sample128(k, seed=SEED, threshold=FULL, canonical=canonical, drop_last=True)
        keep = dense["valid"] == 1
        assert full["count"] == dense["count"] > 0
        assert np.array_equal(full["values"], dense["values"][keep]) and np.array_equal(full["hashes"], dense["hashes"][keep])
        assert np.array_equal(full["positions"], np.nonzero(keep)[0].astype(np.uint64))
        same(full, M.sample(m, FULL))
        # a sixteenth of the hash space
        m = model(k, canonical, False)
        want = M.sample(m, 2**60)
        got = b.hash_sample128(k, seed=SEED, threshold=2**60, canonical=canonical)
        same(got, want)
        assert 0 < got["count"] < N // 4 and np.all(np.diff(got["positions"].astype(np.int64)) > 0)
        # nothing is below 0
        none = b.hash_sample128(k, seed=SEED, threshold=0, canonical=canonical)
        assert none["count"] == 0 and len(none["positions"]) == 0 and none["xor_hash"] == 0
        # a range cut in two composes to the whole
        left = b.hash_sample128(k, seed=SEED, threshold=2**60, canonical=canonical, first=0, n=4101)
        right = b.hash_sample128(k, seed=SEED, threshold=2**60, canonical=canonical, first=4101)
        same(left, M.sample(m, 2**60, 0, 4101))
        for key in ("values", "positions", "hashes"):
            assert np.array_equal(np.concatenate([left[key], right[key]]), got[key]), key
        # one record short: BL_ERR_CAPACITY with the full count, nothing written at or beyond capacity
        import torch

        cap, guard = want["count"] - 1, 0x5A5A5A5A5A5A5A5A
        v = torch.full((cap + 4, 2), guard, dtype=torch.int64, device=ctx.torch_device)
        p = torch.full((cap + 4,), guard, dtype=torch.int64, device=ctx.torch_device)
        h = torch.full((cap + 4,), guard, dtype=torch.int64, device=ctx.torch_device)
        r = B.Result()
        with pytest.raises(B.BiolibError) as e:
            b.hash_sample128_raw(k, SEED, 2**60, (B.FLAG_CANONICAL if canonical else 0) | B.FLAG_SYNC, values=v, positions=p, hashes=h, capacity=cap, result=r)
        assert e.value.code == -4 and r.count == want["count"] and r.status == -4
        assert np.array_equal(p[:cap].cpu().numpy().view(np.uint64), want["positions"][:cap])
        assert np.array_equal(v[:cap, 0].cpu().numpy().view(np.uint64), want["lo"][:cap])
        assert (v[cap:] == guard).all() and (p[cap:] == guard).all() and (h[cap:] == guard).all()
    # positions of a batch that is a piece of a longer whole
    b.set_origin(10**12)
    moved = b.hash_sample128(k, seed=SEED, threshold=2**60, canonical=True)
    same(moved, M.sample(model(k, True, False), 2**60, origin=10**12))
    b.close()


@pytest.mark.gpu
def test_workflow_sample_sort_unique_jaccard(ctx):
    k, thr = 51, 2**61
    sets, tensors = [], []
    seq, offs = batch_for(k)
    other = seq.copy()
    rot = np.arange(256, dtype=np.uint8)
    rot[list(b"ACGT")] = list(b"CGTA")
    other[25::50] = rot[other[25::50]]  # every 50th base substituted
    for s in (seq, other):
        b = ctx.upload(s, offs)
        got = b.hash_sample128(k, seed=SEED, threshold=thr, canonical=True, device=True)
        n = ctx.sort_unique(got["hashes_device"], got["n"])
        tensors.append((got["hashes_device"], n))
        m = M.scan(s.tobytes(), offs, k, SEED, True, False)
        sets.append(set(M.sample(m, thr)["hashes"].tolist()))
        assert n == len(sets[-1]) > 0
        b.close()
    inter, union = ctx.jaccard(tensors[0][0], tensors[0][1], tensors[1][0], tensors[1][1])
    # (a substitution every 50 bases leaves no 51-mer untouched: the two sets are disjoint, and the device says so too)
    assert (inter, union) == (len(sets[0] & sets[1]), len(sets[0] | sets[1])) and union > 0


@pytest.mark.gpu
def test_argument_errors(ctx):
    import biolib_amd as B

    seq, offs = batch_for(33)
    b = ctx.upload(seq, offs)
    other_ctx = B.Context(0)
    foreign = other_ctx.upload(seq, offs)
    for bad in (0, 65):
        with pytest.raises(B.BiolibError) as e:
            b.kmers128(bad)
        assert e.value.code == -1 and "k must be" in str(e.value)
        with pytest.raises(B.BiolibError) as e:
            b.hash_sample128(bad)
        assert e.value.code == -1 and "k must be" in str(e.value)
    for call in (ctx._lib.bl_scan_kmers128, ):
        rc = call(ctx._h, foreign._h, 0, 0, 33, 0, B.FLAG_SYNC, None, None, None, None)
        assert rc == -1 and b"another context" in ctx._lib.bl_last_error()
    rc = ctx._lib.bl_scan_hash_sample128(ctx._h, foreign._h, 0, 0, 33, 0, FULL, B.FLAG_SYNC, None, None, None, 0, None)
    assert rc == -1 and b"another context" in ctx._lib.bl_last_error()
    with pytest.raises(B.BiolibError):
        b.kmers(33)  # the 64-bit scan keeps its limit
    assert b.kmers128(64, arrays=False)["count"] > 0
    foreign.close()
    other_ctx.close()
    b.close()


def _build_cpp():
    """tests/cpp/test_compat_kmer128.cpp with its own compile line (the flags of tests/cpp/Makefile); the library itself is built by
    the session fixture of conftest.py when it is missing"""
    out = os.path.join(ROOT, "tests", "cpp", "_build", "test_compat_kmer128")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "biolib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-pthread", "-I" + os.path.join(ROOT, "include", "compat"),
                           os.path.join(ROOT, "tests", "cpp", "test_compat_kmer128.cpp"), "-L" + lib, "-lbiolib_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", out], timeout=600)
    return out


def test_cpp_compat_kmer128_compiles_and_links():
    """CPU-only twin: the 128-bit instantiation of the drop-in view compiles and links against the C ABI"""
    assert os.path.exists(_build_cpp())


def _parse(stdout):
    loop, last, mask = [], None, None
    for ln in stdout.splitlines():
        t = ln.split()
        if t[0] == "last":
            last = [int(t[1]), int(t[2])] + ([None, None] if t[3] == "null" else [int(t[3]), int(t[4])])
        elif t[0] == "mask":
            mask = int(t[1]) | (int(t[2]) << 64)
        elif t[0].isdigit():
            loop.append([int(t[0]), int(t[1])] + ([None, None] if t[2] == "null" else [int(t[2]), int(t[3])]))
    return loop, last, mask


@pytest.mark.gpu
def test_cpp_compat_kmer_view_128(golden):
    import oracle_lib as O

    exe = _build_cpp()
    s = golden["string"]
    for k in (33, 64):
        for name, canonical in (("forward", 0), ("canonical", 1)):
            out = subprocess.run([exe, s, str(k), str(canonical), "wide"], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0 and "test_compat_kmer128: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
            loop, last, mask = _parse(out.stdout)
            want = golden["items"][str(k)][name]
            assert loop == want["loop"] and last == want["last"], (k, name)  # items, positions, ids, nulls; Q1: the last k-mer is not in the loop
            assert any(item[2] is None for item in loop) and mask == (1 << (2 * k)) - 1
    # kmer_view<uint64_t> gives what it gave
    for canonical in (0, 1):
        out = subprocess.run([exe, s, "31", str(canonical), "u64"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        loop, last, mask = _parse(out.stdout)
        assert [(p, i, lo) for p, i, lo, _ in loop] == O.kmer_items(s, 31, bool(canonical), False) and mask == (1 << 62) - 1
        assert all(hi in (0, None) for _, _, _, hi in loop)
