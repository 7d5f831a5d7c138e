"""GPU tests of bl_scan_syncmers128 (syncmers of k-mers up to k = 64, s-mers up to 32 hashed as 16-byte keys) and of syncmer_sampler over
kmer_view<__uint128_t>, against the independent Python model (tests/syncmers128_model.py) and tests/golden/syncmers128.json.

Shapes: the 13,295-base batch of the 128-bit k-mer tests (3 tiles + 1,007 bases, not a multiple of 16; reads of length 1, k-1, k, k+1, 150
and one of 5,000 that crosses a tile edge, an N every 911 bases, one run of bytes 0x80-0xff), and a second batch of tandem repeats and a
reverse palindrome for ties and strands."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import syncmers128_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4096
N = 3 * H + 1007
SEED = 42
# W = 2, 1, 16, 32, 18, 41, 33, 63, 64, 15
SHAPES = ((33, 32), (32, 32), (47, 32), (48, 17), (49, 32), (51, 11), (64, 32), (64, 2), (64, 1), (17, 3))


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
def model(k, s, canonical, drop_last, width=16):
    seq, offs = batch_for(k)
    return M.scan(seq.tobytes(), offs, k, s, SEED, canonical, drop_last, width)


def offset_pairs(w):
    return ((0, w - 1), (2, 5), (3, 3), (w, 65535))


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "syncmers128.json")) as f:
        return json.load(f)


def same(got, want):
    assert got["count"] == want["count"] and got["xor_pos"] == want["xor_pos"]
    assert got["xor_value"] == 0 and got["xor_hash"] == 0 and got["aux"] == 0
    if "positions" in got:
        assert got["positions"].dtype == np.uint64 and np.array_equal(got["positions"], want["positions"])


@pytest.mark.gpu
@pytest.mark.parametrize("k,s", SHAPES)
def test_positions_and_digest_vs_model(ctx, k, s):
    seq, offs = batch_for(k)
    b = ctx.upload(seq, offs)
    w = k - s + 1
    for canonical in (False, True):
        for drop_last in (False, True):
            m = model(k, s, canonical, drop_last)
            kw = dict(seed=SEED, canonical=canonical, drop_last=drop_last)
            for a, e in offset_pairs(w):
                want = M.syncmers(m, a, e)
                got = b.syncmers128(k, s, a, e, **kw)
                same(got, want)
                if want["count"] > 0:
                    assert got["count"] > 0
                if a >= w:
                    assert got["count"] == 0 and len(got["positions"]) == 0
                same(b.syncmers128(k, s, a, e, positions=False, **kw), want)  # count only: the same count and xor_pos
            assert M.syncmers(m, 0, w - 1)["count"] > 0
            # a range that is not 16-aligned and ends inside a tile; a range cut in two composes to the whole
            a, e = 0, w - 1
            same(b.syncmers128(k, s, a, e, first=37, n=8200, **kw), M.syncmers(m, a, e, 37, 37 + 8200))
            whole = b.syncmers128(k, s, a, e, **kw)
            left, right = b.syncmers128(k, s, a, e, first=0, n=4101, **kw), b.syncmers128(k, s, a, e, first=4101, n=0, **kw)
            same(left, M.syncmers(m, a, e, 0, 4101))
            assert np.array_equal(np.concatenate([left["positions"], right["positions"]]), whole["positions"])
            assert left["count"] + right["count"] == whole["count"] and left["xor_pos"] ^ right["xor_pos"] == whole["xor_pos"]
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,s", ((51, 11), (64, 32)))
def test_capacity_origin(ctx, k, s):
    import biolib_amd as B
    import torch

    seq, offs = batch_for(k)
    b = ctx.upload(seq, offs)
    w = k - s + 1
    for canonical in (False, True):
        want = M.syncmers(model(k, s, canonical, False), 0, w - 1)
        # one record short: BL_ERR_CAPACITY with the full count, nothing written at or beyond capacity
        cap, guard = want["count"] - 1, 0x5A5A5A5A5A5A5A5A
        p = torch.full((cap + 64,), guard, dtype=torch.int64, device=ctx.torch_device)
        r = B.Result()
        with pytest.raises(B.BiolibError) as e:
            b.syncmers128_raw(k, s, 0, w - 1, SEED, (B.FLAG_CANONICAL if canonical else 0) | B.FLAG_SYNC, positions=p, capacity=cap, result=r)
        assert e.value.code == -4 and r.count == want["count"] and r.status == -4 and r.xor_pos == want["xor_pos"]
        assert np.array_equal(p[:cap].cpu().numpy().view(np.uint64), want["positions"][:cap])
        assert (p[cap:] == guard).all()
        # the wrapper runs again with the count reported
        same(b.syncmers128(k, s, 0, w - 1, seed=SEED, canonical=canonical, capacity=64), want)
    # positions of a batch that is a piece of a longer whole
    b.set_origin(10**12)
    want = M.syncmers(model(k, s, True, False), 0, w - 1, origin=10**12)
    same(b.syncmers128(k, s, 0, w - 1, seed=SEED, canonical=True), want)
    same(b.syncmers128(k, s, 0, w - 1, seed=SEED, canonical=True, positions=False), want)
    assert want["xor_pos"] != M.syncmers(model(k, s, True, False), 0, w - 1)["xor_pos"]
    b.close()


def revcomp(t):
    return t[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def tie_batch(k):
    """tandem repeats of period 1, 2, 3 and 7 in both orientations, a reverse palindrome x + revcomp(x) of 64 bases, reads of length
    k - 1 (= W + s - 2: one base short of a k-mer) and k; every piece a read of its own, then all of them again inside one read"""
    rng = np.random.default_rng(11)
    rnd = lambda n: rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()
    units = [b"A", b"AC", b"ACG", b"ACGGTCA"]
    pieces = []
    for u in units:
        for rep in (u, revcomp(u)):
            pieces.append(rep * (200 // len(rep)))
    x = rnd(32)
    pal = x + revcomp(x)
    assert pal == revcomp(pal) and len(pal) == 64
    pieces += [rnd(40) + pal + rnd(40), pal, rnd(k - 1), rnd(k)]
    joined = b"".join(p + rnd(70) for p in pieces)
    text = b"".join(pieces) + joined
    offs = np.cumsum([0] + [len(p) for p in pieces] + [len(joined)]).astype(np.uint64)
    return np.frombuffer(text, np.uint8).copy(), offs, pal


@pytest.mark.gpu
@pytest.mark.parametrize("k,s", ((64, 32), (64, 3), (34, 5), (34, 20)))
def test_ties_strands_and_palindromes(ctx, k, s):
    seq, offs, pal = tie_batch(k)
    text = seq.tobytes()
    w = k - s + 1
    m = M.scan(text, offs, k, s, SEED, True, False, 16)
    ok = m["valid"] == 1
    # the MODEL says the input exercises these paths: tied minima on either strand, and a k-mer that is its own reverse complement
    assert (ok & m["tied"] & (m["strand"] == 1)).any() and (ok & m["tied"] & (m["strand"] == 0)).any()
    mid = text.index(pal) + (64 - k) // 2
    assert ok[mid] and text[mid:mid + k] == revcomp(text[mid:mid + k]) and m["strand"][mid] == 0
    b = ctx.upload(seq, offs)
    for canonical in (True, False):
        mm = m if canonical else M.scan(text, offs, k, s, SEED, False, False, 16)
        for a, e in ((0, w - 1), (1, 2), (w - 2, w // 2)):
            want = M.syncmers(mm, a, e)
            same(b.syncmers128(k, s, a, e, seed=SEED, canonical=canonical), want)
            assert want["count"] > 0
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", (31, 32))
def test_k_up_to_32_hashes_16_byte_keys(ctx, k):
    s = 11
    seq, offs = batch_for(k)
    b = ctx.upload(seq, offs)
    for canonical in (False, True):
        wide = b.syncmers128(k, s, 0, k - s, seed=SEED, canonical=canonical, drop_last=True)
        same(wide, M.syncmers(model(k, s, canonical, True), 0, k - s))
        narrow = b.syncmers(k, s, 0, k - s, seed=SEED, canonical=canonical, drop_last=True)
        want8 = M.syncmers(model(k, s, canonical, True, 8), 0, k - s)  # the 64-bit call is the model at 8 key bytes
        assert narrow["count"] == want8["count"] and np.array_equal(narrow["positions"], want8["positions"])
        assert wide["count"] > 0 and narrow["count"] > 0 and not np.array_equal(wide["positions"], narrow["positions"])
    b.close()


@pytest.mark.gpu
def test_argument_errors(ctx):
    import biolib_amd as B

    seq, offs = batch_for(33)
    b = ctx.upload(seq, offs)
    for k, s in ((0, 1), (65, 11), (33, 0), (64, 33), (20, 21)):
        with pytest.raises(B.BiolibError) as e:
            b.syncmers128(k, s, 0, 0)
        assert e.value.code == -1 and "1 <= s <= 32" in str(e.value) and "k <= 64" in str(e.value), (k, s)
        rc = ctx._lib.bl_scan_syncmers128(ctx._h, b._h, 0, 0, k, s, 0, 0, 0, B.FLAG_SYNC, None, 0, None)
        assert rc == -1 and b"s <= k <= 64" in ctx._lib.bl_last_error()
    other_ctx = B.Context(0)
    foreign = other_ctx.upload(seq, offs)
    rc = ctx._lib.bl_scan_syncmers128(ctx._h, foreign._h, 0, 0, 33, 11, 0, 22, 0, B.FLAG_SYNC, None, 0, None)
    assert rc == -1 and b"another context" in ctx._lib.bl_last_error()
    with pytest.raises(B.BiolibError):
        b.syncmers(33, 11, 0, 22)  # the 64-bit call keeps its limit
    assert b.syncmers128(64, 32, 0, 32, positions=False)["count"] > 0
    foreign.close()
    other_ctx.close()
    b.close()


def _build_cpp():
    """tests/cpp/test_compat_syncmer128.cpp with its own compile line (the flags of tests/cpp/Makefile); the library itself is built by
    the session fixture of conftest.py when it is missing"""
    out = os.path.join(ROOT, "tests", "cpp", "_build", "test_compat_syncmer128")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "biolib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-pthread", "-I" + os.path.join(ROOT, "include", "compat"),
                           os.path.join(ROOT, "tests", "cpp", "test_compat_syncmer128.cpp"), "-L" + lib, "-lbiolib_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", out], timeout=600)
    return out


def test_cpp_compat_syncmer128_compiles_and_links():
    """CPU-only twin: syncmer_sampler and the host extractor over the 128-bit view compile and link against the C ABI"""
    assert os.path.exists(_build_cpp())


def _parse(stdout):
    off = [(int(t[1]), int(t[2])) for t in (ln.split() for ln in stdout.splitlines()) if t and t[0] == "off"]
    syn = [(int(t[1]), int(t[2])) for t in (ln.split() for ln in stdout.splitlines()) if t and t[0] == "syn"]
    cnt = [int(t[1]) for t in (ln.split() for ln in stdout.splitlines()) if t and t[0] == "count"]
    return off, syn, cnt[0]


@pytest.mark.gpu
def test_cpp_compat_syncmer_sampler_128(golden):
    import kmers128_model as K
    import oracle_lib as O

    exe = _build_cpp()
    text = golden["strings"]["s200"]
    cuts = np.array([0, len(text)], np.uint64)
    for k, s in ((33, 11), (64, 32)):
        for name, canonical in (("forward", 0), ("canonical", 1)):
            e = golden["cases"]["s200"][f"{k},{s}"][name]
            a, z = e["closed"]["offsets"]
            out = subprocess.run([exe, text, str(k), str(s), str(a), str(z), str(canonical), "wide"], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0 and "test_compat_syncmer128: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
            off, syn, cnt = _parse(out.stdout)
            assert off == list(zip(e["positions"], e["offsets"])), (k, s, name)  # the host extractor, the last k-mer included
            want = [p for p in e["closed"]["positions"] if p != len(text) - k]    # Q1: the sampler's range stops before the last k-mer
            assert [p for p, _ in syn] == want and cnt == len(want) > 0, (k, s, name)
            km = K.scan(text.encode(), cuts, k, 0, bool(canonical), False)
            assert [v for _, v in syn] == [int(km["lo"][p]) for p in want]         # operator*: the k-mer's low word
    # kmer_view<uint64_t> with the same sampler gives what it gave: 8-byte keys
    for canonical in (0, 1):
        out = subprocess.run([exe, text, "31", "11", "0", "20", str(canonical), "u64"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        off, syn, cnt = _parse(out.stdout)
        n, pos = O.syncmers(text, cuts, 31, 11, 0, 20, bool(canonical), True)
        assert [p for p, _ in syn] == pos.tolist() and cnt == n > 0
        m8 = M.scan(text.encode(), cuts, 31, 11, 0, bool(canonical), False, 8)
        idx = np.nonzero(m8["valid"])[0]
        assert off == list(zip(idx.tolist(), m8["offset"][idx].tolist()))
