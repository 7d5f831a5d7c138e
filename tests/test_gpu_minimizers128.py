"""GPU tests of bl_scan_minimizers128 (window minimizers of k-mers up to k = 64, the units hashed as 16-byte keys) and of
minimizer_sampler over kmer_view<__uint128_t>, against the independent Python model (tests/minimizers128_model.py).

Shapes: the 13,295-base batch of the 128-bit k-mer tests (3 tiles + 1,007 bases, not a multiple of 16; reads of length 1, k-1, k, k+1, 150
and one of 5,000 that crosses a tile edge, an N every 911 bases, one run of bytes 0x80-0xff), and a second batch of tandem repeats and a
reverse palindrome for ties and strands."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import minimizers128_model as M
from test_gpu_syncmers128 import batch_for, revcomp, tie_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 42
# w = 1, 2, 15, 16, 17, 11, 33, 63, 64, 11: both window forms, their threshold, the largest halo, and ordinary shapes
SHAPES = ((33, 1), (64, 2), (48, 15), (33, 16), (51, 17), (51, 11), (64, 33), (40, 63), (64, 64), (17, 11))
DIGEST = ("count", "xor_value", "aux", "xor_hash", "xor_pos", "redone")


@functools.lru_cache(maxsize=None)
def model(unit, w, canonical, drop_last, width=16):
    seq, offs = batch_for(unit)
    return M.scan(seq.tobytes(), offs, unit, w, SEED, canonical, drop_last, width)


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def same(got, want):
    assert [got[key] for key in DIGEST] == [want[key] for key in DIGEST]
    if "positions" in got:
        assert got["values"].dtype == np.uint64 and got["values"].shape == (want["count"], 2)
        assert np.array_equal(got["values"][:, 0], want["lo"]) and np.array_equal(got["values"][:, 1], want["hi"])
        assert np.array_equal(got["positions"], want["positions"]) and np.array_equal(got["hashes"], want["hashes"])


@pytest.mark.gpu
@pytest.mark.parametrize("unit,w", SHAPES)
def test_records_and_digest_vs_model(ctx, unit, w):
    seq, offs = batch_for(unit)
    b = ctx.upload(seq, offs)
    for canonical in (False, True):
        for drop_last in (False, True):
            m = model(unit, w, canonical, drop_last)
            kw = dict(seed=SEED, canonical=canonical, drop_last=drop_last)
            want = M.minimizers(m)
            assert want["count"] > 0
            whole = b.minimizers128(unit, w, **kw)
            same(whole, want)
            same(b.minimizers128(unit, w, arrays=False, **kw), want)  # count only: the same digest
            # a range that is not 16-aligned and ends inside a tile; a range cut in two just past a tile edge composes to the whole
            same(b.minimizers128(unit, w, first=37, n=8200, **kw), M.minimizers(m, 37, 37 + 8200))
            left, right = b.minimizers128(unit, w, first=0, n=4101, **kw), b.minimizers128(unit, w, first=4101, n=0, **kw)
            same(left, M.minimizers(m, 0, 4101))
            same(right, M.minimizers(m, 4101))
            for key in ("positions", "hashes", "values"):
                assert np.array_equal(np.concatenate([left[key], right[key]]), whole[key])
            assert left["count"] + right["count"] == whole["count"]
            for key in ("xor_value", "aux", "xor_hash", "xor_pos"):
                assert left[key] ^ right[key] == whole[key]
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("unit,w", ((51, 11), (64, 64)))
def test_capacity_origin_alignment(ctx, unit, w):
    import biolib_amd as B
    import torch

    seq, offs = batch_for(unit)
    b = ctx.upload(seq, offs)
    for canonical in (False, True):
        want = M.minimizers(model(unit, w, canonical, False))
        flags = (B.FLAG_CANONICAL if canonical else 0) | B.FLAG_SYNC
        # one record short: BL_ERR_CAPACITY with the full count and digest, nothing written at or beyond capacity
        cap, guard = want["count"] - 1, 0x5A5A5A5A5A5A5A5A
        v = torch.full((cap + 64, 2), guard, dtype=torch.int64, device=ctx.torch_device)
        p = torch.full((cap + 64,), guard, dtype=torch.int64, device=ctx.torch_device)
        h = torch.full((cap + 64,), guard, dtype=torch.int64, device=ctx.torch_device)
        r = B.Result()
        with pytest.raises(B.BiolibError) as e:
            b.minimizers128_raw(unit, w, SEED, flags, values=v, positions=p, hashes=h, capacity=cap, result=r)
        assert e.value.code == -4 and r.status == -4
        assert [int(getattr(r, key)) for key in DIGEST] == [want[key] for key in DIGEST]
        assert np.array_equal(p[:cap].cpu().numpy().view(np.uint64), want["positions"][:cap])
        assert np.array_equal(h[:cap].cpu().numpy().view(np.uint64), want["hashes"][:cap])
        assert np.array_equal(v[:cap].cpu().numpy().view(np.uint64)[:, 0], want["lo"][:cap])
        assert (p[cap:] == guard).all() and (h[cap:] == guard).all() and (v[cap:] == guard).all()
        # the wrapper runs again with the count reported
        same(b.minimizers128(unit, w, seed=SEED, canonical=canonical, capacity=64), want)
        # d_values that is not 16-byte aligned
        odd = torch.empty((2 * want["count"] + 1,), dtype=torch.int64, device=ctx.torch_device)[1:]
        with pytest.raises(B.BiolibError) as e:
            b.minimizers128_raw(unit, w, SEED, flags, values=odd, capacity=want["count"])
        assert e.value.code == -1 and "16-byte aligned" in str(e.value)
    # positions of a batch that is a piece of a longer whole: positions and xor_pos move, nothing else
    base = M.minimizers(model(unit, w, True, False))
    b.set_origin(10**12)
    want = M.minimizers(model(unit, w, True, False), origin=10**12)
    same(b.minimizers128(unit, w, seed=SEED, canonical=True), want)
    same(b.minimizers128(unit, w, seed=SEED, canonical=True, arrays=False), want)
    assert want["xor_pos"] != base["xor_pos"] and all(want[key] == base[key] for key in ("count", "xor_value", "aux", "xor_hash"))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("unit,w", ((64, 11), (34, 5), (33, 64), (40, 3)))
def test_ties_strands_and_palindromes(ctx, unit, w):
    import kmers128_model as K

    seq, offs, pal = tie_batch(unit)
    text = seq.tobytes()
    m = M.scan(text, offs, unit, w, SEED, True, False, 16)
    fwd = K.scan(text, offs, unit, SEED, False, False)
    strand = (m["lo"] != fwd["lo"]) | (m["hi"] != fwd["hi"])  # 1: the canonical value is the reverse complement
    rec = M.minimizers(m)
    # the MODEL says the input exercises these paths: windows with a tied minimum whose occurrence lies on either strand, and a unit
    # that is its own reverse complement inside a record's window
    tied_occ = m["occ"][m["tied"]]
    assert len(tied_occ) and strand[tied_occ].any() and not strand[tied_occ].all()
    if unit % 2 == 0:  # a unit of odd length has a middle base and is never its own reverse complement
        mid = text.index(pal) + (64 - unit) // 2
        assert m["valid"][mid] and text[mid:mid + unit] == revcomp(text[mid:mid + unit]) and not strand[mid]
        assert ((rec["windows"] <= mid) & (mid < rec["windows"] + w)).any()
    # a repeat of period 1: every window's leftmost unit is the minimizer — one record per window
    first_run = np.arange(0, 200 - unit - w + 2)
    assert m["exist"][first_run].all() and np.array_equal(m["occ"][first_run], first_run) and np.isin(first_run, rec["windows"]).all()
    b = ctx.upload(seq, offs)
    for canonical in (True, False):
        mm = m if canonical else M.scan(text, offs, unit, w, SEED, False, False, 16)
        want = M.minimizers(mm)
        assert want["count"] > 0
        same(b.minimizers128(unit, w, seed=SEED, canonical=canonical), want)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", (33, 64))
def test_w1_equals_hash_sample128(ctx, k):
    seq, offs = batch_for(k)
    b = ctx.upload(seq, offs)
    for canonical in (False, True):
        for drop_last in (False, True):
            a = b.minimizers128(k, 1, seed=SEED, canonical=canonical, drop_last=drop_last)
            s = b.hash_sample128(k, seed=SEED, threshold=2**64 - 1, canonical=canonical, drop_last=drop_last)
            assert a["count"] == s["count"] > 0
            for key in ("values", "positions", "hashes"):
                assert np.array_equal(a[key], s[key])
            for key in ("xor_value", "aux", "xor_hash", "xor_pos"):
                assert a[key] == s[key]
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("unit", (31, 32))
def test_units_up_to_32_hash_16_byte_keys(ctx, unit):
    w = 11
    seq, offs = batch_for(unit)
    b = ctx.upload(seq, offs)
    for canonical in (False, True):
        wide = b.minimizers128(unit, w, seed=SEED, canonical=canonical)
        want = M.minimizers(model(unit, w, canonical, False))
        same(wide, want)
        narrow = b.minimizers(unit, w, seed=SEED, canonical=canonical)
        want8 = M.minimizers(model(unit, w, canonical, False, 8))  # the 64-bit call is the model at 8 key bytes
        assert narrow["count"] == want8["count"] and np.array_equal(narrow["positions"], want8["positions"]) and np.array_equal(narrow["values"], want8["lo"])
        # the same units — a zero high word, and every value the 64-bit call's value at that position
        m8 = model(unit, w, canonical, False, 8)
        assert not want["hi"].any() and np.array_equal(want["lo"], m8["lo"][want["positions"].astype(np.int64)])
        assert wide["count"] > 0 and narrow["count"] > 0 and not np.array_equal(wide["positions"], narrow["positions"])
    b.close()


@pytest.mark.gpu
def test_argument_errors(ctx):
    import biolib_amd as B

    seq, offs = batch_for(33)
    b = ctx.upload(seq, offs)
    for unit, w in ((0, 11), (65, 11), (33, 0), (33, 65)):
        with pytest.raises(B.BiolibError) as e:
            b.minimizers128(unit, w)
        assert e.value.code == -1 and "1 <= unit <= 64" in str(e.value) and "1 <= w <= 64" in str(e.value), (unit, w)
        rc = ctx._lib.bl_scan_minimizers128(ctx._h, b._h, 0, 0, unit, w, 0, B.FLAG_SYNC, None, None, None, 0, None)
        assert rc == -1 and b"1 <= unit <= 64" in ctx._lib.bl_last_error()
    other_ctx = B.Context(0)
    foreign = other_ctx.upload(seq, offs)
    rc = ctx._lib.bl_scan_minimizers128(ctx._h, foreign._h, 0, 0, 33, 11, 0, B.FLAG_SYNC, None, None, None, 0, None)
    assert rc == -1 and b"another context" in ctx._lib.bl_last_error()
    with pytest.raises(B.BiolibError):
        b.minimizers(33, 11)  # the 64-bit call keeps its limit
    assert b.minimizers128(64, 64, arrays=False)["count"] > 0
    foreign.close()
    other_ctx.close()
    b.close()


def _build_cpp():
    """tests/cpp/test_compat_minimizer128.cpp with its own compile line (the flags of tests/cpp/Makefile); the library itself is built by
    the session fixture of conftest.py when it is missing"""
    out = os.path.join(ROOT, "tests", "cpp", "_build", "test_compat_minimizer128")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    lib = os.path.join(ROOT, "biolib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-pthread", "-I" + os.path.join(ROOT, "include", "compat"),
                           os.path.join(ROOT, "tests", "cpp", "test_compat_minimizer128.cpp"), "-L" + lib, "-lbiolib_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", out], timeout=600)
    return out


def test_cpp_compat_minimizer128_compiles_and_links():
    """CPU-only twin: minimizer_sampler over the 128-bit view compiles and links against the C ABI"""
    assert os.path.exists(_build_cpp())


def _parse(stdout):
    rows = [ln.split() for ln in stdout.splitlines()]
    return [(int(t[1]), int(t[2]), int(t[3])) for t in rows if t and t[0] == "min"], [int(t[1]) for t in rows if t and t[0] == "count"][0]


@pytest.mark.gpu
def test_cpp_compat_minimizer_sampler_128():
    import oracle_lib as O

    exe = _build_cpp()
    with open(os.path.join(ROOT, "tests", "golden", "kmers128.json")) as f:
        text = json.load(f)["string"]
    assert len(text) == 200
    cuts = np.array([0, len(text)], np.uint64)
    for k, w in ((33, 11), (64, 5)):
        for canonical in (0, 1):
            out = subprocess.run([exe, text, str(k), str(w), str(canonical), "wide"], capture_output=True, text=True, timeout=300)
            assert out.returncode == 0 and "test_compat_minimizer128: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
            got, cnt = _parse(out.stdout)
            # Q1: the sampler's range stops before the last k-mer — the model with drop_last (the sampler hashes with seed 0)
            want = M.minimizers(M.scan(text.encode(), cuts, k, w, 0, bool(canonical), True, 16))
            assert got == list(zip(want["positions"].tolist(), want["lo"].tolist(), want["hi"].tolist())) and cnt == want["count"] > 0, (k, w, canonical)
    # kmer_view<uint64_t> with the same sampler gives what it gave: 8-byte keys, the range without its last k-mer
    for canonical in (0, 1):
        out = subprocess.run([exe, text, "31", "11", str(canonical), "u64"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        got, cnt = _parse(out.stdout)
        v, p, _ = O.minimizers(text[:-1], np.array([0, len(text) - 1], np.uint64), 31, 11, 0, bool(canonical), brute=True)
        assert got == [(int(a), int(b), 0) for a, b in zip(p, v)] and cnt == len(v) > 0
