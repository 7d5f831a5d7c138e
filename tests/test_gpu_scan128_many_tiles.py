"""GPU test of the workgroup glue the 128-bit tile kernels share (biolib_amd/csrc/bl_tile128.hpp) and of their host driver, at the smallest
size where that glue does more than the other tests of these families ask of it: more than 2,048 tiles.  The kernels are launched with
2,048 workgroups, so here four of them take a second tile (the barrier in front of a tile's staging guards the previous tile's LDS) and
the last four tiles lie in the second block of the tile prefix scan (block_base[1]).

Shapes: the 13,295-base block of the 128-bit k-mer tests (3 tiles + 1,007 bases; reads of length 1, k-1, k, k+1, 150 and one that crosses a
tile edge, an N every 911 bases, bytes >= 0x80), a block of whole reads, laid end to end 632 times: 8,402,440 bases = 2,052 tiles.
13,295 mod 16 = 15: every repetition meets the lanes and the tiles at another alignment.  No record crosses a sequence, so the expected
result is the Python model's result on ONE block, repeated at the offsets r * 13,295; nothing expected comes from the library."""
import functools

import numpy as np
import pytest

import kmers128_model as K
import minimizers128_model as MM
import syncmers128_model as SM
from test_gpu_syncmers128 import N, SEED, batch_for

H = 4096
REPS = 632
TOTAL = N * REPS
K_DENSE = 51
GUARD = 0x5A5A5A5A5A5A5A5A
FAMILIES = ("hash_sample128", "syncmers128", "minimizers128")


def xr(a):
    return int(np.bitwise_xor.reduce(a)) if len(a) else 0


def tiled_positions(pos):
    """the block's positions at every repetition's offset, in batch order"""
    return (np.arange(REPS, dtype=np.uint64)[:, None] * np.uint64(N) + pos[None, :]).ravel()


@functools.lru_cache(maxsize=None)
def upload_args(k):
    seq, offs = batch_for(k)
    assert int(offs[0]) == 0 and int(offs[-1]) == N  # whole reads: a repetition starts a sequence
    starts = (np.arange(REPS, dtype=np.uint64)[:, None] * np.uint64(N) + offs[None, :-1]).ravel()
    return np.tile(seq, REPS), np.append(starts, np.uint64(TOTAL))


@functools.lru_cache(maxsize=None)
def expected(family):
    """the model on one block, repeated: dict of the record fields (numpy uint64) and the digest words"""
    if family == "hash_sample128":
        seq, offs = batch_for(51)
        one = K.sample(K.scan(seq.tobytes(), offs, 51, SEED, True, False), 2**60)
    elif family == "syncmers128":
        seq, offs = batch_for(33)
        one = SM.syncmers(SM.scan(seq.tobytes(), offs, 33, 11, SEED, True, False, 16), 0, 33 - 11)
    else:
        seq, offs = batch_for(51)
        one = MM.minimizers(MM.scan(seq.tobytes(), offs, 51, 11, SEED, True, False, 16))
    assert one["count"] > 0
    want = dict(count=one["count"] * REPS, positions=tiled_positions(one["positions"]))
    for key in ("lo", "hi", "hashes"):
        want[key] = np.tile(one[key], REPS) if key in one else None
    want["xor_pos"] = xr(want["positions"])
    # an even number of repetitions: the XORs of values and hashes cancel (the arrays themselves are compared word by word)
    assert REPS % 2 == 0
    want.update(xor_value=0, aux=0, xor_hash=0)
    return want


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def test_shape_reaches_the_second_scan_block():
    assert N % 16 == 15 and TOTAL == 8_402_440 and (TOTAL - 1) // H + 1 == 2052 > 2048


@pytest.mark.gpu
def test_dense_scan_many_tiles(ctx):
    seq, offs = upload_args(K_DENSE)
    block, block_offs = batch_for(K_DENSE)
    one = K.scan(block.tobytes(), block_offs, K_DENSE, SEED, True, False)
    want = {key: np.tile(one[key], REPS) for key in ("lo", "hi", "hashes", "valid")}
    d = K.digest(want)
    assert d["count"] == REPS * int(one["valid"].sum()) > 0
    b = ctx.upload(seq, offs)
    got = b.kmers128(K_DENSE, seed=SEED, canonical=True)
    for key in ("count", "xor_value", "aux", "xor_hash", "sum_hash"):
        assert got[key] == d[key], key
    assert got["values"].shape == (TOTAL, 2)
    assert np.array_equal(got["values"][:, 0], want["lo"]) and np.array_equal(got["values"][:, 1], want["hi"])
    assert np.array_equal(got["hashes"], want["hashes"]) and np.array_equal(got["valid"], want["valid"])
    without = b.kmers128(K_DENSE, seed=SEED, canonical=True, arrays=False)
    assert all(without[key] == d[key] for key in d)
    b.close()


def run_raw(ctx, b, family, cap):
    """the family's raw call into buffers of cap records and 64 guard records behind them: (error code or 0, Result, dict of host arrays)"""
    import biolib_amd as B
    import torch

    flags = B.FLAG_CANONICAL | B.FLAG_SYNC
    full = lambda *shape: torch.full(shape, GUARD, dtype=torch.int64, device=ctx.torch_device)
    r = B.Result()
    code = 0
    if family == "syncmers128":
        bufs = dict(positions=full(cap + 64))
        call = lambda: b.syncmers128_raw(33, 11, 0, 33 - 11, SEED, flags, positions=bufs["positions"], capacity=cap, result=r)
    else:
        bufs = dict(values=full(cap + 64, 2), positions=full(cap + 64), hashes=full(cap + 64))
        if family == "hash_sample128":
            call = lambda: b.hash_sample128_raw(51, SEED, 2**60, flags, capacity=cap, result=r, **bufs)
        else:
            call = lambda: b.minimizers128_raw(51, 11, SEED, flags, capacity=cap, result=r, **bufs)
    try:
        call()
    except B.BiolibError as e:
        code = e.code
    return code, r, {key: t.cpu().numpy().view(np.uint64) for key, t in bufs.items()}


def check_records(host, want, n):
    """the first n records word by word, every word behind them the guard"""
    assert np.array_equal(host["positions"][:n], want["positions"][:n]) and (host["positions"][n:] == GUARD).all()
    if "values" in host:
        assert np.array_equal(host["values"][:n, 0], want["lo"][:n]) and np.array_equal(host["values"][:n, 1], want["hi"][:n])
        assert np.array_equal(host["hashes"][:n], want["hashes"][:n])
        assert (host["values"][n:] == GUARD).all() and (host["hashes"][n:] == GUARD).all()


def check_digest(r, want):
    for key in ("count", "xor_value", "aux", "xor_hash", "xor_pos"):
        assert int(getattr(r, key)) == want[key], key


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_two_pass_scan_many_tiles(ctx, family):
    want = expected(family)
    need = want["count"]
    seq, offs = upload_args(33 if family == "syncmers128" else 51)
    b = ctx.upload(seq, offs)
    # the records of the last four tiles are placed through block_base[1]
    assert (want["positions"] >= 2048 * H).any()
    code, r, host = run_raw(ctx, b, family, need)
    assert code == 0 and r.status == 0
    check_digest(r, want)
    check_records(host, want, need)
    # half the room: BL_ERR_CAPACITY with the full count and digest, the first `cap` records, nothing behind them
    cap = need // 2
    code, r, host = run_raw(ctx, b, family, cap)
    assert code == -4 and r.status == -4
    check_digest(r, want)
    check_records(host, want, cap)
    b.close()
