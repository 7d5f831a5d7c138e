"""Every kernel that decides on murmur64_top (bl_scan_core.hpp) against the CPU oracle, records materialised: the read-tiled (31, 11)
kernels (150 bp fully specialised; 14 and 16 units per lane with run-time geometry), the position-tiled one, and the closed-syncmer
form.  Each case on random bases and on a batch of period-3 repeats, where every window holds a key twice and every tile is handed to
the exact kernels.  Small on purpose: one read, one tile of 32 reads, a second ragged tile."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

K, W, SEED = 31, 11, 42


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.set_exact_windows(False)
    c.close()


def bases(flavour, seed, n):
    if flavour == "repeats":
        return np.resize(np.frombuffer(b"ACG", np.uint8), n).copy()
    return O.synth(seed, n).copy()


def scan_minimizers(ctx, b, cap):
    import biolib_amd as B

    v, p, h = ctx.empty_u64(cap), ctx.empty_u64(cap), ctx.empty_u64(cap)
    r = b.minimizers_raw(K, W, SEED, B.FLAG_CANONICAL | B.FLAG_SYNC, values=v, positions=p, hashes=h, capacity=cap)
    n = int(r.count)
    assert n <= cap
    host = lambda t: t[:n].cpu().numpy().view(np.uint64)  # the device words are 64-bit unsigned in int64 tensors
    return r.as_dict(), int(r.redone), host(v), host(p), host(h)


def check_minimizers(ctx, seq, offs, read_len, want_redo, exact_too=False):
    v, p, h = O.minimizers(seq, offs, K, W, SEED, True, brute=False)
    want = O.minimizer_digest(seq, offs, K, W, SEED, True)
    assert want["count"] == len(v)
    b = ctx.upload(seq, read_len=read_len) if read_len else ctx.upload(seq, offs)
    try:
        for exact in (False, True) if exact_too else (False,):
            ctx.set_exact_windows(exact)
            d, redone, gv, gp, gh = scan_minimizers(ctx, b, len(v) + 64)
            assert (d["count"], d["xor_value"], d["xor_hash"], d["xor_pos"]) == (want["count"], want["xor_value"], want["xor_hash"], want["xor_pos"]), exact
            assert np.array_equal(gv, v) and np.array_equal(gp, p) and np.array_equal(gh, h), exact
            if exact:
                assert redone == 0
            elif want_redo:
                assert redone > 0
    finally:
        ctx.set_exact_windows(False)
        b.close()


@pytest.mark.parametrize("flavour", ["random", "repeats"])
@pytest.mark.parametrize("n_reads", [1, 32, 33])
def test_c3_reads_of_150(ctx, n_reads, flavour):
    """scan_count_frl_kernel<0,11,15,31,150,1,true>: one read, one tile, a second ragged tile; the same batch with exact_windows = 1"""
    n = 150 * n_reads
    check_minimizers(ctx, bases(flavour, 21 + n_reads, n), O.fixed_offsets(n, 150), 150, flavour == "repeats", exact_too=True)


@pytest.mark.parametrize("flavour", ["random", "repeats"])
@pytest.mark.parametrize("read_len", [151, 100])
def test_read_tiled_kernels_with_run_time_geometry(ctx, read_len, flavour):
    """33 reads of 151 bp (16 units per lane) and of 100 bp (14)"""
    n = read_len * 33
    check_minimizers(ctx, bases(flavour, read_len, n), O.fixed_offsets(n, read_len), read_len, flavour == "repeats")


@pytest.mark.parametrize("flavour", ["random", "repeats"])
@pytest.mark.parametrize("shape", ["one_sequence", "ragged_reads"])
def test_position_tiled_kernel(ctx, shape, flavour):
    if shape == "one_sequence":
        offs = np.array([0, 10_000], np.uint64)
    else:
        lens = np.random.default_rng(9).integers(100, 152, 70)
        lens[:4] = (100, 151, 151, 100)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(offs[-1])
    check_minimizers(ctx, bases(flavour, 33, n), offs, 0, flavour == "repeats")


@pytest.mark.parametrize("flavour", ["random", "repeats"])
def test_closed_syncmers(ctx, flavour):
    """(31, 11) with offsets {0, 20}, both orders, on two 10-kbp reads (the oracle's seed: 0)"""
    import biolib_amd as B

    n = 20_000
    seq = bases(flavour, 35, n)
    offs = O.fixed_offsets(n, 10_000)
    b = ctx.upload(seq, read_len=10_000)
    try:
        for (a, e) in ((0, 20), (20, 0)):
            cnt, pos = O.syncmers(seq, offs, 31, 11, a, e, True)
            cap = cnt + 64
            p = ctx.empty_u64(cap)
            r = b.syncmers_raw(31, 11, a, e, 0, B.FLAG_CANONICAL | B.FLAG_SYNC, positions=p, capacity=cap)
            assert int(r.count) == cnt and int(r.xor_pos) == O.xor_reduce(pos)
            assert np.array_equal(p[:cnt].cpu().numpy().view(np.uint64), pos)
            if flavour == "repeats":
                assert int(r.redone) > 0
    finally:
        b.close()
