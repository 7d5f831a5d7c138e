"""The batches of test_approx_adversaries.py (mined windows and keys on which the approximate hash dword of pass 1 is wrong, nearly wrong
or must trip a wrap guard; tests/approx_plant.py plants them across the lane maps) through the C ABI: records against the oracle AND
against the same scan with set_exact_windows(True), Result.redone at least the tiles the model says must be decided again, and 0 with
exact windows (those kernels carry their exact form inline and list nothing)."""
import numpy as np
import pytest

import approx_plant as P
import oracle_lib as O

pytestmark = pytest.mark.gpu

UNIT, W, SEED = P.UNIT, P.W, P.SEED
WINDOW_CASES, case_entries = P.WINDOW_CASES, P.case_entries


N_POS = 2 * P.POS_STRIDE + 1777


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def scan(ctx, b, n_expected):
    import biolib_amd as B

    got = b.minimizers(UNIT, W, seed=SEED, canonical=True)
    cap = max(n_expected, 1)
    vv, pp, hh = ctx.empty_u64(cap), ctx.empty_u64(cap), ctx.empty_u64(cap)
    r = b.minimizers_raw(UNIT, W, SEED, B.FLAG_CANONICAL | B.FLAG_SYNC, values=vv, positions=pp, hashes=hh, capacity=cap)
    assert int(r.count) == got["count"]
    return got, int(r.redone)


def check(ctx, seq, read_len, form, planted_tiles, control=False):
    offs = O.fixed_offsets(len(seq), read_len) if read_len else np.array([0, len(seq)], np.uint64)
    v, p, h = O.minimizers(seq, offs, UNIT, W, SEED, True, brute=False)
    must, _ = P.redo_bounds(seq, read_len, form)
    assert must >= planted_tiles
    b = ctx.upload(seq, read_len=read_len) if read_len else ctx.upload(seq)
    try:
        got, redone = scan(ctx, b, len(v))
        try:
            ctx.set_exact_windows(True)
            exact, redone_exact = scan(ctx, b, len(v))
        finally:
            ctx.set_exact_windows(False)
    finally:
        b.close()
    _, may = P.redo_bounds(seq, read_len, form)
    print(f"read_len {read_len} {form}: redone {redone} (must {len(must)}, may {len(may)}), exact windows {redone_exact}")
    for name, res in (("approximate", got), ("exact", exact)):
        assert res["count"] == len(v), name
        assert np.array_equal(res["positions"], p) and np.array_equal(res["values"], v) and np.array_equal(res["hashes"], h), name
    assert redone >= len(must)
    if control:  # nothing planted: no more tiles than the model allows (read-tiled: lane 63's halo is lane 0's keys on the device, which the
        # model does not pair up -- one more tile is tolerated there, a chance of about 2^-20 per tile)
        assert redone <= len(may) + (1 if read_len else 0)
    assert redone_exact == 0
    return redone


@pytest.mark.parametrize("case", WINDOW_CASES)
@pytest.mark.parametrize("L", [150, 100, 143, 286])
def test_read_tiled_windows(ctx, L, case):
    g = P.frl_plan(L)
    n_reads = 3 * g["reads_per_tile"] + 5
    seq, control = P.frl_batch(case_entries("top_plus_one", case), L, n_reads, seed=1000 + L)
    check(ctx, seq, L, "top_plus_one", {r // g["reads_per_tile"] for (r, _, _) in P.frl_spots(L, n_reads)})
    check(ctx, control, L, "top_plus_one", set(), control=True)


@pytest.mark.parametrize("cls", P.KEY_CLASSES)
@pytest.mark.parametrize("L", [150, 100, 143, 286])
def test_read_tiled_keys(ctx, L, cls):
    g = P.frl_plan(L)
    n_reads = (P.FRL_KEY_TILES - 1) * g["reads_per_tile"] + 5
    seq, _ = P.frl_batch(P.entries("top_plus_one", (cls,)), L, n_reads, seed=2000 + L, keys=True)
    check(ctx, seq, L, "top_plus_one", {r // g["reads_per_tile"] for (r, _) in P.frl_key_spots(L, n_reads)})


@pytest.mark.parametrize("case", WINDOW_CASES)
def test_position_tiled_windows(ctx, case):
    seq, control = P.pos_batch(case_entries("top", case), N_POS, seed=3001)
    check(ctx, seq, 0, "top", {0, 1, 2})
    check(ctx, control, 0, "top", set(), control=True)


@pytest.mark.parametrize("cls", P.KEY_CLASSES)
def test_position_tiled_keys(ctx, cls):
    seq, _ = P.pos_batch(P.entries("top", (cls,)), N_POS, seed=3002, keys=True)
    check(ctx, seq, 0, "top", {0, 1, 2})


N_CLOSED = 2 * P.CL_STRIDE + 1777


@pytest.mark.parametrize("offsets", [(0, 20), (20, 0)])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("cls", P.CLOSED_CLASSES)
def test_closed_syncmers(ctx, cls, which, offsets):
    """C5: closed syncmers (31, 11) on murmur64_top<true>; positions against the model (and the oracle at the reference's seed 0) and against
    exact windows; all three tiles hold a planted comparison the kernel may not trust"""
    import hash_top_model as T

    e = P.entries("top_plus_one", (cls,), unit=P.CS)[which]
    seq, _ = P.closed_batch(e, N_CLOSED, seed=4001)
    pos = T.closed_syncmers(bytes(seq).decode(), P.CK, P.CS, e["seed"], offsets)
    if e["seed"] == 0:
        n0, pos0 = O.syncmers(seq, np.array([0, len(seq)], np.uint64), P.CK, P.CS, offsets[0], offsets[1], True)
        assert n0 == len(pos) and np.array_equal(pos0, pos)
    b = ctx.upload(seq)
    try:
        got = b.syncmers(P.CK, P.CS, offsets[0], offsets[1], seed=e["seed"], canonical=True)
        r = b.syncmers_raw(P.CK, P.CS, offsets[0], offsets[1], e["seed"], 1 | 4)
        try:
            ctx.set_exact_windows(True)
            exact = b.syncmers(P.CK, P.CS, offsets[0], offsets[1], seed=e["seed"], canonical=True)
        finally:
            ctx.set_exact_windows(False)
    finally:
        b.close()
    print(f"closed {cls}[{which}] {offsets}: redone {int(r.redone)}")
    assert np.array_equal(got["positions"], pos) and np.array_equal(exact["positions"], pos)
    assert int(r.count) == len(pos) and int(r.redone) >= 3
