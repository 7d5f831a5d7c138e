"""GPU test of bl_scan_read_edits at the smallest size where a workgroup of its state pass takes a second tile: state_kernel goes through
the 128-bit tile launcher, which caps the grid at TILE_GRID_MAX workgroups, and from there on the barrier in front of a tile's staging
guards the previous tile's codes and flags.  test_gpu_count_scans_many_tiles.py does the same for the two count scans on that launcher.

Shape: the named reads of correct_cases.py (some 11,000 bases at k = 31 and 12,000 at k = 33, no multiple of 16, so every repetition meets
the lanes and the tiles at another alignment) laid end to end until the batch holds TILE_GRID_MAX + 4 tiles or more.  No run crosses a read, so the
expected answer is the Python model's answer on ONE block, tiled: the edits record for record, the stats word for word.  Nothing
expected comes from the library.  The same batch is cut into two ranges inside a run that lies behind the cap, and corrected."""
import numpy as np
import pytest

import correct_cases as CC
import scale_cases as S
from test_gpu_correct import same_edits, scan, table_on

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def tiled_case(k, canonical):
    c = CC.cases(k, canonical)
    L = CC.layout(c, "offsets")
    n = len(L["bases"])
    reps = S.smallest_even(lambda r: S.n_tiles(r * n) >= S.CAPS["TILE_GRID_MAX"] + 4 or r * n > S.MAX_POSITIONS)
    assert reps is not None and reps * n <= S.MAX_POSITIONS and n % 16 != 0
    edits, stats, detail = CC.model(L["bases"], L["offs"], k, c["table"], c["min_count"], 1, canonical)
    want = np.tile(edits, reps)
    want["pos"] += np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(n), len(edits))
    return dict(c=c, n=n, reps=reps, total=reps * n, bases=np.tile(L["bases"], reps), offs=S.tiled_offsets(L["offs"], n, reps), block_bases=L["bases"],
                block_edits=edits, block_detail=detail, edits=want, stats={name: v * reps for name, v in stats.items()})


@pytest.mark.parametrize("k,canonical", [(31, True), (33, False)])
def test_more_tiles_than_the_state_pass_has_workgroups(ctx, k, canonical):
    t = tiled_case(k, canonical)
    assert S.n_tiles(t["total"]) >= S.CAPS["TILE_GRID_MAX"] + 4 and len(t["block_edits"]) > 100 and t["stats"]["n_misfit"] > 0
    table = table_on(ctx, t["c"]["table"], k)
    b = ctx.upload(t["bases"], t["offs"])
    assert b.n_seqs == len(t["offs"]) - 1
    _, got, stats = scan(b, table, k, canonical, CC.MIN_COUNT, need=len(t["edits"]))
    assert stats == t["stats"], (stats, t["stats"])
    same_edits(got, t["edits"], "whole")
    # two ranges cut inside an edited run of a repetition that lies behind the cap: the second range starts in a tile a workgroup takes second
    rep = (S.CAPS["TILE_GRID_MAX"] * S.H) // t["n"] + 1
    a, bb = next((a, bb) for _, a, bb, cls in t["block_detail"] if cls == "edit" and bb - a >= 4)
    cut = rep * t["n"] + a + 2
    assert S.n_tiles(cut) > S.CAPS["TILE_GRID_MAX"] and cut < t["total"]
    _, e1, s1 = scan(b, table, k, canonical, CC.MIN_COUNT, first=0, n=cut, need=len(t["edits"]))
    _, e2, s2 = scan(b, table, k, canonical, CC.MIN_COUNT, first=cut, n=0, need=len(t["edits"]))
    same_edits(np.concatenate([e1, e2]), t["edits"], "two ranges")
    assert {name: s1[name] + s2[name] for name in stats} == t["stats"]
    w1, ws1, _ = CC.model(t["block_bases"], t["offs"][:len(t["c"]["reads"]) + 1], k, t["c"]["table"], CC.MIN_COUNT, 1, canonical, 0, a + 2)
    assert len(e1) == rep * len(t["block_edits"]) + len(w1) and s1 == {name: rep * t["stats"][name] // t["reps"] + ws1[name] for name in stats}
    # the corrected batch, byte for byte
    edits, _ = b.read_edits(table, k, CC.MIN_COUNT, canonical=canonical, capacity=len(t["edits"]))
    fixed = b.apply_edits(edits)
    assert np.array_equal(fixed.download(), np.tile(CC.apply_model(t["block_bases"], t["block_edits"]), t["reps"]))
    for x in (fixed, b, table):
        x.close()


def test_apply_edits_on_a_fixed_length_batch_that_never_built_its_start_bits(ctx):
    """the copy of such a batch carries no start bits either and builds them when a position-tiled scan first needs them"""
    from test_gpu_correct import one_error_reads

    k, m = 21, 300
    bases, offs, table, at, truth = one_error_reads(k, m, True)
    R = int(offs[1])
    want, stats, _ = CC.model(bases, offs, k, table, 3, 1, True)
    t = table_on(ctx, table, k)
    made = ctx.upload(bases, read_len=R)
    edits, _ = made.read_edits(t, k, 3, canonical=True)
    fresh = ctx.upload(bases, read_len=R)  # (no scan has touched it)
    fixed = fresh.apply_edits(edits)
    assert np.array_equal(fixed.download(), truth) and (fixed.n_seqs, fixed.read_len) == (m, R)
    _, again, s = scan(fixed, t, k, True, 3)
    assert len(again) == 0 and s["n_runs"] == 0, "every k-mer of the corrected batch is solid, read by read"
    _, got, s = scan(fresh, t, k, True, 3)
    same_edits(got, want, "the source, scanned after it was copied")
    assert s == stats
    for x in (fixed, fresh, made, t):
        x.close()
