"""GPU test of the two count scans that share the 128-bit tile launcher (scan_counts_kernel of bl_lookup.hip, read_counts_kernel of
bl_read_counts.hip) at the smallest size where a workgroup takes a second tile: more than TILE_GRID_MAX tiles.  There the barrier in
front of a tile's staging guards the previous tile's codes and flags, the wave's bisection of the offsets runs per tile over 10^5 and
10^6 sequences, and the identity fill strides over more records than it has threads.  test_gpu_scan128_many_tiles.py covers the hash
sampler, syncmers and minimizers in the same way; these two kernels are not in it.

Shapes (scale_cases.py): the 9,199-base blocks of the per-read count tests laid end to end 914 times: 8,407,886 bases = 2,053 tiles.
9,199 mod 16 = 15: every repetition meets the lanes and the tiles at another alignment.  No record crosses a block, so the expected
result is the Python model's result on ONE block, tiled; nothing expected comes from the library."""
import numpy as np
import pytest

import read_counts_cases as RC
import scale_cases as S
from test_gpu_read_counts import build, canaries, dev_offsets, host_records

pytestmark = pytest.mark.gpu
MIN_COUNT = 2


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def assert_records(got, want, tag):
    assert RC.same(got, want), (tag, "first differing records", S.first_differences(got, want))


def check_records_init_on_canaries(b, t, sc, k):
    """INIT over the whole batch on a buffer of canary bytes: byte-identical to the tiled model, no canary inside the touched span"""
    from biolib_amd.scan import _flags

    buf = canaries(sc["n_seqs"])
    b.read_counts_raw(t, k, _flags(True, False, True), MIN_COUNT, buf, 0, 0, dev_offsets(sc["offs"]))
    got = host_records(buf)
    want, (lo, hi) = S.expected_tiled_records(sc, MIN_COUNT, S.canary_record())
    assert_records(got, want, (sc["block"]["name"], k, "INIT on canaries"))
    inside = got[lo:hi + 1].view(np.uint8).reshape(-1, 48)
    assert not (inside == RC.CANARY_BYTE).all(axis=1).any(), "a canary record inside the touched span"
    return lo, hi


@pytest.mark.parametrize("k,key_words", [(31, 1), (33, 2)])
def test_ragged_many_tiles(ctx, k, key_words):
    import torch

    sc = S.scan_case("ragged", k)
    c = sc["block"]
    assert S.n_tiles(sc["total"]) >= S.CAPS["TILE_GRID_MAX"] + 4
    b = ctx.upload(sc["seq"], sc["offs"])
    t = build(ctx, c["table"], key_words, 2 * k)
    assert b.n_seqs == sc["n_seqs"]
    # bl_scan_kmer_counts: every position
    want_counts, want_valid, words = S.expected_positions(sc)
    counts, valid, r = b.kmer_counts(t, k, canonical=True, valid=True)
    got_counts, got_valid = host_u32(counts), valid.cpu().numpy()
    bad = np.nonzero((got_counts != want_counts) | (got_valid != want_valid))[0]
    assert len(bad) == 0, ("first wrong positions", bad[:8].tolist(), "tiles", (bad[:8] // S.H).tolist())
    print({word: r[word] for word in words})
    assert {word: r[word] for word in words} == words and r["status"] == 0
    del counts, valid
    # bl_scan_read_counts: the records, from the binding (identities outside the touched span) and raw on canaries
    whole, r2 = b.read_counts(t, k, min_count=MIN_COUNT, canonical=True, offsets=sc["offs"])
    assert {word: r2[word] for word in words} == words
    want, (lo, hi) = S.expected_tiled_records(sc, MIN_COUNT, RC.IDENTITY)
    assert_records(whole.host(), want, ("ragged", k, "read_counts"))
    assert check_records_init_on_canaries(b, t, sc, k) == (1, sc["n_seqs"] - 2)
    # ACCUMULATE over two ranges cut inside the three-tile read of a middle repetition
    cut = S.three_tile_read_cut(sc)
    acc, first_part = b.read_counts(t, k, min_count=MIN_COUNT, canonical=True, first=cut, n=sc["total"] - cut, offsets=sc["offs"])
    acc, second_part = b.read_counts(t, k, min_count=MIN_COUNT, canonical=True, first=0, n=cut, offsets=sc["offs"], into=acc)
    assert torch.equal(acc.records, whole.records), S.first_differences(acc.host(), whole.host())
    for word in ("count", "found", "sum_counts"):
        assert (first_part[word] + second_part[word]) & S.M64 == words[word], word
    t.close()
    b.close()


def test_fixed7_many_sequences(ctx):
    """1,315 reads of 7 bases (the last one 1 base) x 914: more touched records than the identity fill has threads, and a bisection over
    1.2 M offsets per wave and tile"""
    k = 5
    sc = S.scan_case("fixed7", k)
    c = sc["block"]
    assert sc["n_seqs"] > S.CAPS["INIT_GRID_MAX"] * S.CAPS["ITPB"]
    b = ctx.upload(sc["seq"], sc["offs"])
    t = build(ctx, c["table"], 1, 2 * k)
    assert b.n_seqs == sc["n_seqs"]
    want_counts, want_valid, words = S.expected_positions(sc)
    whole, r = b.read_counts(t, k, min_count=MIN_COUNT, canonical=True, offsets=sc["offs"])
    print({word: r[word] for word in words})
    assert {word: r[word] for word in words} == words and r["status"] == 0
    want, (lo, hi) = S.expected_tiled_records(sc, MIN_COUNT, RC.IDENTITY)
    assert_records(whole.host(), want, ("fixed7", k, "read_counts"))
    assert int(want["n_kmers"].sum()) == words["count"] and int(want["sum_counts"].sum()) & S.M64 == words["sum_counts"]
    assert check_records_init_on_canaries(b, t, sc, k) == (0, sc["n_seqs"] - 1)
    t.close()
    b.close()
