"""The reference side of tests/test_gpu_superkmer128.py, checked without a GPU: the 32-byte record model against the 128-bit k-mer
model (kmers128_model.scan), its minimizer hashes against bl_hash64_u64 through the C oracle, and — at k <= 29, where both records hold
the same groups — against superkmer_model, which is itself pinned to the oracle."""
import numpy as np
import pytest

import kmers128_model as K
import oracle_lib as O
import superkmer128_model as M
import superkmer_model as M64


def _hash64(v, seed):
    return int(O.hash64_np(np.array([v], np.uint64), seed)[0])


def _batch(n, read_len, seed):
    seq = O.synth(seed, n)
    seq[np.random.default_rng(seed).integers(0, n, 6)] = ord("N")
    return seq, O.fixed_offsets(n, read_len)


@pytest.mark.parametrize("k,m,canon", [(33, 32, True), (64, 32, True), (64, 6, False), (48, 17, True), (63, 4, False), (40, 9, True)])
def test_expand_of_packed_groups_is_the_128_bit_scan(k, m, canon):
    seq, offs = _batch(1500, 300, k)
    mn, fp, mp, sz, hs = M.groups(seq, offs, k, m, 9, canon, _hash64)
    assert len(fp) > 20 and max(sz) <= k - m + 1 and max(mp) <= k - m
    recs = M.pack(seq, fp, sz, k, mp)
    scan = K.scan(seq.tobytes(), offs, k, 0, canon)
    idx = np.concatenate([np.arange(p, p + s) for p, s in zip(fp, sz)])
    assert np.all(scan["valid"][idx] == 1) and len(idx) == int(scan["valid"].sum())  # the groups tile the valid k-mers
    want = [int(lo) | (int(hi) << 64) for lo, hi in zip(scan["lo"][idx].tolist(), scan["hi"][idx].tolist())]
    assert M.expand(recs, k, canon) == want
    assert M.from_words(M.to_words(want)) == want
    counts = M.expected_counts(recs, k, canon)
    assert sum(counts.values()) == len(want) and set(counts) == set(want)
    text = bytes(seq).decode()
    for g in range(len(fp)):
        assert M.record_bases(recs[g], k) == text[fp[g]:fp[g] + sz[g] + k - 1] and M.record_size(recs[g]) == sz[g] and M.record_mm_pos(recs[g]) == mp[g]
        assert M.minimizer_of(recs[g], k, m, canon) == mn[g]
    assert hs == O.hash64_np(np.array(mn, np.uint64), 9).tolist()
    M.assert_bucketable(recs, k, m, canon)
    origin = 10**12 + 7
    assert np.array_equal(M.pack_clipped(seq, fp, sz, k, mp), recs)
    assert np.array_equal(M.pack_clipped(seq, (np.array(fp, np.uint64) + np.uint64(origin)).tolist(), sz, k, mp, origin), recs)


@pytest.mark.parametrize("k,m,canon", [(29, 15, True), (21, 11, False), (5, 5, True), (16, 1, False)])
def test_small_k_ties_the_record_to_the_16_byte_one(k, m, canon):
    seq, offs = _batch(3000, 500, 31 + k)
    mn, fp, mp, sz, hs = O.super_kmers(seq, offs, k, m, 9, canon)
    g = M.groups(seq, offs, k, m, 9, canon, _hash64)
    assert [list(map(int, x)) for x in (mn, fp, mp, sz, hs)] == [list(x) for x in g]  # the plain rule is the oracle's
    recs = M.pack(seq, fp, sz, k, mp)
    recs64 = M64.pack(seq, fp, sz, k, mp)
    assert M.expand(recs, k, canon) == M64.expand(recs64, k, canon).tolist()
    u, c = M64.expected_counts(recs64, k, canon)
    assert M.expected_counts(recs, k, canon) == dict(zip(u.tolist(), c.tolist()))
    for a, b in zip(recs[::5], recs64[::5]):
        assert M.minimizer_of(a, k, m, canon) == M64.minimizer_of(b, k, m, canon)


def test_hand_checked_records():
    r = M.records_from_bases(["ACGTA"], 3, 2)
    assert r[0].tolist() == [0b0001101100 << 54, 0, 0, (2 << 6) | 2]
    assert M.expand(r, 3, True) == [0b000110, 0b000110, 0b101100]
    # 122 bases: base 96 is the top pair of word 3, base 121 sits in bits 13..12
    s = "A" * 32 + "C" + "A" * 31 + "G" + "A" * 31 + "T" + "A" * 24 + "G"
    r = M.records_from_bases([s], 59, 63)
    assert r[0].tolist() == [0, 1 << 62, 2 << 62, (3 << 62) | (2 << 12) | (63 << 6) | 63]
    assert M.record_bases(r[0], 59) == s
    assert M.expand(M.records_from_bases(["T" * 64], 64), 64, False) == [2**128 - 1]
    assert M.expand(M.records_from_bases(["T" * 64], 64), 64, True) == [0]
    with pytest.raises(AssertionError):
        M.assert_bucketable(M.records_from_bases(["ACGTAC", "CCGTAC"], 5, 0), 5, 1, False)


def test_pack_clipped_by_hand():
    seq = np.frombuffer(b"CGTACGT", np.uint8)
    low = lambda mp, size: (mp << 6) | (size - 1)
    got = M.pack_clipped(seq, [5, 6, 7, 2**64 - 1, 0], [2, 2, 2, 2, 3], 3, [1, 2, 3, 4, 5])
    assert got[0].tolist() == [int("23", 4) << 60, 0, 0, low(1, 2)]
    assert got[1].tolist() == [3 << 62, 0, 0, low(2, 2)]
    assert got[2].tolist() == [0, 0, 0, low(3, 2)] and got[3].tolist() == [0, 0, 0, low(4, 2)]
    assert got[4].tolist() == [int("12301", 4) << 54, 0, 0, low(5, 3)]
    got = M.pack_clipped(seq, [99, 100, 106, 107], [1, 1, 1, 1], 3, [0, 0, 0, 0], origin=100)
    assert got[:, 0].tolist() == [0, int("123", 4) << 58, 3 << 62, 0]


def test_limits_are_all_found_and_sound():
    lim = M.limits()
    assert lim == dict(CT_SLOTS=1024, CT_CAP=700, CT_FULL=820, CT_RECS=64, CT_MAXREC=1023, SLOT_MUL_HI=0x9E3779B97F4A7C15, SLOT_MUL=0xD6E8FEB86659FD93,
                       SLOT_BITS=10, BUCKET_RECS=24)
    assert lim["CT_MAXREC"] * 64 <= 0xFFFF and lim["CT_FULL"] < lim["CT_SLOTS"] and lim["CT_CAP"] >= 64 and lim["CT_RECS"] == 64
    # with a zero high word the slot is the 64-bit table's
    for v in (0, 1, 2**64 - 1, M64.kmer_value("C" * 27, False)):
        assert M.table_slot(v) == M64.table_slot(v)
    keys = [2**128 - 1, (5 << 64) | 7, 1 << 64]
    arr = M.to_words(keys)
    assert M.table_slots_np(arr[:, 0], arr[:, 1]).tolist() == [M.table_slot(v) for v in keys]


def test_every_directed_case_sits_where_it_claims():
    lim = M.limits()
    cases = M.all_count_cases(lim)
    assert len({c["name"] for c in cases}) == len(cases)
    for case in cases:
        M.check_case(case, lim)
