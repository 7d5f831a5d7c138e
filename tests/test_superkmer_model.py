"""The reference side of tests/test_gpu_superkmer_edges.py, checked without a GPU: the record model against the C oracle's
k-mers, the rounds and the limits against values worked out by hand, and the directed cases' construction against a
retuned copy of the kernel source."""
import re

import numpy as np
import pytest

import oracle_lib as O
import superkmer_model as M


@pytest.mark.parametrize("k,m,canon", [(31, 15, True), (31, 15, False), (32, 5, True), (21, 11, True), (5, 5, True), (16, 1, False)])
def test_expand_of_packed_oracle_groups_is_the_oracle_units(k, m, canon):
    n, L = 6000, 500
    seq = O.synth(31, n)
    seq[np.random.default_rng(k).integers(0, n, 12)] = ord("N")
    offs = O.fixed_offsets(n, L)
    mn, fp, mp, sz, hs = O.super_kmers(seq, offs, k, m, 9, canon)
    assert len(fp) > 100
    recs = M.pack(seq, fp, sz, k, mp)
    vals, ok = O.units(seq, offs, k, canon)
    idx = np.concatenate([np.arange(p, p + s) for p, s in zip(fp.tolist(), sz.tolist())])
    assert np.all(ok[idx] != 0)
    assert np.array_equal(M.expand(recs, k, canon), vals[idx])
    eu, ec = np.unique(vals[idx], return_counts=True)
    gu, gc = M.expected_counts(recs, k, canon)
    assert np.array_equal(gu, eu) and np.array_equal(gc, ec)
    # the record's own fields, its bases and the minimizer the counter finds again through mm_pos
    text = bytes(seq).decode()
    for g in range(0, len(fp), 7):
        s = text[int(fp[g]):int(fp[g]) + int(sz[g]) + k - 1]
        assert M.record_bases(recs[g], k) == s and M.record_size(recs[g]) == sz[g] and M.record_mm_pos(recs[g]) == mp[g]
        assert M.minimizer_of(recs[g], k, m, canon) == int(mn[g])
    assert np.array_equal(M.records_from_bases([text[int(p):int(p) + int(s) + k - 1] for p, s in zip(fp[:300], sz[:300])], k, mp[:300].tolist()), recs[:300])
    M.assert_bucketable(recs, k, m, canon)  # real super-k-mers: a k-mer has one minimizer
    # groups inside the batch: the clipped packing is the plain one, with and without an origin
    origin = 10**12 + 7
    assert np.array_equal(M.pack_clipped(seq, fp, sz, k, mp), recs)
    assert np.array_equal(M.pack_clipped(seq, fp + np.uint64(origin), sz, k, mp, origin), recs)


def test_hand_checked_records():
    # k = 3, "ACGTA": 3 k-mers ACG CGT GTA = 0b000110 0b011011 0b101100; canonical: min with CGT, ACG, TAC
    r = M.records_from_bases(["ACGTA"], 3, 2)
    assert int(r[0, 0]) == 0b0001101100 << 54 and int(r[0, 1]) == (2 << 5) | 2
    assert M.expand(r, 3, False).tolist() == [0b000110, 0b011011, 0b101100]
    assert M.expand(r, 3, True).tolist() == [0b000110, 0b000110, 0b101100]  # CGT -> ACG; GTA < TAC
    assert M.expected_counts(r, 3, True)[0].tolist() == [0b000110, 0b101100] and M.expected_counts(r, 3, True)[1].tolist() == [2, 1]
    # 59 bases: base 32 is the top pair of the second word, base 58 sits in bits 11..10
    s = "A" * 32 + "T" + "A" * 25 + "G"
    r = M.records_from_bases([s], 28, 31)
    assert int(r[0, 0]) == 0 and int(r[0, 1]) == (3 << 62) | (2 << 10) | (31 << 5) | 31
    assert M.record_bases(r[0], 28) == s
    assert M.expand(r, 28, False)[-1] == int("0" * 1 + "3" + "0" * 25 + "2", 4)
    # k = 32: all 64 bits of a value are in use
    assert M.expand(M.records_from_bases(["T" * 32], 32), 32, False).tolist() == [2**64 - 1]
    assert M.expand(M.records_from_bases(["T" * 32], 32), 32, True).tolist() == [0]
    with pytest.raises(AssertionError):
        M.assert_bucketable(M.records_from_bases(["ACGTAC", "CCGTAC"], 5, 0), 5, 1, False)  # CGTAC under minimizers A and C


def test_pack_clipped_by_hand():
    seq = np.frombuffer(b"CGTACGT", np.uint8)
    low = lambda mp, size: (mp << 5) | (size - 1)
    got = M.pack_clipped(seq, [5, 6, 7, 2**64 - 1, 0], [2, 2, 2, 2, 3], 3, [1, 2, 3, 4, 5])
    assert got[0].tolist() == [int("23", 4) << 60, low(1, 2)]      # "GT", then the end of the batch: the record is short
    assert got[1].tolist() == [3 << 62, low(2, 2)]                 # "T"
    assert got[2].tolist() == [0, low(3, 2)]                       # at the end: empty, the low ten bits kept
    assert got[3].tolist() == [0, low(4, 2)]                       # one base in front of origin 0: empty
    assert got[4].tolist() == [int("12301", 4) << 54, low(5, 3)]   # inside: "CGTAC"
    got = M.pack_clipped(seq, [99, 100, 106, 107], [1, 1, 1, 1], 3, [0, 0, 0, 0], origin=100)
    assert got[:, 0].tolist() == [0, int("123", 4) << 58, 3 << 62, 0]


def test_rounds_by_hand():
    assert M.rounds([], 700, 64) == []
    assert M.rounds([32] * 21, 700, 64) == [21] and M.rounds([32] * 22, 700, 64) == [21, 1]     # 672, 704 k-mers
    assert M.rounds([1] * 64, 700, 64) == [64] and M.rounds([1] * 65, 700, 64) == [64, 1]       # the record limit
    assert M.rounds([10] * 64, 700, 64) == [64] and M.rounds([11] * 64, 700, 64) == [63, 1]     # 640 fit; 693 + 11 do not
    assert M.rounds([32] * 21 + [28], 700, 64) == [22] and M.rounds([32] * 21 + [29], 700, 64) == [21, 1]  # exactly 700, 701
    assert M.rounds([32] * 2040, 700, 64) == [21] * 97 + [3]
    assert M.rounds([3, 3, 3, 3], 7, 3) == [2, 2] and M.rounds([3, 3, 1, 3], 7, 3) == [3, 1]


def test_limits_are_all_found_and_as_documented():
    lim = M.limits()
    assert lim == dict(CT_SLOTS=1024, CT_CAP=700, CT_FULL=820, CT_RECS=64, CT_MAXREC=2040, CT_CHUNK=4096, SLOT_MUL=0xD6E8FEB86659FD93, SLOT_BITS=10,
                       BUCKET_RECS=36)
    # what the constants must satisfy among themselves for the table to be sound
    assert lim["CT_MAXREC"] * 32 <= 0xFFFF            # a k-mer comes at most 32 times per record: counts are 16 bits wide
    assert lim["CT_FULL"] < lim["CT_SLOTS"]           # probing always finds an empty slot
    assert lim["CT_CAP"] >= 32 and lim["CT_RECS"] == 64  # a round takes at least one record; one record per lane
    assert M.n_buckets(1) == 1 and M.n_buckets(36) == 1 and M.n_buckets(37) == 2 and M.n_buckets(72) == 2 and M.n_buckets(73) == 3
    # slots worked out by hand: homopolymers of k = 28 are even (low half of a count word), poly-C / poly-T of k = 27 odd
    hp = lambda ch, k: M.kmer_value(ch * k, False)
    assert [M.table_slot(hp(c, 28)) for c in "ACGT"] == [0, 592, 160, 752]
    assert M.table_slot(hp("C", 27)) == 189 and M.table_slot(hp("T", 27)) == 567
    keys = np.array([hp("C", 27), hp("T", 28), 2**64 - 1], np.uint64)
    assert M.table_slots_np(keys).tolist() == [M.table_slot(int(v)) for v in keys]


def test_bucket_fate_by_hand():
    lim = dict(M.limits(), CT_CAP=6, CT_RECS=3, CT_FULL=12, CT_MAXREC=7)
    recs = M.records_from_bases(["ACGTAC", "ACGTAC", "TTGCA", "GGGGGGG"], 3, 0)  # sizes 4, 4, 3, 5
    f = M.bucket_fate(recs, 3, False, lim)
    assert f == dict(path="table", rounds=[1, 1, 1, 1], totals=[4, 4, 3, 5], held=[0, 4, 4, 7], distinct=8)  # the last round: 7 held + 5 = 12
    assert M.bucket_fate(recs, 3, False, dict(lim, CT_FULL=11))["path"] == "fallback"
    assert M.bucket_fate(recs, 3, False, dict(lim, CT_MAXREC=4))["path"] == "table"
    assert M.bucket_fate(recs, 3, False, dict(lim, CT_MAXREC=3))["path"] == "fallback"


def test_directed_cases_move_with_a_retuned_constant(tmp_path):
    """a scratch copy of the kernel source with another CT_CAP / CT_FULL: limits() reads it, and the directed buckets of the
    GPU tests (built by the same functions) sit on the NEW edges"""
    with open(M.SOURCE) as f:
        text = f.read()
    text, n1 = re.subn(r"(constexpr\s+int\s+CT_CAP\s*=\s*)700", r"\g<1>650", text)
    text, n2 = re.subn(r"(constexpr\s+int\s+CT_FULL\s*=\s*)820", r"\g<1>800", text)
    assert n1 == 1 and n2 == 1
    scratch = tmp_path / "retuned.hip"
    scratch.write_text(text)
    lim = M.limits(str(scratch))
    assert lim["CT_CAP"] == 650 and lim["CT_FULL"] == 800 and lim["CT_MAXREC"] == 2040
    for lm in (M.limits(), lim):
        for case in M.round_cases(lm) + M.full_cases(lm):
            M.check_case(case, lm)  # asserts the rounds, the path and the edge the case claims
    names = {c["name"]: c for c in M.round_cases(lim)}
    assert names["cap_floor"]["rounds"] == [650 // 32] and names["cap_floor_plus_1"]["rounds"] == [650 // 32, 1]
    assert names["total_eq_cap"]["totals"] == [650] and names["recs_bind"]["rounds"] == [64] and names["kmers_bind"]["rounds"] == [59, 5]


def test_every_directed_case_sits_where_it_claims():
    lim = M.limits()
    for case in M.all_count_cases(lim):
        M.check_case(case, lim)
