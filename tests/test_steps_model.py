"""CPU-only: the Python model of the reads' steps (tests/steps_cases.py) restated on strings.  The model looks k-mers up in a dictionary
and reads the node labels; here every one of its records is held against the unitig STRINGS, every LINKED pair against the link records,
every GAF line against the read's bases, and the supports against the number of transitions — so that the emulation and the device are
compared with a model that itself says what the header says."""
import numpy as np
import pytest

import graph_cases as GC
import links_cases as LK
import steps_cases as SC


def all_batches(k):
    for name, table in GC.cases(k):
        m = GC.model(table, k)
        for form, batch in SC.batches_for(name, table, k, m):
            yield name, form, m, batch


def read_of(batch, rec):
    q = int(rec["seq"])
    return batch.reads[q], int(rec["pos"]) - int(batch.offsets[q])


@pytest.mark.parametrize("k", LK.KS)
def test_every_step_spells_its_unitig_and_cannot_be_extended(k):
    seen = dict(steps=0, reverse=0)
    for name, form, m, batch in all_batches(k):
        recs, stats = SC.steps(m, k, batch)
        assert stats["n_steps"] == len(recs) and stats["n_chains"] + stats["n_linked"] == len(recs), "a whole-batch call never sets CONTINUED"
        assert all(int(a["pos"]) < int(b["pos"]) for a, b in zip(recs[:-1], recs[1:])), "strictly ascending pos"
        for s in recs:
            read, at = read_of(batch, s)
            u, o, off, nk = int(s["end"]) >> 1, int(s["end"]) & 1, int(s["offset"]), int(s["n_kmers"])
            text = LK.oriented(m["strings"][u], o)
            assert read[at:at + nk + k - 1] == text[off:off + nk + k - 1], (name, form, "the read's bases are the oriented unitig's")
            assert len(text[off:off + nk + k - 1]) == nk + k - 1
            # not extensible: the k-mer in front of / behind the step does not continue the unitig's string
            if at > 0 and off > 0:
                assert read[at - 1:at - 1 + k] != text[off - 1:off - 1 + k], (name, form, "extends to the left")
            if at + nk + k - 1 < len(read) and off + nk + k - 1 < len(text):
                assert read[at + nk:at + nk + k] != text[off + nk:off + nk + k], (name, form, "extends to the right")
            seen["steps"] += 1
            seen["reverse"] += o
    assert seen["steps"] > 50 and seen["reverse"] > 10


@pytest.mark.parametrize("k", LK.KS)
def test_every_linked_pair_is_a_link_record(k):
    crossed = 0
    for name, form, m, batch in all_batches(k):
        recs, _ = SC.steps(m, k, batch)
        records = set(LK.links(m, k)["records"])
        assert records == LK.string_links(m["strings"], k)
        for a, b in zip(recs[:-1], recs[1:]):
            if not int(b["flags"]) & SC.LINKED:
                continue
            assert int(a["seq"]) == int(b["seq"]) and int(a["pos"]) + int(a["n_kmers"]) == int(b["pos"]), (name, form, "the previous position had a node")
            assert (int(a["end"]), int(b["end"])) in records, (name, form, "a LINKED pair is a record")
            assert int(a["offset"]) + int(a["n_kmers"]) == len(m["unitigs"][int(a["end"]) >> 1][0]), "it leaves at offset L - 1"
            assert int(b["offset"]) == 0, "and enters at offset 0"
            crossed += 1
    assert crossed > 5


@pytest.mark.parametrize("k", LK.KS)
def test_every_gaf_line_spells_the_read_interval(k):
    lines = 0
    for c, (name, form, m, batch) in enumerate(all_batches(k)):
        recs, _ = SC.steps(m, k, batch)
        rule = SC.GAF_RULES[c % len(SC.GAF_RULES)]
        text = SC.gaf_lines(m, k, batch, recs, *rule)
        assert len(text) == len(SC.chains(recs))
        for line, chain in zip(text, SC.chains(recs)):
            f = line[:-1].split(b"\t")
            assert line.endswith(b"\n") and len(f) == 12 and f[4] == b"+" and f[11] == b"255"
            q = int(chain[0]["seq"])
            assert f[0] == rule[0].encode("latin1") + str((rule[1] + q) & SC.M64).encode()
            qlen, qstart, qend, plen, pstart, pend, m1, m2 = (int(f[i]) for i in (1, 2, 3, 6, 7, 8, 9, 10))
            spelled, path = "", f[5].decode("latin1")
            for piece in path.replace("<", " <").replace(">", " >").split():
                number = (int(piece[1 + len(rule[2]):]) - rule[3]) & SC.M64
                assert piece[1:1 + len(rule[2])] == rule[2]
                s = LK.oriented(m["strings"][number], 1 if piece[0] == "<" else 0)
                spelled += s if not spelled else s[k - 1:]
            assert qlen == len(batch.reads[q]) and plen == len(spelled)
            assert m1 == m2 == qend - qstart == pend - pstart
            assert spelled[pstart:pend] == batch.reads[q][qstart:qend], (name, form, "the path spells the read interval")
            lines += 1
    assert lines > 20


@pytest.mark.parametrize("k", LK.KS)
def test_supports_sum_to_the_transitions(k):
    for name, form, m, batch in all_batches(k):
        recs, _ = SC.steps(m, k, batch)
        for once in (False, True):
            lk = LK.links(m, k, once=once)
            sup, stats = SC.support(recs, lk["records"])
            assert stats["n_unmatched"] == 0, "on the unitigs' own table every transition is a record"
            self_reverse = sum(1 for a, b in SC.transitions(recs) if a == b ^ 1)
            want = stats["n_transitions"] if once else 2 * stats["n_transitions"] - self_reverse
            assert int(sup.astype(np.uint64).sum()) == want, (name, form, once)


def test_consecutive_ranges_fold_to_the_whole():
    table, m, batch = SC.cut_batch()
    nodes = SC.position_nodes(m, 31, batch)
    whole, stats = SC.steps(m, 31, batch, 0, 0, nodes)
    continued = 0
    for c in range(1, batch.n_bases):
        a, sa = SC.steps(m, 31, batch, 0, c, nodes)
        b, sb = SC.steps(m, 31, batch, c, 0, nodes)
        assert np.array_equal(SC.fold(list(a) + list(b)), whole), c
        assert sa["n_valid"] + sb["n_valid"] == stats["n_valid"] and sa["n_found"] + sb["n_found"] == stats["n_found"]
        continued += len(b) > 0 and bool(int(b[0]["flags"]) & SC.CONTINUED)
    assert 0 < continued < batch.n_bases - 1


def test_the_seam_batch_has_its_three_kinds_of_run():
    table, m, batch = SC.seam_case()
    k = SC.SEAM_K
    nodes = SC.position_nodes(m, k, batch)
    recs, _ = SC.steps(m, k, batch, 0, 0, nodes)
    spans = [(int(s["pos"]), int(s["pos"]) + int(s["n_kmers"])) for s in recs]
    for seam in SC.SEAMS["across"]:
        assert any(a < seam < b for a, b in spans), ("a step lies across", seam)
    for seam in SC.SEAMS["ending"]:
        assert any(b == seam for a, b in spans) and nodes[seam][1] is None, ("a step ends exactly in front of", seam)
    for seam in SC.SEAMS["hole"]:
        assert nodes[seam - 1][1] is None and nodes[seam][1] is None and not any(a <= seam - 1 < b or a <= seam < b for a, b in spans), ("no node across", seam)
    valid = SC.valid_positions(k, batch)
    assert not valid[176] and valid[3072] and valid[12288], "one hole without k-mers, two with k-mers outside the table"


def test_cases_hold_what_they_are_named_for():
    for k in (5, 31):
        whats = {name: {w for w, _ in SC.reads_for(name, table, k)} for name, table in GC.cases(k)}
        if k == 31:  # (at k = 5 the random strings of these two cases repeat k-mers: other graphs than their names say)
            assert "cycle_2.5_times" in whats["pure_cycle"] and "hairpin" in whats["hairpin"]
        assert {"walk", "substitution", "n_in_the_middle", "k_minus_1", "k", "k_plus_1", "empty", "random", "unitig+", "unitig-"} <= whats["fork"]
        assert all(form in dict(SC.batches_for("fork", dict(GC.cases(k))["fork"], k)) for form in ("ragged", "fixed"))
    # the cycle read goes round: a step per round, LINKED over u+ -> u+
    table = dict(GC.cases(31))["pure_cycle"]
    m = GC.model(table, 31)
    read = dict(SC.reads_for("pure_cycle", table, 31, m))["cycle_2.5_times"]
    recs, _ = SC.steps(m, 31, SC.Reads([read]))
    assert len(recs) == 3 and [int(s["flags"]) for s in recs] == [0, SC.LINKED, SC.LINKED] and len({int(s["end"]) for s in recs}) == 1
    # the hairpin read turns round: u+ then u-
    table = dict(GC.cases(31))["hairpin"]
    m = GC.model(table, 31)
    read = dict(SC.reads_for("hairpin", table, 31, m))["hairpin"]
    recs, _ = SC.steps(m, 31, SC.Reads([read]))
    assert any(int(b["flags"]) & SC.LINKED and int(a["end"]) == int(b["end"]) ^ 1 for a, b in zip(recs[:-1], recs[1:]))
