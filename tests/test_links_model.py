"""CPU-only: the Python model of the unitig links and of the GFA text (links_cases.py) against restatements that share nothing with it:
the links against the oriented unitig strings (a record is a (k - 1)-overlap of two of them), the text against lines joined field by
field.  The model is what the emulation (test_emu_links.py) and the device (test_gpu_links.py) are held against."""
import numpy as np
import pytest

import graph_cases as GC
import links_cases as LK


def check(table, k, m, tag):
    full, once = LK.links(m, k), LK.links(m, k, once=True)
    recs = full["records"]
    st, gs = full["stats"], m["stats"]
    assert st["n_links"] == len(recs) == gs["n_arcs"] - gs["n_linked_sides"] + 2 * gs["n_cycles"], (tag, "the count identity")
    rset = set(recs)
    assert len(rset) == len(recs), (tag, "records are unique")
    assert all((b ^ 1, a ^ 1) in rset for a, b in recs), (tag, "the reverse of every record is a record")
    assert rset == LK.string_links(m["strings"], k), (tag, "the records are the (k - 1)-overlaps of the oriented unitig strings")
    assert recs == sorted(recs, key=lambda r: r[0]) and full["offsets"][-1] == len(recs) and len(full["offsets"]) == 2 * len(m["strings"]) + 1, tag
    for e in range(st["n_ends"]):
        assert all(a == e for a, _ in recs[full["offsets"][e]:full["offsets"][e + 1]]), (tag, "CSR")
    n_self = sum(1 for a, b in recs if a == b ^ 1)
    assert st["n_self_reverse"] == once["stats"]["n_self_reverse"] == n_self
    assert 2 * len(once["records"]) - n_self == len(recs), (tag, "ONCE keeps one of each reverse pair and a self-reverse record once")
    assert set(once["records"]) == {(a, b) for a, b in recs if a <= b ^ 1}
    assert (st["n_dead_ends"], st["n_branch_ends"]) == (once["stats"]["n_dead_ends"], once["stats"]["n_branch_ends"]), "degrees are counted before the filter"
    return full


@pytest.mark.parametrize("k", LK.KS + (7,))
def test_named_cases(k):
    for name, table in GC.cases(k):
        m = GC.model(table, k)
        full = check(table, k, m, (name, k))
        if name == "pure_cycle":
            assert k < 15 or (m["stats"]["n_unitigs"], m["stats"]["n_cycles"]) == (1, 1)  # (a small k folds the random genome)
        if name == "pure_cycle" and k >= 15:
            assert full["records"] == [(0, 0), (1, 1)], "a pure cycle: u+ -> u+ and u- -> u-"
        if name == "empty":
            assert full["records"] == [] and full["offsets"] == [0]
        if name == "hairpin":
            assert any(a == b ^ 1 for a, b in full["records"]), "a hairpin links an end to its own reverse"


@pytest.mark.parametrize("name", [c[0] for c in LK.dense_cases()])
def test_dense_cases(name):
    k, table, m = LK.dense_model(name)
    full = check(table, k, m, name)
    assert full["stats"]["n_branch_ends"] > full["stats"]["n_ends"] // 4, "dense: many branching ends"
    if name == "dense_40000":
        assert len(m["strings"]) > 10000


@pytest.mark.parametrize("n_forks", (0, 1, 15, 31, 63))
def test_forked_paths(n_forks):
    table = LK.forked_path(n_forks)
    m = GC.model(table, 31)
    full = check(table, 31, m, n_forks)
    assert full["stats"]["n_ends"] == 2 + 4 * n_forks and full["stats"]["n_links"] == 4 * n_forks, "every fork: two unitigs more, four records"


def test_a_cycle_beside_forked_paths():
    for n_forks in (1, 31):
        table = LK.forked_path(n_forks, cycle=True)
        m = GC.model(table, 31)
        full = check(table, 31, m, n_forks)
        assert m["stats"]["n_cycles"] == 1 and full["stats"]["n_links"] == 4 * n_forks + 2 and len(LK.links(m, 31, once=True)["records"]) == 2 * n_forks + 1


@pytest.mark.parametrize("k", (3, 5, 7, 9))
def test_random_dense_tables(k):
    """thirty key sets per k, from a handful of keys to a table dense enough that most ends branch"""
    rng = np.random.default_rng(100 + k)
    most = min(len(LK.canonical_kmers(k)), 600)
    for i in range(30):
        table = GC.table_of(LK._random_keys(k, int(rng.integers(1, most + 1)), 1000 * k + i))
        check(table, k, GC.model(table, k), (k, i))


def restated(m, records, k, prefix, first_number, header):
    lines = ["\t".join(("H", "VN:Z:1.0"))] if header else []
    for u, s in enumerate(m["strings"]):
        lines.append("\t".join(("S", prefix + str((first_number + u) % 2**64), s, "LN:i:%d" % len(s), "KC:i:%d" % int(m["sums"][u]))))
    for a, b in records:
        lines.append("\t".join(("L", prefix + str((first_number + (a >> 1)) % 2**64), "+-"[a & 1], prefix + str((first_number + (b >> 1)) % 2**64), "+-"[b & 1],
                                "%dM" % (k - 1))))
    return "".join(line + "\n" for line in lines).encode("latin1")


def test_gfa_text():
    for name, k, table, m in [(n, 5, t, GC.model(t, 5)) for n, t in GC.cases(5)] + [(n,) + LK.dense_model(n) for n in ("dense_300_of_512", "dense_40000")]:
        for once in (False, True):
            recs = LK.links(m, k, once)["records"]
            for prefix, first, header in (LK.RULES if len(m["strings"]) < 1000 else LK.RULES[::3]):
                text = LK.GfaText(LK.gfa_lines(m, recs, k, prefix, first, header))
                want = restated(m, recs, k, prefix, first, header)
                assert text.bytes() == want, (name, once, prefix)
                rng = np.random.default_rng(len(want))
                for x in [0, text.total - 1] + [int(v) for v in rng.integers(0, max(text.total, 1), 200)]:
                    if text.total:
                        assert text.byte(x) == want[x], (name, x)
    # names cross every power of ten up to 10,000, and 2^32 and 2^64
    k, table, m = LK.dense_model("dense_40000")
    lines = LK.gfa_lines(m, [], k, "", 0, False)
    assert [len(lines[u].split(b"\t")[1]) for u in (9, 10, 99, 100, 999, 1000, 9999, 10000)] == [1, 2, 2, 3, 3, 4, 4, 5]
    lines = LK.gfa_lines(m, [], k, "", (1 << 64) - 2, False)
    assert [line.split(b"\t")[1] for line in lines[:3]] == [b"18446744073709551614", b"18446744073709551615", b"0"]
