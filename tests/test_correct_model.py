"""CPU-only: the Python model of the repair rule (correct_cases.py) against a second, brute-force statement of it — apply each single-base
change to the read and recount all of its k-mers — and the rule's invariants on simulated reads: nothing outside a corrected run changes,
every corrected run becomes solid, no edit differs from the planted truth."""
import numpy as np
import pytest

import correct_cases as CC


def brute_force(bases, offs, k, table, min_count, min_support, canonical):
    """edits as (pos, to) and the classes, from recounting whole reads"""
    bases = CC.as_bytes(bases)
    edits, classes = [], []
    for q in range(len(offs) - 1):
        lo, hi = int(offs[q]), int(offs[q + 1])
        read = bases[lo:hi]
        L = len(read)
        n = L - k + 1
        if n < 1:
            continue

        def states(r):
            return CC.states_of(CC.read_kmers(CC._CODE[r], k, canonical), table, min_count)

        st = states(read)
        for a, b in CC.weak_runs(st):
            # the bases whose substitution touches exactly the k-mers a .. b
            touching = [p for p in range(L) if (max(0, p - k + 1), min(p, n - 1)) == (a, b)]
            if a >= 1 and st[a - 1] == CC.SOLID:
                ps = [p for p in touching if p == a + k - 1]
            elif b <= n - 2 and st[b + 1] == CC.SOLID:
                ps = [p for p in touching if p == b]
            else:
                ps = []
            if not ps:
                classes.append("misfit")
                continue
            (p,) = ps
            if b - a + 1 < min_support:
                classes.append("low_support")
                continue
            good = []
            for letter in b"ACGT":
                if CC._CODE[letter] == CC._CODE[read[p]]:
                    continue
                changed = read.copy()
                changed[p] = letter
                st2 = states(changed)
                if all(s == CC.SOLID for s in st2[a:b + 1]):
                    good.append(letter)
                    assert st2[:a] == st[:a] and st2[b + 1:] == st[b + 1:], "a change at p touches the k-mers a .. b only"
            classes.append("edit" if len(good) == 1 else ("ambiguous" if good else "no_base"))
            if len(good) == 1:
                edits.append((lo + p, good[0] | (int(read[p]) & 0x20)))
    return edits, classes


@pytest.mark.parametrize("canonical", (False, True), ids=("forward", "canonical"))
@pytest.mark.parametrize("k", (1, 2, 5, 31, 33))
def test_model_against_brute_force(k, canonical):
    c = CC.cases(k, canonical)
    keep = [i for i, name in enumerate(c["names"]) if not name.startswith("every_base") or int(name.rsplit("_p", 1)[1]) % 5 in (0, 3)]
    reads = [c["reads"][i] for i in keep]
    for kind in CC.LAYOUTS:
        L = CC.layout(dict(c, reads=reads), kind)
        for min_support in sorted({1, min(2, k)}):
            edits, stats, detail = CC.model(L["bases"], L["offs"], k, c["table"], c["min_count"], min_support, canonical)
            want_edits, want_classes = brute_force(L["bases"], L["offs"], k, c["table"], c["min_count"], min_support, canonical)
            assert [d[3] for d in detail] == want_classes, kind
            assert [(int(e["pos"]), int(e["to"])) for e in edits] == want_edits, kind
            assert stats["n_runs"] == len(want_classes) == sum(stats[name] for name in CC.STAT_NAMES[1:])


def test_range_rule_of_the_model():
    c = CC.cases(5, False)
    L = CC.layout(c, "offsets")
    whole, stats, _ = CC.model(L["bases"], L["offs"], 5, c["table"], c["min_count"])
    n = len(L["bases"])
    for cut in range(0, n + 1, 3):
        e1, s1, _ = CC.model(L["bases"], L["offs"], 5, c["table"], c["min_count"], first=0, n=cut) if cut else (whole[:0], dict.fromkeys(CC.STAT_NAMES, 0), None)
        e2, s2, _ = CC.model(L["bases"], L["offs"], 5, c["table"], c["min_count"], first=cut, n=0) if cut < n else (whole[:0], dict.fromkeys(CC.STAT_NAMES, 0), None)
        assert np.array_equal(np.concatenate([e1, e2]), whole) and {k: s1[k] + s2[k] for k in stats} == stats, cut


# The experiment of the feature's proposal: a 20-kbp random genome, 100-bp reads at 30x from both strands, 1 % substitutions, a canonical
# table counted from the erroneous reads themselves, min_count = 3.  68 - 74 % of the planted errors were repaired there; the floor below
# (half) only keeps the test from going vacuous.  "No edit differs from the truth" is a property of the data, not of the rule: a chance solid
# k-mer inside an error's run can split it into two that fit other bases (seed 20260 has one such read at k = 15: an error at base 13, its
# k-mer 2 solid by coincidence, the run [0, 1] repaired at base 1).  Seeds 1, 2, 3, 7 and 11 have none at either k; 1 is committed.
SIM = dict(seed=1, genome_len=20000, read_len=100, coverage=30, rate=0.01)


@pytest.mark.parametrize("k", (15, 21))
def test_invariants_on_simulated_reads(k):
    bases, truth, offs, planted = CC.simulate(**SIM)
    table = CC.counted_table(bases, offs, k, True)
    edits, stats, detail = CC.model(bases, offs, k, table, 3, 1, True)
    fixed = CC.apply_model(bases, edits)
    st0, cnt0 = CC.position_states(bases, offs, k, table, 3, True)
    st1, cnt1 = CC.position_states(fixed, offs, k, table, 3, True)
    corrected = np.zeros(len(bases), bool)
    for _, a, b, cls in detail:
        if cls == "edit":
            corrected[a:b + 1] = True
    assert (st1[corrected] == CC.SOLID).all(), "every corrected run becomes solid"
    assert np.array_equal(st1[~corrected], st0[~corrected]) and np.array_equal(cnt1[~corrected], cnt0[~corrected]), "no state outside the corrected runs changes"
    assert int(corrected.sum()) == int(edits["support"].sum())
    want = dict(planted)
    wrong = [int(e["pos"]) for e in edits if want.get(int(e["pos"])) != int(e["to"])]
    assert not wrong, ("edits that differ from the planted truth", wrong[:5])
    print(f"k = {k}: {len(edits)} of {len(planted)} planted errors repaired, {stats}")
    assert 2 * len(edits) >= len(planted)
