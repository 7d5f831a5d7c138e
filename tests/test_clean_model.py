"""CPU-only: the Python model of graph cleaning (clean_cases.mark_arrays, remove, clean) against its restatement on strings
(clean_cases.string_marks: oriented unitig strings, neighbours through a dict from (k - 1)-prefix, means as fractions) and against the
invariants the header promises.  The model is what the emulation and the device are compared with."""
import fractions

import numpy as np
import pytest

import clean_cases as CC
import graph_cases as GC


def lengths(m, k):
    return [len(s) - k + 1 for s in m["strings"]]


@pytest.mark.parametrize("k", CC.KS)
def test_model_is_the_string_restatement(k):
    for name, table, r in CC.all_cases(k):
        marks, st, m = CC.mark(table, k, r)
        assert marks == CC.string_marks(m["strings"], m["sums"], r), (name, k)
        assert st == CC.stats_of(marks, lengths(m, k), m["sums"]), (name, k)
        assert CC.mark(table, k, r, m)[0] == marks, "a rerun gives the same marks"


@pytest.mark.parametrize("k", CC.KS)
def test_what_is_never_marked(k):
    """an isolated unitig by the tip or bubble rule, the first tip at a junction of tips only, the first branch of a bubble; a flag that is
    off marks nothing of its kind"""
    for name, table, r in CC.all_cases(k):
        marks, _, m = CC.mark(table, k, r)
        offsets, sums, lo, records = CC.arrays_of(m, k)
        L = lengths(m, k)
        deg = [lo[e + 1] - lo[e] for e in range(2 * len(L))]
        out = {e: [t for f, t in records if f == e] for e in range(2 * len(L))}
        for u, mk in enumerate(marks):
            if deg[2 * u] == 0 and deg[2 * u + 1] == 0:
                assert mk in (CC.KEEP, CC.ISLAND), (name, u)
            if mk == CC.TIP:
                assert r["flags"] & CC.TIPS and (deg[2 * u] == 0) != (deg[2 * u + 1] == 0) and L[u] <= r["max_tip_keys"], (name, u)
            if mk == CC.ISLAND:
                assert r["flags"] & CC.ISOLATED and L[u] <= r["max_isolated_keys"], (name, u)
            if mk == CC.BUBBLE:
                assert r["flags"] & CC.BUBBLES and deg[2 * u] == 1 and deg[2 * u + 1] == 1 and L[u] <= r["max_bubble_keys"], (name, u)
        # junctions: the ends that touch one — every x ^ 1 of the records of f ^ 1, for an end f some end leads into
        for f in range(2 * len(L)):
            touching = [x ^ 1 for x in out[f ^ 1]]
            if len(touching) < 2:
                continue
            spurs = [e for e in touching if deg[e ^ 1] == 0 and deg[e] > 0 and L[e >> 1] <= r["max_tip_keys"]]
            if len(spurs) == len(touching) and all(len(out[e]) == 1 for e in touching):
                # every spur's one record leads into this junction, so nothing else decides: the first in the keep order (the greatest
                # mean as a fraction, then the longest, then the smallest number) stays, and with the rule on every other one goes
                best = min(spurs, key=lambda e: (-fractions.Fraction(sums[e >> 1], L[e >> 1]), -L[e >> 1], e >> 1))
                assert marks[best >> 1] == CC.KEEP, (name, "a junction of tips only keeps its first", f, best)
                if r["flags"] & CC.TIPS:
                    assert [e for e in spurs if marks[e >> 1] != CC.TIP] == [best], (name, "and only its first", f)
        # bubbles: the branches between one pair of anchors
        groups = {}
        for u in range(len(L)):
            if deg[2 * u] == 1 and deg[2 * u + 1] == 1:
                a, b = out[2 * u][0], out[2 * u + 1][0]
                groups.setdefault(min((a, b), (b, a)), []).append(u)
        for us in groups.values():
            best = min(us, key=lambda u: (-fractions.Fraction(sums[u], L[u]), -L[u], u))
            assert marks[best] != CC.BUBBLE, (name, "the first branch of a bubble stays", best)


def by_name(k):
    return {name: (table, r) for name, table, r in CC.planted(k)}


@pytest.mark.parametrize("k", CC.CASE_KS)
def test_planted_cases_do_what_they_are_named_for(k):
    cases = by_name(k)

    def marked(name):
        table, r = cases[name]
        marks, st, m = CC.mark(table, k, r)
        return marks, st, m

    marks, st, m = marked("tip_of_max_keys")
    assert st["n_tips"] == 1 and st["n_keys_marked"] == CC.TIP_KEYS and len(marks) == 3
    assert marked("tip_of_one_more")[1]["n_tips"] == 0
    assert marked("tip_beside_a_continuation_with_more_counts_than_it")[1]["n_tips"] == 1, "a real continuation wins whatever the counts"
    for n in (2, 3):
        marks, st, m = marked("%d_spurs_equal_means" % n)
        L = lengths(m, k)
        spurs = [u for u in range(len(L)) if L[u] == 3]
        assert len(spurs) == n and [marks[u] for u in spurs] == [CC.KEEP] + [CC.TIP] * (n - 1), "equal means and lengths: the number decides"
        marks, st, m = marked("%d_spurs_unequal_means" % n)
        L = lengths(m, k)
        spurs = [u for u in range(len(L)) if L[u] == 3]
        best = max(spurs, key=lambda u: int(m["sums"][u]))
        assert [marks[u] for u in spurs] == [CC.KEEP if u == best else CC.TIP for u in spurs]
        marks, st, m = marked("%d_spurs_unequal_lengths" % n)
        L = lengths(m, k)
        assert st["n_tips"] == n - 1 and marks[L.index(3 + n - 1)] == CC.KEEP, "equal means: the longer one stays"
    assert marked("tip_on_a_cycle")[1]["n_tips"] == 1
    for name in ("hairpin_end", "hairpin_end_on_a_path", "pure_cycle"):
        assert not any(marked(name)[0]), name
    assert marked("three_allele_bubble")[1]["n_bubbles"] == 2
    assert marked("snp_bubble_equal_means")[1]["n_bubbles"] == 1
    assert marked("indel_bubble_diff_0")[1]["n_bubbles"] == 0
    marks, st, m = marked("indel_bubble_diff_1")
    assert st["n_bubbles"] == 1 and st["n_keys_marked"] == k, "the insertion's k keys go"
    marks, st, m = marked("indel_bubble_diff_1_short_branch_weaker")
    assert st["n_bubbles"] == 1 and st["n_keys_marked"] == k - 1
    assert marked("bubble_longer_than_max_bubble_keys")[1]["n_bubbles"] == 0
    marks, st, m = marked("bubble_with_one_anchor")
    assert st["n_bubbles"] == 1 and len(marks) == 3
    table, r = cases["eight_bubbles"]
    trace = []
    marks, st, m = CC.mark(table, k, r, trace=trace)
    assert st["n_bubbles"] == 8 and {x & 1 for _, x in trace} == {0, 1}, "branches met in both orientations"
    assert marked("islands_short_long_and_rich")[0].count(CC.ISLAND) == 1
    st = marked("tip_then_bubble_then_island")[1]
    assert (st["n_tips"], st["n_bubbles"], st["n_isolated"]) == (1, 1, 1)


@pytest.mark.parametrize("k", CC.KS)
def test_clean_ends_with_a_round_of_no_marks(k):
    for name, table, r in CC.all_cases(k):
        out, history = CC.clean(table, k, r, max_rounds=64)
        assert history and not any(history[-1][s] for s in ("n_tips", "n_isolated", "n_bubbles")), (name, len(history))
        assert all(any(h[s] for s in ("n_tips", "n_isolated", "n_bubbles")) for h in history[:-1])
        assert set(out) <= set(table) and all(out[x] == table[x] for x in out), "a subset with the counts it had"
        assert len(table) - len(out) == sum(h["n_keys_marked"] for h in history), (name, "every round removes the keys it counted")
        assert not any(CC.mark(out, k, r)[0]), "the result is clean"
        assert CC.clean(table, k, r, max_rounds=1)[1] == history[:1], "max_rounds cuts the loop"


def test_rounds_reach_secondary_effects():
    """a tip on a bubble's branch: the branch is no bubble until the tip is gone"""
    k = 31
    rng = np.random.default_rng(9)
    a, b = GC._rand_seq(rng, 3 * k), GC._rand_seq(rng, 3 * k)
    first = a + "A" + b
    table = CC.counted([(first, 30), (a + "C" + b, 12), (CC._spur(first, 3 * k - 5, k, 2, rng, by=2), 2)], k)
    out, history = CC.clean(table, k)
    assert len(history) >= 3 and history[0]["n_tips"] == 1 and history[0]["n_bubbles"] == 0 and history[1]["n_bubbles"] == 1
    assert len(GC.model(out, k)["strings"]) == 1


@pytest.mark.parametrize("seed", range(4))
def test_products_beyond_64_bits(seed):
    for make, kind in ((CC.synthetic_tips, CC.TIP), (CC.synthetic_bubble, CC.BUBBLE)):
        offsets, sums, link_offsets, links, r = make(seed)
        marks, st = CC.mark_arrays(offsets, sums, link_offsets, links, r)
        loser = 2 if sums[1] * (offsets[3] - offsets[2] - 30) > sums[2] * (offsets[2] - offsets[1] - 30) else 1
        assert [u for u, mk in enumerate(marks) if mk] == [loser] and marks[loser] == kind
        assert CC.wrapped_precedes(sums, offsets, 31, loser, 3 - loser), "a 64-bit product would keep the other one"
        assert st["count_sum_marked"] == sums[loser] and st["n_keys_marked"] == offsets[loser + 1] - offsets[loser] - 30


def test_arrays_that_hold_anything():
    """the model itself takes any arrays: offsets beyond the records, `to` words beyond the ends, more than four records"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        nu, nl = int(rng.integers(1, 9)), int(rng.integers(0, 12))
        offsets = [int(x) for x in rng.integers(0, 200, nu + 1)]
        sums = [int(x) for x in rng.integers(0, 1 << 63, nu)]
        link_offsets = [int(x) for x in rng.integers(0, nl + 4, 2 * nu + 1)]
        links = [(int(rng.integers(0, 1 << 32)), int(rng.integers(0, 2 * nu + 3))) for _ in range(nl)]
        marks, st = CC.mark_arrays(offsets, sums, link_offsets, links, CC.default_rule(5))
        assert len(marks) == nu and st["n_unitigs"] == nu
