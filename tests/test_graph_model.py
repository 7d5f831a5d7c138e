"""CPU-only: the Python model of the table graph (graph_cases.py) against a restatement on strings — a dict of k-mer strings, neighbours
by slicing and reverse complement — and the invariants every table must satisfy, on the named cases and on random tables."""
import numpy as np
import pytest

import graph_cases as GC


def string_adjacency(kmers, k):
    """kmers: sorted canonical k-mer strings -> mask bytes and, per side, the neighbours [(slot, side)]"""
    slot = {s: i for i, s in enumerate(kmers)}
    mask, sides = [], []
    for s in kmers:
        m, left, right = 0, [], []
        for c, ch in enumerate("ACGT"):
            f = s[1:] + ch
            y = min(f, GC.revcomp(f))
            if y in slot:
                m |= 1 << c
                right.append((slot[y], GC.LEFT if y == f else GC.RIGHT))
            f = ch + s[:-1]
            y = min(f, GC.revcomp(f))
            if y in slot:
                m |= 16 << c
                left.append((slot[y], GC.RIGHT if y == f else GC.LEFT))
        mask.append(m)
        sides.append((left, right))
    return mask, sides


def string_unitigs(kmers, sides):
    """the unitig strings by walking: a set of strings, each in the orientation whose start rule the model states"""
    def link(i, s):
        if len(sides[i][s]) != 1:
            return None
        j, t = sides[i][s][0]
        return (j, t) if j != i and len(sides[j][t]) == 1 else None

    done, out = set(), {}
    for i in range(len(kmers)):
        if i in done:
            continue
        # all keys of i's component, walking both ways
        comp, cyc = [i], False
        for first in (GC.RIGHT, GC.LEFT):
            cur, side = i, first
            while link(cur, side):
                cur, t = link(cur, side)
                if cur == i:
                    cyc = True
                    break
                comp.append(cur)
                side = 1 - t
            if cyc:
                break
        if cyc:
            start, side = min(comp), GC.RIGHT
        else:
            ends = [j for j in comp if link(j, GC.LEFT) is None or link(j, GC.RIGHT) is None]
            start = min(ends)
            side = GC.RIGHT if link(start, GC.RIGHT) or len(comp) == 1 else GC.LEFT
        s = kmers[start] if side == GC.RIGHT else GC.revcomp(kmers[start])
        cur, n = start, 1
        while n < len(comp):
            cur, t = link(cur, side)
            s += (kmers[cur] if t == GC.LEFT else GC.revcomp(kmers[cur]))[-1]
            side = 1 - t
            n += 1
        done.update(comp)
        out[start] = s
    return [out[i] for i in sorted(out)]


def check_against_strings(table, k):
    m = GC.model(table, k)
    kmers = [GC.decode(x, k) for x in m["keys"]]
    assert kmers == sorted(kmers), "the numeric order of the keys is the alphabetic order of the k-mers"
    mask, sides = string_adjacency(kmers, k)
    assert mask == [int(x) for x in m["mask"]]
    assert string_unitigs(kmers, sides) == m["strings"]
    GC.check_invariants(table, k, m)
    return m


@pytest.mark.parametrize("k", GC.KS)
def test_named_cases(k):
    names = set()
    for name, table in GC.cases(k):
        m = check_against_strings(table, k)
        names.add(name)
        st = m["stats"]
        if name == "pure_cycle" and k >= 15:
            assert st["n_cycles"] == 1 and st["n_unitigs"] == 1 and st["n_linked_sides"] == 2 * st["n_keys"]
        if name == "two_key_cycle":
            assert st["n_cycles"] == 1 and st["n_keys"] == 2 and m["strings"][0] == ("AC" * k)[:k + 1]
        if name == "single_key":
            assert st["n_unitigs"] == 1 and m["nodes"][0]["rank_flip"] == 0
        if name == "snp_bubble" and k >= 15:
            assert st["n_unitigs"] == 4 and st["n_branch_sides"] == 2
        if name == "homopolymer_self_arc":
            assert m["mask"][0] & 1 and m["keys"][0] == 0, "AAA..A's right side holds A: itself"
        if name == "double_arc":
            assert int(m["mask"][0]) & 0x0F == 0b1001 and st["n_branch_sides"] == 2
        if name == "hairpin" and k >= 15:
            assert st["n_unitigs"] == 1 and st["n_dead_end_sides"] == 1 and st["n_branch_sides"] == 0, "a hairpin's turn is a dead-end side... of nobody: it loops"
        if name == "alternating_flips" and k >= 15:
            flips = [f for _, f in m["unitigs"][0][0]]
            assert len(flips) >= 4 and all(x != y for x, y in zip(flips[:-1], flips[1:])), flips
        if name == "start_at_the_smaller_end" and k >= 5:
            path = m["unitigs"][0][0]
            assert path[0][0] < path[-1][0]
    assert {"single_key", "straight_path", "fork", "merge", "snp_bubble", "tip", "hairpin", "homopolymer_self_arc", "pure_cycle"} <= names


def test_path_lengths_are_one_unitig():
    for n in GC.PATH_LENGTHS:
        m = GC.model(GC.path_case(n), 31)
        assert m["stats"]["n_unitigs"] == 1 and m["stats"]["longest_unitig"] == n and len(m["strings"][0]) == n + 30


@pytest.mark.parametrize("k", (1, 3, 5, 7, 9, 15))
def test_invariants_on_random_tables(k):
    rng = np.random.default_rng(5 * k)
    for trial in range(24):
        kind = trial % 4
        if kind == 0:
            keys = {GC.canon(int(rng.integers(0, 4 ** k)), k) for _ in range(int(rng.integers(1, 200)))}
        elif kind == 1:
            keys = GC.keys_of([GC._rand_seq(rng, int(rng.integers(k, 300)))], k)
        elif kind == 2:
            g = GC._rand_seq(rng, int(rng.integers(k + 1, 200)))
            keys = GC.keys_of([g + g[:k - 1]], k)
        else:
            keys = GC.keys_of([GC._rand_seq(rng, int(rng.integers(k, 300)), "AT"), GC._rand_seq(rng, 60, "AC")], k)
        check_against_strings(GC.table_of(keys), k)
