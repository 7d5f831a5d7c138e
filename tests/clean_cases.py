"""TEST INFRASTRUCTURE: the Python model of graph cleaning (bl_unitigs_mark, bl_table_remove_unitigs, CountTable.clean) and the named cases
of its tests (tests/test_clean_model.py on strings, tests/test_emu_clean.py on the host emulation, tests/test_gpu_clean.py on the device).
Built on graph_cases.model and links_cases.links; the model is the specification (include/biolib_amd.h states it in words).  mark_arrays
reads only the four arrays and the rule, as the library does, with Python integers: no product can wrap.  string_marks states the same
rules on oriented unitig strings with fractions.Fraction means and shares no code with mark_arrays."""
import fractions
import functools
import struct

import numpy as np

import graph_cases as GC
import links_cases as LK
import lookup_cases as LC

TIPS, ISOLATED, BUBBLES = 1, 2, 4
KEEP, TIP, ISLAND, BUBBLE = 0, 1, 2, 3
M64 = (1 << 64) - 1
KS = (3, 5, 7, 15, 31, 33, 63)
STAT_NAMES = ("n_unitigs", "n_tips", "n_isolated", "n_bubbles", "n_keys_marked", "count_sum_marked")
ROWS = (1, 2, 8)  # the compaction's tile is 64 * rows keys; the library's own is the last


def rule(k, tips=None, isolated=None, isolated_mean=None, bubbles=None, bubble_diff=0):
    """the bl_clean_rule of Unitigs.mark's arguments: None switches a rule off (isolated_mean None: no bound on the mean)"""
    flags = (TIPS if tips is not None else 0) | (ISOLATED if isolated is not None else 0) | (BUBBLES if bubbles is not None else 0)
    return dict(flags=flags, k=k, max_tip_keys=tips or 0, max_isolated_keys=isolated or 0, max_isolated_mean=M64 if isolated_mean is None else isolated_mean,
                max_bubble_keys=bubbles or 0, max_bubble_diff=bubble_diff)


def default_rule(k):
    """CountTable.clean's defaults"""
    return rule(k, tips=2 * k, isolated=2 * k, isolated_mean=2**32 - 1, bubbles=2 * k, bubble_diff=0)


def mark_arrays(offsets, sums, link_offsets, links, r, trace=None):
    """the specification on the arrays alone: offsets [nu + 1], sums [nu], link_offsets [2 nu + 1], links [(from, to)] -> (marks, stats).
    The arrays may hold anything: L is taken mod 2^64, link offsets are clamped to the number of records, only the first four records of
    an end are read and a `to` at or above 2 nu is ignored."""
    nu, nl, k, flags = len(sums), len(links), r["k"], r["flags"]

    def L(u):
        return (int(offsets[u + 1]) - int(offsets[u]) - (k - 1)) & M64

    def out(e):
        lo, hi = min(int(link_offsets[e]), nl), min(int(link_offsets[e + 1]), nl)
        d = hi - lo if hi > lo else 0
        return d, [int(links[lo + j][1]) for j in range(min(d, 4))]

    def precedes(w, u):
        return (int(sums[w]) * L(u), L(w), -w) > (int(sums[u]) * L(w), L(u), -u)

    def tip_live_end(w):
        d0, d1 = out(2 * w)[0], out(2 * w + 1)[0]
        if (d0 == 0) == (d1 == 0) or L(w) > r["max_tip_keys"]:
            return None
        return 2 * w if d0 else 2 * w + 1

    def is_tip(u):
        e = tip_live_end(u)
        if e is None:
            return False
        for f in out(e)[1]:
            if f >= 2 * nu:
                continue
            for x in out(f ^ 1)[1]:
                if x >= 2 * nu or x >> 1 == u:
                    continue
                if tip_live_end(x >> 1) != x ^ 1 or precedes(x >> 1, u):
                    return True
        return False

    def is_bubble(u):
        (d0, o0), (d1, o1) = out(2 * u), out(2 * u + 1)
        if d0 != 1 or d1 != 1 or L(u) > r["max_bubble_keys"]:
            return False
        f0, f1 = o0[0], o1[0]
        if f0 >= 2 * nu or f1 >= 2 * nu or f0 >> 1 == u or f1 >> 1 == u:
            return False
        for x in out(f1 ^ 1)[1]:
            if x >= 2 * nu or x >> 1 == u:
                continue
            w = x >> 1
            (dx, ox), (dy, oy) = out(x), out(x ^ 1)
            if dx == 1 and dy == 1 and ox[0] == f0 and oy[0] == f1 and L(w) <= r["max_bubble_keys"] and abs(L(w) - L(u)) <= r["max_bubble_diff"] and precedes(w, u):
                if trace is not None:
                    trace.append((u, x))
                return True
        return False

    marks = []
    for u in range(nu):
        d0, d1 = out(2 * u)[0], out(2 * u + 1)[0]
        m = KEEP
        if d0 == 0 and d1 == 0:
            if flags & ISOLATED and L(u) <= r["max_isolated_keys"] and int(sums[u]) <= r["max_isolated_mean"] * L(u):
                m = ISLAND
        elif d0 == 0 or d1 == 0:
            if flags & TIPS and is_tip(u):
                m = TIP
        elif flags & BUBBLES and is_bubble(u):
            m = BUBBLE
        marks.append(m)
    return marks, stats_of(marks, [L(u) for u in range(nu)], sums)


def stats_of(marks, lengths, sums):
    hit = [u for u, m in enumerate(marks) if m]
    return dict(n_unitigs=len(marks), n_tips=marks.count(TIP), n_isolated=marks.count(ISLAND), n_bubbles=marks.count(BUBBLE),
                n_keys_marked=sum(lengths[u] for u in hit) & M64, count_sum_marked=sum(int(sums[u]) for u in hit) & M64)


def arrays_of(m, k):
    """the four arrays of a graph_cases.model, as the library's calls write them"""
    lk = LK.links(m, k)
    return [int(x) for x in m["offsets"]], [int(x) for x in m["sums"]], lk["offsets"], lk["records"]


def mark(table, k, r, m=None, trace=None):
    m = m or GC.model(table, k)
    return mark_arrays(*arrays_of(m, k), r, trace) + (m,)


def remove(table, m, marks, n_unitigs=None):
    """the table without the keys whose node names a marked unitig below n_unitigs"""
    n_unitigs = len(marks) if n_unitigs is None else n_unitigs
    return {x: table[x] for x, nd in zip(m["keys"], m["nodes"]) if not (int(nd["unitig"]) < n_unitigs and marks[int(nd["unitig"])])}


def clean(table, k, r=None, max_rounds=8):
    """CountTable.clean: -> (table, history); history holds every round's stats, the last round that marked nothing included"""
    r = r or default_rule(k)
    history = []
    for _ in range(max_rounds):
        marks, st, m = mark(table, k, r)
        history.append(st)
        if not any(marks):
            break
        table = remove(table, m, marks)
    return table, history


def string_marks(strings, sums, r):
    """the restatement on strings.  A unitig u read in orientation o is the node (u, o); its successors are the nodes whose string begins
    with its last k - 1 bases (a dict from (k - 1)-prefix, as links_cases.string_links), its predecessors the nodes it succeeds."""
    k, flags = r["k"], r["flags"]
    by_prefix, succ, pred = {}, {}, {}
    for v, s in enumerate(strings):
        for b in (0, 1):
            by_prefix.setdefault(LK.oriented(s, b)[:k - 1], []).append((v, b))
    for u, s in enumerate(strings):
        for o in (0, 1):
            succ[(u, o)] = set(by_prefix.get(LK.oriented(s, o)[len(s) - (k - 1):], ()))
            pred.setdefault((u, o), set())
    for a, bs in succ.items():
        for b in bs:
            pred[b].add(a)
    keys = [len(s) - k + 1 for s in strings]
    mean = [fractions.Fraction(int(sums[u]), keys[u]) for u in range(len(strings))]

    def better(w, u):
        return (mean[w], keys[w], -w) > (mean[u], keys[u], -u)

    def spur(u):
        """the orientation in which a short unitig with exactly one dead end leaves through its live end"""
        live = [o for o in (0, 1) if succ[(u, o)]]
        return live[0] if len(live) == 1 and keys[u] <= r["max_tip_keys"] else None

    marks = []
    for u in range(len(strings)):
        n_out = [len(succ[(u, o)]) for o in (0, 1)]
        m = KEEP
        if n_out == [0, 0]:
            if flags & ISOLATED and keys[u] <= r["max_isolated_keys"] and mean[u] <= r["max_isolated_mean"]:
                m = ISLAND
        elif 0 in n_out:
            o = spur(u)
            if flags & TIPS and o is not None:
                rivals = {wc for junction in succ[(u, o)] for wc in pred[junction] if wc[0] != u}
                if any(spur(w) != c or better(w, u) for w, c in rivals):
                    m = TIP
        elif n_out == [1, 1] and flags & BUBBLES and keys[u] <= r["max_bubble_keys"]:
            ahead, behind = next(iter(succ[(u, 0)])), next(iter(succ[(u, 1)]))
            if ahead[0] != u and behind[0] != u:
                for w in range(len(strings)):
                    if w == u or keys[w] > r["max_bubble_keys"] or abs(keys[w] - keys[u]) > r["max_bubble_diff"] or not better(w, u):
                        continue
                    if any(succ[(w, c)] == {ahead} and succ[(w, 1 - c)] == {behind} for c in (0, 1)):
                        m = BUBBLE
        marks.append(m)
    return marks


# ------------------------------------------------------------------------------------------------------------------------ the named cases

CASE_KS = (15, 31, 33)  # the planted cases: random strings share no (k - 1)-mer by chance at these k
TIP_KEYS = 6            # max_tip_keys of the planted cases' rule


def planted_rule(k, bubble_diff=0):
    return rule(k, tips=TIP_KEYS, isolated=TIP_KEYS, isolated_mean=2**32 - 1, bubbles=k + 2, bubble_diff=bubble_diff)


def counted(parts, k):
    """parts: [(string, count)] -> table; a key takes the count of the first string that holds it"""
    t = {}
    for s, c in parts:
        for p in range(len(s) - k + 1):
            t.setdefault(GC.canon(GC.encode(s[p:p + k]), k), c)
    return t


def _spur(main, at, k, n_keys, rng, by=1):
    """a string that shares k - 1 bases with main at `at`, then leaves: n_keys new k-mers"""
    return main[at:at + k - 1] + GC._other(main[at + k - 1], by) + GC._rand_seq(rng, n_keys - 1)


@functools.lru_cache(maxsize=None)
def planted(k):
    """[(name, table, rule)]"""
    rng = np.random.default_rng(5000 + k)
    R = GC._rand_seq
    out = []

    def add(name, parts, r=None):
        out.append((name, counted(parts, k), r or planted_rule(k)))

    main = R(rng, 4 * k + 30)
    add("tip_of_max_keys", [(main, 50), (_spur(main, k + 5, k, TIP_KEYS, rng), 3)])
    add("tip_of_one_more", [(main, 50), (_spur(main, k + 5, k, TIP_KEYS + 1, rng), 3)])
    add("tip_beside_a_continuation_with_more_counts_than_it", [(main, 2), (_spur(main, k + 5, k, 3, rng), 900)])
    stem = R(rng, 3 * k)
    for n_spurs in (2, 3):
        spurs = [stem[-(k - 1):] + "ACG"[j] + R(rng, 2) for j in range(n_spurs)]
        add("%d_spurs_equal_means" % n_spurs, [(stem, 9)] + [(s, 7) for s in spurs])
        add("%d_spurs_unequal_means" % n_spurs, [(stem, 9)] + [(s, 5 + 3 * j) for j, s in enumerate(spurs)])
        add("%d_spurs_unequal_lengths" % n_spurs, [(stem, 9)] + [(s + "ACGT"[:j], 7) for j, s in enumerate(spurs)])
    ring = R(rng, 4 * k + 9)
    ring = ring + ring[:k - 1]
    add("tip_on_a_cycle", [(ring, 20), (_spur(ring, k, k, 4, rng), 2)])
    w = R(rng, k + 2)
    add("hairpin_end", [(w + GC.revcomp(w), 5)])
    add("hairpin_end_on_a_path", [(main + w + GC.revcomp(w), 5)])
    a, b = R(rng, 2 * k), R(rng, 2 * k)
    add("three_allele_bubble", [(a + "A" + b, 30), (a + "C" + b, 12), (a + "G" + b, 12)])
    add("snp_bubble_equal_means", [(a + "A" + b, 30), (a + "C" + b, 30)])
    ins = a + next(c for c in "ACGT" if c not in (a[-1], b[0])) + b  # (k new k-mers against the k - 1 of a + b)
    add("indel_bubble_diff_0", [(a + b, 30), (ins, 12)], planted_rule(k, 0))
    add("indel_bubble_diff_1", [(a + b, 30), (ins, 12)], planted_rule(k, 1))
    add("indel_bubble_diff_1_short_branch_weaker", [(ins, 30), (a + b, 12)], planted_rule(k, 1))
    add("bubble_longer_than_max_bubble_keys", [(a + "AC" + b, 30), (a + "CA" + b, 12)], rule(k, bubbles=k, bubble_diff=0))
    g = R(rng, 5 * k)
    g2 = g[:2 * k] + GC._other(g[2 * k]) + g[2 * k + 1:]
    add("bubble_with_one_anchor", [(g + g[:k - 1], 30), (g2 + g2[:k - 1], 11)])
    many = []
    for j in range(8):
        a, b = R(rng, 2 * k), R(rng, 2 * k)
        many += [(a + "A" + b, 10 + j), (a + "T" + b, 10 + (j * 5) % 8)]
    add("eight_bubbles", many)
    add("pure_cycle", [(ring, 4)])
    add("islands_short_long_and_rich", [(R(rng, k + 2), 4), (R(rng, k + TIP_KEYS + 3), 4), (R(rng, k + 1), 2**32 - 1)],
        rule(k, tips=TIP_KEYS, isolated=TIP_KEYS, isolated_mean=1000, bubbles=2 * k))
    add("tip_then_bubble_then_island", [(main, 50), (_spur(main, k + 5, k, 3, rng), 3), (a + "A" + b, 30), (a + "C" + b, 12), (R(rng, k), 1)])
    return out


def rule_sets(k):
    """each rule alone and all together"""
    return (rule(k, tips=2 * k), rule(k, isolated=2 * k, isolated_mean=2**32 - 1), rule(k, bubbles=2 * k), rule(k, bubbles=2 * k, bubble_diff=1), default_rule(k))


def all_cases(k):
    """[(name, table, rule)]: every named case of graph_cases at this k under every rule set, and the planted cases where they exist"""
    out = [("%s/r%d" % (name, j), table, r) for name, table in GC.cases(k) for j, r in enumerate(rule_sets(k))]
    if k in CASE_KS:
        out += [(name, table, r) for name, table, r in planted(k)]
        out += [("%s/all" % name, table, default_rule(k)) for name, table, _ in planted(k)]
    return out


def spur_path(n_unitigs, k=31):
    """a path with planted spurs, as links_cases.forked_path but with as many unitigs as asked for: a spur adds two (itself and a cut of
    the path); an even number gets an island as well"""
    assert n_unitigs >= 3
    rng = np.random.default_rng(6000 + n_unitigs)
    n_spurs = (n_unitigs - 1) // 2
    main = GC._rand_seq(rng, 40 * (n_spurs + 1) + k)
    parts = [(main, 40)] + [(_spur(main, 40 * (f + 1), k, 1 + f % 5, rng), 2 + f % 3) for f in range(n_spurs)]
    if n_unitigs % 2 == 0:
        parts.append((GC._rand_seq(rng, k + 1), 1))
    return counted(parts, k)


def synthetic_tips(seed):
    """array sets that come from no table: a long unitig 0 whose + end leads into two spurs, 1 and 2, with sums near 2^64 and lengths near
    2^31, drawn until the products' low 64 bits order the pair the other way round than the products themselves"""
    rng = np.random.default_rng(seed)
    k = 31
    while True:
        l1, l2 = (int(x) for x in (1 << 31) - rng.integers(1, 1000, 2))
        s1, s2 = (M64 - int(x) for x in rng.integers(0, 1 << 40, 2, dtype=np.uint64))
        if l1 != l2 and (s1 * l2 > s2 * l1) != ((s1 * l2) & M64 > (s2 * l1) & M64) and s1 * l2 != s2 * l1:
            break
    lengths = [1 << 33, l1, l2]
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n + k - 1)
    ends = [[2, 4], [], [], [1], [], [1]]
    return _synthetic(offsets, [7, s1, s2], ends, rule(k, tips=1 << 31))


def synthetic_bubble(seed):
    """the same for a bubble: anchors 0 and 3, branches 1 and 2 of equal length near 2^31 would tie; unequal lengths within bubble_diff"""
    rng = np.random.default_rng(seed)
    k = 31
    while True:
        l1, l2 = (int(x) for x in (1 << 31) - rng.integers(1, 1000, 2))
        s1, s2 = (M64 - int(x) for x in rng.integers(0, 1 << 40, 2, dtype=np.uint64))
        if l1 != l2 and (s1 * l2 > s2 * l1) != ((s1 * l2) & M64 > (s2 * l1) & M64) and s1 * l2 != s2 * l1:
            break
    offsets = [0]
    for n in (5, l1, l2, 9):
        offsets.append(offsets[-1] + n + k - 1)
    ends = [[2, 4], [], [6], [1], [6], [1], [], [3, 5]]
    return _synthetic(offsets, [7, s1, s2, 7], ends, rule(k, bubbles=1 << 31, bubble_diff=1000))


def _synthetic(offsets, sums, ends, r):
    link_offsets, links = [0], []
    for e, tos in enumerate(ends):
        links += [(e, t) for t in tos]
        link_offsets.append(len(links))
    return offsets, sums, link_offsets, links, r


def wrapped_precedes(sums, offsets, k, w, u):
    """the keep order as a 64-bit product would get it: what the library must NOT compute"""
    L = lambda v: offsets[v + 1] - offsets[v] - (k - 1)
    return ((sums[w] * L(u)) & M64, L(w), -w) > ((sums[u] * L(w)) & M64, L(u), -u)


# ------------------------------------------------------------------------------------------------------------------------ the emulation's file

def clean_file(arrays, r, table=None, m=None, key_words=1, key_bits=62):
    """the emulation program's input: sixteen words, then offsets, sums, link offsets and link records, then (with a table) the keys, the
    counts and the nodes"""
    offsets, sums, link_offsets, links = arrays
    keys = sorted(table) if table is not None else []
    head = struct.pack("<16Q", key_words, key_bits, len(keys), r["k"], r["flags"], r["max_tip_keys"], r["max_isolated_keys"], r["max_isolated_mean"],
                       r["max_bubble_keys"], r["max_bubble_diff"], len(sums), len(links), 0, 0, 0, 0)
    body = (np.array(offsets, np.uint64).tobytes() + np.array(sums, np.uint64).tobytes() + np.array(link_offsets, np.uint64).tobytes()
            + np.array(links, np.uint32).reshape(-1, 2).tobytes())
    if keys:
        body += LC.words(keys, key_words).tobytes() + np.array([table[x] for x in keys], np.uint32).tobytes() + m["nodes"].tobytes()
    return head + body
