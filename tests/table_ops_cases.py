"""Shared cases and the model of the count-table algebra (bl_table_combine / bl_table_filter; CountTable.union, intersect, subtract,
subtract_counts, filter, compare).  The model is plain Python dicts {key: count}.  The tile geometry (threads, elements per thread, tile
size per key width) is read out of biolib_amd/csrc/bl_table_ops_core.hpp, so that the planted cases move with a retuned constant; each
planted case is checked on the model's merged order to sit where it claims (check_case).

A case is a dict: name, key_words, key_bits, a, b ({key: count}; b None: the NULL table), same (pass the A object twice), planted (list
of diagonals d: merged[d - 1] is an A element and merged[d] its equal B partner), kind ("size", "relation", "planted", "words", "counts"),
rules (list of (op, mode, count_lo, count_hi))."""
import os
import random
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "biolib_amd", "csrc", "bl_table_ops_core.hpp")

UNION, INTERSECT, SUBTRACT, COUNT_SUBTRACT = 0, 1, 2, 3
SUM, MIN, MAX, LEFT, RIGHT = 0, 1, 2, 3, 4
U32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
# every op with every mode it takes
OP_MODES = [(UNION, m) for m in (SUM, MIN, MAX, LEFT, RIGHT)] + [(INTERSECT, m) for m in (SUM, MIN, MAX, LEFT, RIGHT)] + [(SUBTRACT, LEFT), (COUNT_SUBTRACT, LEFT)]
KEY_BITS = {1: (2, 62, 64), 2: (102, 128)}


def geometry(source=SOURCE):
    """{"TPB", "ITEMS": {1: , 2: }, "TILE": {1: , 2: }} from the core header; every constant must be found"""
    with open(source) as f:
        text = f.read()

    def one(pat):
        found = re.findall(pat, text)
        assert len(found) == 1, f"{pat}: {len(found)} matches in {source}"
        return found[0]

    tpb = int(one(r"constexpr\s+int\s+TPB\s*=\s*(\d+)\s*;"))
    items = {1: int(one(r"constexpr\s+int\s+ITEMS_U64\s*=\s*(\d+)\s*;")), 2: int(one(r"constexpr\s+int\s+ITEMS_U128\s*=\s*(\d+)\s*;"))}
    one(r"constexpr\s+int\s+TILE_U64\s*=\s*TPB\s*\*\s*ITEMS_U64\s*;")
    one(r"constexpr\s+int\s+TILE_U128\s*=\s*TPB\s*\*\s*ITEMS_U128\s*;")
    return dict(TPB=tpb, ITEMS=items, TILE={w: tpb * items[w] for w in (1, 2)})


# ----------------------------------------------------------------------------- the model

def combine_counts(mode, a, b):
    return {SUM: min(a + b, U32), MIN: min(a, b), MAX: max(a, b), LEFT: a, RIGHT: b}[mode]


def model(a, b, op, mode, lo=0, hi=U32):
    """(result dict, stats dict) of bl_table_combine on the dicts a and b (b may be None)"""
    b = b or {}
    out = {}
    for x in sorted(set(a) | set(b)):
        ina, inb = x in a, x in b
        if op == UNION:
            c = combine_counts(mode, a[x], b[x]) if ina and inb else (a[x] if ina else b[x])
        elif op == INTERSECT:
            if not (ina and inb):
                continue
            c = combine_counts(mode, a[x], b[x])
        elif op == SUBTRACT:
            if not ina or inb:
                continue
            c = a[x]
        else:
            if not ina or a[x] <= b.get(x, 0):
                continue
            c = a[x] - b.get(x, 0)
        if lo <= c <= hi:
            out[x] = c
    both = set(a) & set(b)
    stats = dict(n_a_only=len(set(a) - both), n_b_only=len(set(b) - both), n_both=len(both), n_out=len(out),
                 sum_min=sum(min(a[x], b[x]) for x in both) & M64, sum_max=sum(max(a.get(x, 0), b.get(x, 0)) for x in set(a) | set(b)) & M64,
                 sum_out=sum(out.values()) & M64)
    return out, stats


def jaccards(stats):
    union = stats["n_a_only"] + stats["n_b_only"] + stats["n_both"]
    return (stats["n_both"] / union if union else 0.0), (stats["sum_min"] / stats["sum_max"] if stats["sum_max"] else 0.0)


def merged(a, b):
    """the merged order of the two key sets, ties A first: a list of ("A" | "B", key)"""
    return sorted([(x, 0) for x in a] + [(x, 1) for x in (b or {})], key=lambda e: e)  # (key, 0) sorts in front of (key, 1)


def check_case(case):
    """the planted pairs sit where the case says, the keys fit key_bits, the sizes are the promised ones"""
    a, b = case["a"], (case["a"] if case["same"] else case["b"])
    for t in (a, b or {}):
        assert all(0 <= x < (1 << case["key_bits"]) for x in t) and all(0 <= c <= U32 for c in t.values()), case["name"]
    m = merged(a, b)
    for d in case["planted"]:
        assert 0 < d < len(m) and m[d - 1][1] == 0 and m[d][1] == 1 and m[d - 1][0] == m[d][0], (case["name"], d)
    if "sizes" in case:
        assert (len(a), len(b or {})) == case["sizes"], case["name"]
    for op, mode, lo, hi in case["rules"]:
        assert lo <= hi


# ----------------------------------------------------------------------------- building tables from a layout

def _distinct_keys(rng, n, key_bits, ends):
    """n sorted distinct keys below 2^key_bits; ends: 0 and 2^key_bits - 1 are among them (where n allows)"""
    top = 1 << key_bits
    assert n <= top
    keys = set()
    if ends and n >= 1:
        keys.add(0)
    if ends and n >= 2:
        keys.add(top - 1)
    if top <= 4 * n + 16:
        rest = [x for x in range(top) if x not in keys]
        rng.shuffle(rest)
        keys.update(rest[: n - len(keys)])
    while len(keys) < n:
        keys.add(rng.randrange(top))
    return sorted(keys)


def from_layout(rng, layout, key_bits, ends=True, max_count=5):
    """layout: a string over "A" (key of A only), "B" (of B only), "P" (an equal pair) in key order -> the two dicts"""
    keys = _distinct_keys(rng, len(layout), key_bits, ends)
    a, b = {}, {}
    for x, what in zip(keys, layout):
        if what in "AP":
            a[x] = rng.randint(1, max_count)
        if what in "BP":
            b[x] = rng.randint(1, max_count)
    return a, b


def _shuffled(rng, n_a, n_b, pairs):
    tokens = list("P" * pairs + "A" * (n_a - pairs) + "B" * (n_b - pairs))
    rng.shuffle(tokens)
    return "".join(tokens)


def planted_layout(rng, total, diagonals, runs=()):
    """a layout of `total` merged elements with an equal pair across every diagonal d of `diagonals` (the A element at d - 1, its partner
    at d) and, for (start, n) in runs, n consecutive pairs from merged position start; singles elsewhere"""
    want = {}
    for d in diagonals:
        want[d - 1] = 1
    for start, n in runs:
        want[start] = n
    out, pos = [], 0
    for start in sorted(want):
        assert start >= pos, "planted pairs overlap"
        out.extend(rng.choice("AB") for _ in range(start - pos))
        out.extend("P" * want[start])
        pos = start + 2 * want[start]
    assert pos <= total
    out.extend(rng.choice("AB") for _ in range(total - pos))
    return "".join(out)


def _bound_rules(a, b, op, mode):
    """bounds exactly at, one below and one above a result count, bounds that empty the result, the full bounds"""
    out, _ = model(a, b, op, mode)
    rules = [(op, mode, 0, U32)]
    if out:
        counts = sorted(out.values())
        c = counts[len(counts) // 2]
        for lo, hi in ((c, U32), (c + 1, U32), (max(c - 1, 0), U32), (0, c), (0, max(c - 1, 0)), (0, c + 1), (c, c), (counts[-1] + 1, U32), (0, counts[0] - 1)):
            if 0 <= lo <= hi <= U32:
                rules.append((op, mode, lo, hi))
    return rules


def _case(name, kw, kb, a, b, kind, same=False, planted=(), sizes=None, bounds=False):
    rules = [(op, mode, 0, U32) for op, mode in OP_MODES]
    if bounds:
        bb = a if same else b
        for op, mode in ((UNION, SUM), (INTERSECT, MIN), (COUNT_SUBTRACT, LEFT), (SUBTRACT, LEFT)):
            rules += _bound_rules(a, bb, op, mode)[1:]
    case = dict(name=name, key_words=kw, key_bits=kb, a=a, b=b, same=same, planted=list(planted), kind=kind, rules=rules)
    if sizes is not None:
        case["sizes"] = sizes
    return case


def sizes(kw):
    g = geometry()
    T, I = g["TILE"][kw], g["ITEMS"][kw]
    return [(0, 0), (0, 1), (1, 0), (1, 1), (I - 1, 1), (I, I), (I + 1, I), (T // 2, T - 1 - T // 2), (T // 2, T - T // 2), (T // 2 + 1, T - T // 2),
            (3 * T // 2, 3 * T + 1 - 3 * T // 2), (4097, 63)]


_CACHE = {}


def cases():
    """every case, built once (the tests share them and leave them unchanged)"""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    g = geometry()
    rng = random.Random(20241)
    out = []
    for kw in (1, 2):
        T, I = g["TILE"][kw], g["ITEMS"][kw]
        for kb in KEY_BITS[kw]:
            # sizes: about half of the smaller table is shared; key_bits = 2 takes the sizes that fit in its four keys
            for n_a, n_b in sizes(kw):
                pairs = min(n_a, n_b) // 2 if min(n_a, n_b) > 1 else 0
                if n_a + n_b - pairs > (1 << kb):
                    continue
                a, b = from_layout(rng, _shuffled(rng, n_a, n_b, pairs), kb)
                out.append(_case(f"size-{n_a}-{n_b}-w{kw}-b{kb}", kw, kb, a, b, "size", sizes=(n_a, n_b)))
            if kb == 2:
                a, b = from_layout(rng, "PPPP", kb)
                out.append(_case(f"all-four-keys-w{kw}-b{kb}", kw, kb, a, b, "relation", planted=(1, 3, 5, 7), bounds=True))
                continue
            n = T + 3 * I + 1
            # relations
            a, b = from_layout(rng, "P" * n, kb)
            out.append(_case(f"equal-w{kw}-b{kb}", kw, kb, a, b, "relation"))
            out.append(_case(f"same-object-w{kw}-b{kb}", kw, kb, a, None, "relation", same=True))
            a, _ = from_layout(rng, "A" * n, kb)
            out.append(_case(f"b-null-w{kw}-b{kb}", kw, kb, a, None, "relation", bounds=True))
            a, b = from_layout(rng, "AB" * n, kb)
            out.append(_case(f"interleaved-w{kw}-b{kb}", kw, kb, a, b, "relation"))
            a, b = from_layout(rng, "A" * n + "B" * (n + 5), kb)
            out.append(_case(f"a-below-b-w{kw}-b{kb}", kw, kb, a, b, "relation"))
            a, b = from_layout(rng, "B" * n + "A" * (n + 5), kb)
            out.append(_case(f"b-below-a-w{kw}-b{kb}", kw, kb, a, b, "relation"))
            a, b = from_layout(rng, "".join(rng.choice("AP") for _ in range(2 * n)), kb)
            out.append(_case(f"b-subset-w{kw}-b{kb}", kw, kb, a, b, "relation"))
            a, b = from_layout(rng, _shuffled(rng, 2 * n, 2 * n, n), kb)
            out.append(_case(f"random-half-w{kw}-b{kb}", kw, kb, a, b, "random", bounds=True))
            # planted pairs: across thread diagonals (the first, one inside a wave, one at a wave's edge), across tile diagonals, across
            # the very last diagonal that has anything behind it (a thread's: the B partner is the last merged element and the only one
            # of its thread; below, the same with a tile's), and a run of T pairs
            total = 3 * T + 2 * I + 1
            thread_d = [I, 5 * I, 64 * I, T + 3 * I, 2 * T + 255 * I]
            tile_d = [T, 2 * T, 3 * T]
            a, b = from_layout(rng, planted_layout(rng, total, thread_d + tile_d + [total - 1]), kb)
            out.append(_case(f"planted-diagonals-w{kw}-b{kb}", kw, kb, a, b, "planted", planted=thread_d + tile_d + [total - 1], bounds=True))
            a, b = from_layout(rng, planted_layout(rng, T + 1, [T]), kb)
            out.append(_case(f"planted-last-tile-w{kw}-b{kb}", kw, kb, a, b, "planted", planted=[T]))
            start = T // 2 + 1  # odd: the run has a pair across the tile edge T and another across 2 T
            a, b = from_layout(rng, planted_layout(rng, 3 * T, [], runs=[(start, T)]), kb)
            out.append(_case(f"planted-run-w{kw}-b{kb}", kw, kb, a, b, "planted", planted=[T, 2 * T, start + 1, start + 2 * T - 1]))
            # only a pair: both elements of the table, the diagonal between them the only inner one
            a, b = from_layout(rng, "P", kb)
            out.append(_case(f"planted-only-pair-w{kw}-b{kb}", kw, kb, a, b, "planted", planted=[1]))
    # 16-byte keys that agree in one word and differ in the other: a compare of one word only calls them equal
    for name, make in (("same-low", lambda v: (v << 64) | 7), ("same-high", lambda v: (9 << 64) | v)):
        a = {make(v): 1 + v % 3 for v in range(0, 60, 2)}
        b = {make(v): 2 + v % 5 for v in range(0, 60, 3)}
        out.append(_case(f"words-{name}", 2, 128, a, b, "words", bounds=True))
    # counts: the saturating sum at its edge, the count subtraction at its edge, stored zeros
    a = {1: U32 - 1, 2: U32, 3: 1 << 31, 4: U32 - 1, 5: 0, 6: 0, 7: 3, 8: 5, 9: 6, 10: 7, 11: 0, 12: U32}
    b = {1: 1, 2: 1, 3: 1 << 31, 4: 0, 5: 0, 6: 4, 7: 5, 8: 5, 9: 5, 12: U32, 13: 0, 14: 9}
    for kw, kb in ((1, 62), (2, 102)):
        out.append(_case(f"counts-w{kw}", kw, kb, dict(a), dict(b), "counts", bounds=True))
    for case in out:
        check_case(case)
    _CACHE["cases"] = out
    return out


def big_case():
    """about 2^20 + 2^20 one-word keys, half shared (numpy: the dict model would dominate the test) -> keys and counts of A and B"""
    rng = np.random.default_rng(7)
    n = 1 << 20
    keys = np.unique(rng.integers(0, 1 << 62, 3 * n // 2 + 4096, dtype=np.int64))[: 3 * n // 2]
    pick = rng.permutation(keys.size)
    ka, kb = np.sort(keys[pick[:n]]), np.sort(keys[pick[n // 2: n // 2 + n]])
    return ka, rng.integers(1, 1000, ka.size, dtype=np.int64), kb, rng.integers(1, 1000, kb.size, dtype=np.int64)


# ----------------------------------------------------------------------------- the emulation program's input

def key_words_of(keys, kw):
    """uint64 array: one or two words (low, high) per key"""
    arr = np.empty((len(keys), kw), np.uint64)
    for i, x in enumerate(keys):
        arr[i, 0] = x & M64
        if kw == 2:
            arr[i, 1] = x >> 64
    return arr


def emu_file(case, limit=0):
    """uint32 key_words, uint32 n_rules, uint64 na, uint64 nb, uint64 limit (0: the library's); A keys, A counts, B keys, B counts;
    the rules as four uint32 each"""
    a = case["a"]
    b = a if case["same"] else (case["b"] or {})
    kw = case["key_words"]
    blob = struct.pack("<IIQQQ", kw, len(case["rules"]), len(a), len(b), limit)
    for t in (a, b):
        ks = sorted(t)
        blob += key_words_of(ks, kw).tobytes() + np.array([t[x] for x in ks], np.uint32).tobytes()
    return blob + np.array(case["rules"], np.uint32).tobytes()
