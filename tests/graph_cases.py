"""TEST INFRASTRUCTURE: the Python model of the compacted de Bruijn graph of a count table (bl_table_adjacency, bl_table_unitigs) and the
named tables of its tests (tests/test_graph_model.py on strings, tests/test_emu_graph.py on the host emulation, tests/test_gpu_graph.py
on the device).  Keys are Python integers, first base in the most significant pair, A C G T = 0 1 2 3; a table is a dict key -> count of
canonical k-mers, k odd.  The model is the specification (include/biolib_amd.h states it in words); it walks every unitig key by key and
shares no code and no method with the library, which labels by pointer doubling.
"""
import functools
import struct

import numpy as np

import lookup_cases as LC

NONE = 0xFFFFFFFF
LEFT, RIGHT = 0, 1
KS = (1, 3, 5, 15, 31, 33, 63)
STAT_NAMES = ("n_keys", "n_arcs", "n_isolated", "n_dead_end_sides", "n_branch_sides", "n_linked_sides", "n_unitigs", "n_cycles", "longest_unitig")
ADJ_STATS = STAT_NAMES[:6]
PATH_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025)
LONG_PATH = 70000
OPTIONS = (0, 1, 24)  # forced "table_prefix_bits": one bucket for every candidate; two; 2^24 buckets, nearly all of them empty
NODE = np.dtype([("unitig", "<u4"), ("rank_flip", "<u4")])


def rc(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canon(x, k):
    return min(x, rc(x, k))


def encode(s):
    x = 0
    for ch in s:
        x = (x << 2) | "ACGT".index(ch)
    return x


def decode(x, k):
    return "".join("ACGT"[(x >> (2 * (k - 1 - j))) & 3] for j in range(k))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def keys_of(seqs, k):
    """the canonical k-mers of the strings"""
    out = set()
    for s in seqs:
        for p in range(len(s) - k + 1):
            out.add(canon(encode(s[p:p + k]), k))
    return out


def table_of(keys, seed=7):
    """a count for every key: 1 .. 2^32 - 1, both ends of the range among them"""
    rng = np.random.default_rng(seed + len(keys))
    ks = sorted(keys)
    counts = [int(c) for c in rng.integers(1, 1 << 32, len(ks), dtype=np.uint64)]
    if len(ks) > 1:
        counts[0], counts[-1] = (1 << 32) - 1, 1
    return dict(zip(ks, counts))


def adjacency(keys, k):
    """keys: sorted list.  -> mask (list of bytes), links (list of 2n words), and the neighbours of every side (lists of (slot, side))"""
    slot = {x: i for i, x in enumerate(keys)}
    top = 1 << (2 * k)
    mask, sides = [], []
    for x in keys:
        m, right, left = 0, [], []
        for c in range(4):
            f = ((x << 2) | c) % top
            y = canon(f, k)
            if y in slot:
                m |= 1 << c
                right.append((slot[y], LEFT if y == f else RIGHT))
            f = (x >> 2) | (c << (2 * k - 2))
            y = canon(f, k)
            if y in slot:
                m |= 16 << c
                left.append((slot[y], RIGHT if y == f else LEFT))
        mask.append(m)
        sides.append((left, right))
    links = [NONE] * (2 * len(keys))
    for i in range(len(keys)):
        for s in (LEFT, RIGHT):
            if len(sides[i][s]) == 1:
                j, t = sides[i][s][0]
                if j != i and len(sides[j][t]) == 1:
                    links[2 * i + s] = (j << 1) | t
    return mask, links, sides


def walk(links, start, out, cut=None):
    """the keys from `start` leaving through side `out`: [(slot, flip)], stopping at a side without link, at the cut side, or in front of the start"""
    path = [(start, 0 if out == RIGHT else 1)]
    cur = start
    while True:
        if cut is not None and (cur, out) == cut:
            break
        nxt = links[2 * cur + out]
        if nxt == NONE:
            break
        j, t = nxt >> 1, nxt & 1
        if j == start:
            break
        path.append((j, t))  # entered through its left side: read as stored
        cur, out = j, 1 - t
    return path


def unitigs(keys, links):
    """-> list of (path [(slot, flip)], is_cycle), ordered by the slot of the start key"""
    n = len(keys)
    seen = [False] * n
    out = []
    for i in range(n):
        if seen[i]:
            continue
        # the component of i: to the right end, or round the cycle
        fwd = walk(links, i, RIGHT)
        last, last_flip = fwd[-1]
        closes = links[2 * last + (RIGHT if last_flip == 0 else LEFT)]
        if closes != NONE and (closes >> 1) == i and links[2 * i + LEFT] != NONE and len(fwd) > 1:
            members = [j for j, _ in fwd]
            s = min(members)
            path, cyc = walk(links, s, RIGHT), True
        else:
            back = walk(links, i, LEFT)
            a, b = fwd[-1][0], back[-1][0]  # the two end keys
            if a == b:
                assert len(fwd) == 1 and len(back) == 1
                path = [(i, 0)]
            else:
                s = min(a, b)
                side = RIGHT if links[2 * s + RIGHT] != NONE else LEFT
                assert links[2 * s + (1 - side)] == NONE
                path = walk(links, s, side)
            cyc = False
        for j, _ in path:
            assert not seen[j], "a key lies in one unitig"
            seen[j] = True
        out.append((path, cyc))
    out.sort(key=lambda u: u[0][0][0])
    return out


def model(table, k):
    """everything the library returns for the table, as plain numpy / Python values"""
    keys = sorted(table)
    n = len(keys)
    mask, links, sides = adjacency(keys, k)
    us = unitigs(keys, links)
    nodes = np.zeros(n, NODE)
    offsets, sums, strings = [0], [], []
    for u, (path, _) in enumerate(us):
        s = ""
        for r, (j, flip) in enumerate(path):
            nodes[j] = (u, (r << 1) | flip)
            o = decode(rc(keys[j], k) if flip else keys[j], k)
            s += o if r == 0 else o[-1]
        strings.append(s)
        offsets.append(offsets[-1] + len(s))
        sums.append(sum(table[keys[j]] for j, _ in path) & LC.M64)
    deg = [len(sides[i][s]) for i in range(n) for s in (LEFT, RIGHT)]
    arcs = sum(bin(m).count("1") for m in mask)
    assert arcs == sum(deg)
    stats = dict(n_keys=n, n_arcs=arcs, n_isolated=sum(1 for m in mask if m == 0), n_dead_end_sides=sum(1 for d in deg if d == 0),
                 n_branch_sides=sum(1 for d in deg if d >= 2), n_linked_sides=sum(1 for x in links if x != NONE), n_unitigs=len(us),
                 n_cycles=sum(1 for _, c in us if c), longest_unitig=max((len(p) for p, _ in us), default=0))
    return dict(keys=keys, mask=np.array(mask, np.uint8), links=np.array(links, np.uint32), nodes=nodes, offsets=np.array(offsets, np.uint64),
                sums=np.array(sums, np.uint64), strings=strings, bases=np.frombuffer("".join(strings).encode(), np.uint8), stats=stats,
                unitigs=us)


def check_invariants(table, k, m):
    """what must hold of any table: symmetric links, every key in one unitig, the k-mers of the strings are the keys, the sums add up"""
    keys, links = m["keys"], m["links"]
    for s, x in enumerate(links):
        if x != NONE:
            assert links[2 * (int(x) >> 1) + (int(x) & 1)] == s, "links are symmetric"
            assert (int(x) >> 1) != s >> 1
    got = []
    for s in m["strings"]:
        got += [canon(encode(s[p:p + k]), k) for p in range(len(s) - k + 1)]
    assert sorted(got) == keys, "the canonical k-mers of the unitigs are the keys, each once"
    assert int(sum(int(x) for x in m["sums"])) & LC.M64 == sum(table.values()) & LC.M64
    assert sorted(int(u) for u in m["nodes"]["unitig"]) == sorted(u for u, (p, _) in enumerate(m["unitigs"]) for _ in p)


# ------------------------------------------------------------------------------------------------------------------------ the named cases

def _rand_seq(rng, n, letters="ACGT"):
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


def _other(ch, by=1):
    return "ACGT"[("ACGT".index(ch) + by) % 4]


@functools.lru_cache(maxsize=None)
def cases(k):
    """[(name, table)] at this k: the small shapes, the cycles, the degenerate tables and the orientation cases that exist at k"""
    rng = np.random.default_rng(1000 + k)
    out = []

    def add(name, seqs=(), keys=()):
        ks = keys_of(seqs, k) | set(keys)
        out.append((name, table_of(ks)))

    add("empty")
    add("single_key", [_rand_seq(rng, k)])
    if k >= 3:
        add("two_unlinked_keys", [_rand_seq(rng, k), _rand_seq(rng, k)])
    path = _rand_seq(rng, k + 11)
    add("straight_path", [path])
    stem = _rand_seq(rng, k + 3)
    add("fork", [stem + "A" + _rand_seq(rng, k), stem + "C" + _rand_seq(rng, k)])
    add("merge", [_rand_seq(rng, k) + "G" + stem, _rand_seq(rng, k) + "T" + stem])
    a, b = _rand_seq(rng, k + 2), _rand_seq(rng, k + 2)
    add("snp_bubble", [a + "A" + b, a + "C" + b])
    add("tip", [a + "G" + b, a + "T" + _rand_seq(rng, 2)])
    w = _rand_seq(rng, k + 4)
    add("hairpin", [w + revcomp(w)])
    if k == 1:
        add("double_arc", keys=[0])  # A: the bases A and T both lead to the key A
    add("homopolymer_self_arc", ["A" * (k + 1) + _rand_seq(rng, k)])
    genome = _rand_seq(rng, 4 * k + 9)
    add("pure_cycle", [genome + genome[:k - 1]])
    if k >= 3:
        add("two_key_cycle", [("AC" * k)[:k + 1]])
    if k <= 3:
        add("all_keys", keys=[x for x in range(4 ** k) if x <= rc(x, k)])
    add("start_at_the_smaller_end", [_wrong_start_path(rng, k)])
    if k >= 5:
        add("alternating_flips", [_alternating_path(rng, k)])
    add("two_letter_repeats", [_rand_seq(rng, 6 * k + 40, "AC"), _rand_seq(rng, 3 * k + 5, "AT")])
    add("random_keys", keys=[canon(int.from_bytes(rng.bytes(16), "little") % (4 ** k), k) for _ in range(300)])
    return out


def _path_of(seq, k):
    """the unitigs of the string's table when they are one path, else None"""
    t = table_of(keys_of([seq], k))
    keys = sorted(t)
    _, links, _ = adjacency(keys, k)
    us = unitigs(keys, links)
    return (keys, us[0][0]) if len(us) == 1 and not us[0][1] else None


def _wrong_start_path(rng, k):
    """a path of four or more keys whose first k-mer as written has the LARGER slot of the two ends (a walk from the string's first k-mer,
    or from the end with the larger slot, reads the unitig the wrong way round); small k: the best the alphabet gives"""
    for _ in range(400):
        s = _rand_seq(rng, k + 5)
        p = _path_of(s, k)
        if p and len(p[1]) >= 4 and p[0].index(canon(encode(s[:k]), k)) > p[0].index(canon(encode(s[-k:]), k)):
            return s
    return s


def _alternating_path(rng, k):
    """a path of four or more keys along which the flips go 0 1 0 1 (or as near as 2,000 draws come)"""
    best, best_n = None, -1
    for _ in range(2000):
        s = _rand_seq(rng, k + 3)
        p = _path_of(s, k)
        if not p:
            continue
        flips = [f for _, f in p[1]]
        n = sum(1 for x, y in zip(flips[:-1], flips[1:]) if x != y)
        if n > best_n:
            best, best_n = s, n
        if n == len(flips) - 1 and len(flips) >= 4:
            break
    return best


@functools.lru_cache(maxsize=None)
def path_case(n_keys, k=31):
    """the table of a random string with n_keys k-mers (at k = 31 one unitig for every length here: checked by the caller's model run)"""
    rng = np.random.default_rng(77 + n_keys)
    return table_of(keys_of([_rand_seq(rng, n_keys + k - 1)], k))


def table_file(table, k, key_words, key_bits, option):
    """the emulation program's input: five words, then the keys (one or two words each) and the counts"""
    keys = sorted(table)
    return (struct.pack("<5Q", key_words, key_bits, len(keys), k, option) + LC.words(keys, key_words).tobytes()
            + np.array([table[x] for x in keys], np.uint32).tobytes())


def widths(k):
    """(key_words, key_bits) a table of k-mers is stored with in the tests"""
    if k <= 30:
        return ((1, 2 * k),)
    if k == 31:
        return ((1, 62), (2, 62))
    return ((2, 2 * k),)
