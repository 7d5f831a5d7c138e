"""TEST INFRASTRUCTURE: the Python model of the links between unitig ends (bl_unitig_links) and of the GFA text (bl_unitigs_format_gfa), and the
named tables of their tests (tests/test_links_model.py on strings, tests/test_emu_links.py on the host emulation, tests/test_gpu_links.py
on the device).  Built on graph_cases.model and graph_cases.adjacency; the model is the specification (include/biolib_amd.h states it in
words).  It walks the neighbour lists of every end and shares no code and no method with the library, which searches the sorted keys."""
import bisect
import functools
import struct

import numpy as np

import graph_cases as GC
import lookup_cases as LC

LEFT, RIGHT = GC.LEFT, GC.RIGHT
KS = (3, 5, 15, 31, 33, 63)
ONCE = 1
LINK_STAT_NAMES = ("n_ends", "n_links", "n_self_reverse", "n_dead_ends", "n_branch_ends")
HEADER = b"H\tVN:Z:1.0\n"
M64 = (1 << 64) - 1
# (prefix, first_number, header) of the GFA texts: names that cross 2^32 and wrap at 2^64 among them
RULES = (("", 0, True), ("utg", 1, False), ("fifteen_bytes_x", (1 << 32) - 2, True), ("u", (1 << 64) - 2, True))


def links(m, k, once=False):
    """m: graph_cases.model(table, k).  -> dict(ends, records, offsets, stats): ends[e] = (slot, side), records = [(from, to)] in CSR order"""
    keys, nodes, us = m["keys"], m["nodes"], m["unitigs"]
    _, _, sides = GC.adjacency(keys, k)
    ends = []
    for path, _ in us:
        (first, f0), (last, f1) = path[0], path[-1]
        ends.append((last, RIGHT if f1 == 0 else LEFT))   # + : the side the walk leaves its last key by
        ends.append((first, LEFT if f0 == 0 else RIGHT))  # - : the side the walk entered its first key by
    for e, (i, s) in enumerate(ends):
        assert e & 1 == (1 if s == LEFT else 0) ^ (int(nodes[i]["rank_flip"]) & 1), "o = (s == left) XOR f"
    records, offsets, degrees, self_reverse = [], [0], [], 0
    for e, (i, s) in enumerate(ends):
        degrees.append(len(sides[i][s]))
        for j, t in sides[i][s]:  # ascending base c
            v, rf = int(nodes[j]["unitig"]), int(nodes[j]["rank_flip"])
            to = (v << 1) | ((1 if t == RIGHT else 0) ^ (rf & 1))
            assert ends[to ^ 1] == (j, t), "every `to` lands on an end: v read in orientation o is entered by its end of the other sign"
            assert (rf >> 1) == (0 if to & 1 == 0 else len(us[v][0]) - 1), "rank 0 where v is read forward, L - 1 where reversed"
            self_reverse += e == to ^ 1
            if once and e > to ^ 1:
                continue
            records.append((e, to))
        offsets.append(len(records))
    stats = dict(n_ends=len(ends), n_links=len(records), n_self_reverse=self_reverse, n_dead_ends=sum(1 for d in degrees if d == 0),
                 n_branch_ends=sum(1 for d in degrees if d >= 2))
    return dict(ends=ends, records=records, offsets=offsets, stats=stats, array=np.array(records, np.uint32).reshape(-1, 2))


def _name(prefix, first_number, u):
    return prefix.encode("latin1") + str((first_number + u) & M64).encode()


def gfa_lines(m, records, k, prefix="", first_number=0, header=True, sums=True):
    """the lines of the text, each built field by field with its terminator"""
    out = [HEADER] if header else []
    for u, s in enumerate(m["strings"]):
        line = b"S\t" + _name(prefix, first_number, u) + b"\t" + s.encode() + b"\tLN:i:" + str(len(s)).encode()
        if sums:
            line += b"\tKC:i:" + str(int(m["sums"][u])).encode()
        out.append(line + b"\n")
    for a, b in records:
        a, b = int(a), int(b)
        out.append(b"L\t" + _name(prefix, first_number, a >> 1) + b"\t" + b"+-"[a & 1:(a & 1) + 1] + b"\t" + _name(prefix, first_number, b >> 1) + b"\t"
                   + b"+-"[b & 1:(b & 1) + 1] + b"\t" + str(k - 1).encode() + b"M\n")
    return out


class GfaText:
    """the text as a positional byte function: byte(x) finds the line of x by its offset and reads the byte there"""

    def __init__(self, lines):
        self.lines = lines
        self.starts = [0]
        for line in lines:
            self.starts.append(self.starts[-1] + len(line))
        self.total = self.starts[-1]

    def byte(self, x):
        j = bisect.bisect_right(self.starts, x) - 1
        return self.lines[j][x - self.starts[j]]

    def bytes(self):
        return b"".join(self.lines)


def oriented(s, o):
    return GC.revcomp(s) if o else s


def string_links(strings, k):
    """the restatement on strings: all ordered pairs of oriented unitig strings whose (k - 1)-suffix and (k - 1)-prefix agree"""
    by_prefix = {}
    for v, s in enumerate(strings):
        for b in (0, 1):
            by_prefix.setdefault(oriented(s, b)[:k - 1], []).append((v << 1) | b)
    out = set()
    for u, s in enumerate(strings):
        for a in (0, 1):
            for to in by_prefix.get(oriented(s, a)[len(s) - (k - 1):], ()):
                out.add(((u << 1) | a, to))
    return out


# ------------------------------------------------------------------------------------------------------------------------ the named cases

@functools.lru_cache(maxsize=None)
def canonical_kmers(k):
    return [x for x in range(4 ** k) if x <= GC.rc(x, k)]


def _random_keys(k, count, seed):
    rng = np.random.default_rng(seed)
    canon = canonical_kmers(k)
    return [canon[i] for i in sorted(rng.choice(len(canon), count, replace=False))]


@functools.lru_cache(maxsize=None)
def dense_cases():
    """[(name, k, table)]: dense random key sets, which give many branching ends; the last has more than 10,000 unitigs, so that names
    cross 9 -> 10, 99 -> 100, 999 -> 1,000 and 9,999 -> 10,000"""
    out = [("all_keys", 3, dict(GC.cases(3))["all_keys"])]
    out.append(("dense_300_of_512", 5, GC.table_of(_random_keys(5, 300, 5))))
    out.append(("dense_5000_of_8192", 7, GC.table_of(_random_keys(7, 5000, 7))))
    out.append(("dense_40000", 9, GC.table_of(_random_keys(9, 40000, 9))))
    return out


@functools.lru_cache(maxsize=None)
def dense_model(name):
    for n, k, table in dense_cases():
        if n == name:
            return k, table, GC.model(table, k)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def forked_path(n_forks, cycle=False, k=31):
    """a path_case-style table with planted forks: a random string, and at n_forks places along it a second string that shares k - 1 bases
    with it and then leaves.  Every fork adds two unitigs, four ends and four records (two with ONCE), so that their counts step past a
    wave and a workgroup: 2f + 1 unitigs, 4f records.  cycle: a pure cycle beside it, one unitig and two records more (one with ONCE)."""
    rng = np.random.default_rng(4000 + n_forks)
    main = GC._rand_seq(rng, 40 * (n_forks + 1) + k)
    seqs = [main]
    if cycle:
        ring = GC._rand_seq(rng, 3 * k)
        seqs.append(ring + ring[:k - 1])
    for f in range(n_forks):
        at = 40 * (f + 1)
        seqs.append(main[at:at + k - 1] + GC._other(main[at + k - 1]) + GC._rand_seq(rng, 3))
    return GC.table_of(GC.keys_of(seqs, k))


def links_file(table, k, key_words, key_bits, option, m, prefix, first_number, header):
    """the emulation program's input: ten words and the 16 bytes of the prefix, then keys, nodes, offsets, sums and bases"""
    keys = sorted(table)
    p = prefix.encode("latin1")
    assert len(p) < 16
    return (struct.pack("<10Q", key_words, key_bits, len(keys), k, option, len(m["strings"]), len(m["bases"]), first_number, 1 if header else 0, len(p))
            + p.ljust(16, b"\0") + LC.words(keys, key_words).tobytes() + m["nodes"].tobytes() + m["offsets"].astype(np.uint64).tobytes()
            + m["sums"].astype(np.uint64).tobytes() + m["bases"].tobytes())
