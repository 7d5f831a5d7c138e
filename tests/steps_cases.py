"""TEST INFRASTRUCTURE: the Python model of the reads' steps through the compacted graph (bl_scan_read_steps), of the link support
(bl_link_support) and of the GAF text (bl_steps_format_gaf), and the reads of their tests (tests/test_steps_model.py on strings,
tests/test_emu_steps.py on the host emulation, tests/test_gpu_steps.py on the device).  Built on graph_cases.model and
links_cases.links; the model is the specification (include/biolib_amd.h states it in words).  It looks every k-mer up in a dictionary
from key to slot and walks the positions one by one: it shares no code and no method with the library, which searches the sorted keys
and compacts heads and tails by prefix sums."""
import functools
import struct

import numpy as np

import graph_cases as GC
import links_cases as LK
import lookup_cases as LC

LINKED, CONTINUED = 1, 2
M64 = (1 << 64) - 1
STEP = np.dtype([("pos", "<u8"), ("seq", "<u8"), ("end", "<u4"), ("offset", "<u4"), ("n_kmers", "<u4"), ("flags", "<u4")])
STEP_STAT_NAMES = ("n_valid", "n_found", "n_steps", "n_chains", "n_linked", "longest_step")
# (read_prefix, read_first_number, segment_prefix, segment_first_number) of the GAF texts
GAF_RULES = (("read", 0, "", 0), ("", 1, "utg", 1), ("fifteen_bytes_r", (1 << 32) - 2, "fifteen_bytes_x", (1 << 64) - 2))
SEAM_K = 31
SEAMS = dict(across=(16, 1024, 4096), ending=(160, 2048, 8192), hole=(176, 3072, 12288))


class Reads:
    """a batch: the bases, the n_seqs + 1 offsets and the fixed read length (0: ragged)"""

    def __init__(self, reads, fixed=0):
        self.reads = list(reads)
        self.fixed = int(fixed)
        assert not fixed or all(len(r) == fixed for r in self.reads)
        self.text = "".join(self.reads)
        self.bases = np.frombuffer(self.text.encode(), np.uint8)
        self.offsets = np.cumsum([0] + [len(r) for r in self.reads]).astype(np.uint64)
        self.n_bases, self.n_seqs = len(self.text), len(self.reads)


def position_nodes(m, k, batch):
    """for every position of the batch: (seq, node) where node is (end, offset) or None.  The sequence of a position is the LAST one whose
    offset is <= the position."""
    slot = {x: i for i, x in enumerate(m["keys"])}
    n_unitigs = len(m["strings"])
    out = []
    for q, read in enumerate(batch.reads):
        for p in range(len(read)):
            node = None
            w = read[p:p + k]
            if len(w) == k and all(ch in "ACGT" for ch in w):
                f = GC.encode(w)
                c = GC.canon(f, k)
                i = slot.get(c)
                if i is not None and int(m["nodes"][i]["unitig"]) < n_unitigs:
                    u, rf = int(m["nodes"][i]["unitig"]), int(m["nodes"][i]["rank_flip"])
                    o = (1 if f != c else 0) ^ (rf & 1)
                    L = len(m["unitigs"][u][0])
                    node = ((u << 1) | o, (rf >> 1) if o == 0 else L - 1 - (rf >> 1))
            out.append((q, node))
    return out


def valid_positions(k, batch):
    out = []
    for read in batch.reads:
        out += [len(read[p:p + k]) == k and all(ch in "ACGT" for ch in read[p:p + k]) for p in range(len(read))]
    return out


def steps(m, k, batch, first=0, n=0, nodes=None):
    """-> (records as a STEP array, stats) of the range"""
    nodes = nodes if nodes is not None else position_nodes(m, k, batch)
    end = batch.n_bases if n == 0 or n > batch.n_bases - first else first + n

    def continues(p):
        if p == 0:
            return False
        (qa, a), (qb, b) = nodes[p - 1], nodes[p]
        return qa == qb and a is not None and b is not None and a[0] == b[0] and b[1] == a[1] + 1

    out = []
    for p in range(first, end):
        q, node = nodes[p]
        if node is None:
            continue
        if p > first and continues(p):
            out[-1][4] += 1
            continue
        flags = 0
        if p > 0 and nodes[p - 1][0] == q and nodes[p - 1][1] is not None:
            flags = CONTINUED if continues(p) else LINKED
        out.append([p, q, node[0], node[1], 1, flags])
    valid = valid_positions(k, batch)
    stats = dict(n_valid=sum(valid[first:end]), n_found=sum(1 for p in range(first, end) if nodes[p][1] is not None), n_steps=len(out),
                 n_chains=sum(1 for s in out if s[5] == 0), n_linked=sum(1 for s in out if s[5] & LINKED), longest_step=max((s[4] for s in out), default=0))
    return np.array([tuple(s) for s in out], STEP).reshape(-1), stats


def fold(records):
    """the records of consecutive ranges concatenated: every CONTINUED record goes into its predecessor"""
    out = []
    for s in records:
        if int(s["flags"]) & CONTINUED:
            out[-1]["n_kmers"] += s["n_kmers"]
        else:
            out.append(s.copy())
    return np.array(out, STEP).reshape(-1)


def transitions(recs):
    return [(int(a["end"]), int(b["end"])) for a, b in zip(recs[:-1], recs[1:]) if int(b["flags"]) & LINKED and int(a["seq"]) == int(b["seq"])]


def support(recs, link_records):
    """-> (support per record, stats)"""
    index = {r: i for i, r in enumerate(link_records)}
    out = [0] * len(link_records)
    stats = dict(n_transitions=0, n_unmatched=0)
    for a, b in transitions(recs):
        hit = {index[r] for r in ((a, b), (b ^ 1, a ^ 1)) if r in index}
        for i in hit:
            out[i] = (out[i] + 1) & 0xFFFFFFFF
        stats["n_transitions"] += 1
        stats["n_unmatched"] += not hit
    return np.array(out, np.uint32), stats


def chains(recs):
    """the steps grouped: a step without LINKED and every following one with it"""
    out = []
    for i, s in enumerate(recs):
        if i == 0 or not int(s["flags"]) & LINKED:
            out.append([])
        out[-1].append(s)
    return out


def gaf_lines(m, k, batch, recs, read_prefix="read", read_first=0, seg_prefix="", seg_first=0):
    out = []
    for chain in chains(recs):
        s0 = chain[0]
        q = int(s0["seq"])
        K = sum(int(s["n_kmers"]) for s in chain)
        qstart = int(s0["pos"]) - int(batch.offsets[q])
        path = b"".join((b"<" if int(s["end"]) & 1 else b">") + seg_prefix.encode("latin1") + str((seg_first + (int(s["end"]) >> 1)) & M64).encode() for s in chain)
        plen = sum(len(m["unitigs"][int(s["end"]) >> 1][0]) for s in chain) + k - 1
        mm = K + k - 1
        fields = [read_prefix.encode("latin1") + str((read_first + q) & M64).encode(), len(batch.reads[q]), qstart, qstart + mm, "+", path, plen, int(s0["offset"]),
                  int(s0["offset"]) + mm, mm, mm, 255]
        out.append(b"\t".join(f if isinstance(f, bytes) else str(f).encode() for f in fields) + b"\n")
    return out


# ------------------------------------------------------------------------------------------------------------------------ the reads

def _out_records(lk):
    by_end = {}
    for a, b in lk["records"]:
        by_end.setdefault(a, []).append(b)
    return by_end


def _walk_string(m, k, by_end, rng, n_unitigs):
    """a random walk over the link records: the spelled string and the ends visited"""
    e = int(rng.integers(0, 2 * len(m["strings"])))
    ends = [e]
    s = LK.oriented(m["strings"][e >> 1], e & 1)
    while len(ends) < n_unitigs and by_end.get(e):
        e = by_end[e][int(rng.integers(0, len(by_end[e])))]
        ends.append(e)
        s += LK.oriented(m["strings"][e >> 1], e & 1)[k - 1:]
    return s, ends


def _cut(m, k, s, ends, rng):
    """cut at random inner offsets of the first and the last unitig; at least one k-mer stays"""
    a = int(rng.integers(0, len(m["unitigs"][ends[0] >> 1][0])))
    b = int(rng.integers(0, len(m["unitigs"][ends[-1] >> 1][0])))
    if len(ends) == 1 and a + b >= len(m["unitigs"][ends[0] >> 1][0]):
        b = 0
    return s[a:len(s) - b]


def reads_for(name, table, k, m=None):
    """the reads of one table: [(what, string)]"""
    m = m if m is not None else GC.model(table, k)
    rng = np.random.default_rng(sum(map(ord, name)) * 131 + k)
    out = [("k_minus_1", GC._rand_seq(rng, k - 1)), ("empty", ""), ("random", GC._rand_seq(rng, 3 * k + 7)), ("empty", "")]
    strings = m["strings"]
    if not strings:
        return out + [("k", GC._rand_seq(rng, k)), ("k_plus_1", GC._rand_seq(rng, k + 1))]
    for u, s in enumerate(strings[:40]):
        out += [("unitig+", s), ("unitig-", GC.revcomp(s))]
    lk = LK.links(m, k)
    by_end = _out_records(lk)
    walks = []
    for j in range(8):
        s, ends = _walk_string(m, k, by_end, rng, 1 + j % 6)
        walks.append(_cut(m, k, s, ends, rng))
    out += [("walk", w) for w in walks]
    for w in walks[:4]:
        at = int(rng.integers(0, len(w)))
        out.append(("substitution", w[:at] + GC._other(w[at], 1 + int(rng.integers(0, 3))) + w[at + 1:]))
    w = max(walks, key=len)
    out.append(("n_in_the_middle", w[:len(w) // 2] + "N" + w[len(w) // 2 + 1:]))
    long = max(strings, key=len)
    out += [("k", long[:k]), ("k_plus_1", (long + GC._rand_seq(rng, 1))[:k + 1]), ("empty", "")]
    for u, (path, cyc) in enumerate(m["unitigs"]):
        if cyc:
            ring = strings[u][:len(path)]
            out.append(("cycle_2.5_times", (ring * (4 + k // len(path)))[:len(path) * 5 // 2 + k - 1]))
            break
    for a, b in lk["records"]:
        if b == a ^ 1:  # a hairpin: u in orientation o, then the same unitig the other way round
            s = LK.oriented(strings[a >> 1], a & 1)
            out.append(("hairpin", s + GC.revcomp(s)[k - 1:]))
            break
    return out


def batches_for(name, table, k, m=None):
    """[(form, Reads)]: the reads of the table as a ragged batch, and those long enough cut to one length as a fixed-length batch"""
    reads = [r for _, r in reads_for(name, table, k, m)]
    out = [("ragged", Reads(reads))]
    fixed = k + 5
    cut = [r[:fixed] for r in reads if len(r) >= fixed] + [r[-fixed:] for r in reads if len(r) >= 2 * fixed]
    if len(cut) > 1:
        out.append(("fixed", Reads(cut, fixed)))
    return out


@functools.lru_cache(maxsize=None)
def seam_case():
    """(table, model, Reads): about 12,400 bases at k = 31 laid out so that a step lies across the positions 16, 1,024 and 4,096 (the seams
    of a lane, a wave and a tile of the node pass), a step ends exactly in front of 160, 2,048 and 8,192, and a run without nodes lies
    across 176 (no k-mer), 3,072 and 12,288 (k-mers that are not in the table)"""
    k = SEAM_K
    rng = np.random.default_rng(31031)
    genome = GC._rand_seq(rng, 3000)
    stem = genome[1000:1000 + k - 1]
    table = GC.table_of(GC.keys_of([genome, stem + GC._other(genome[1000 + k - 1]) + GC._rand_seq(rng, 40)], k))
    m = GC.model(table, k)
    reads, at = [], 0

    def piece(n):
        a = int(rng.integers(0, len(genome) - n))
        s = genome[a:a + n]
        return GC.revcomp(s) if rng.integers(0, 2) else s

    def add(s):
        nonlocal at
        reads.append(s)
        at += len(s)

    def fill(target):
        while at < target:
            n = min(int(rng.integers(k - 2, 220)), target - at)
            add(piece(n) if n >= k else GC._rand_seq(rng, n))

    add(piece(41 + k - 1))                       # nodes 0 .. 40: across 16
    add(piece(160 - at + k - 1))                 # the last node at 159; 160 .. 189 hold no k-mer: across 176
    fill(1000)
    add(piece(51 + k - 1))                       # nodes 1000 .. 1050
    fill(2000)
    add(piece(48 + k - 1))                       # the last node at 2047
    fill(3050)
    add(GC._rand_seq(rng, 50 + k - 1))           # 3050 .. 3099: k-mers outside the table
    fill(4050)
    add(piece(101 + k - 1))                      # nodes 4050 .. 4150
    fill(8100)
    add(piece(92 + k - 1))                       # the last node at 8191
    fill(12250)
    add(GC._rand_seq(rng, 80 + k - 1))           # 12250 .. 12329
    fill(12400)
    return table, m, Reads(reads)


def cut_batch(k=31):
    """(table, model, Reads) of 300 bases for the cut at every position: walks over a fork, a substitution, an N and a short read"""
    name, table = "fork", dict(GC.cases(k))["fork"]
    m = GC.model(table, k)
    reads = [r for what, r in reads_for(name, table, k, m) if what in ("walk", "substitution", "n_in_the_middle", "k", "empty", "unitig-")]
    text, out = 0, []
    for r in reads:
        if text + len(r) > 300:
            r = r[:300 - text]
        out.append(r)
        text += len(r)
        if text == 300:
            break
    while text < 300:
        r = reads[0][:300 - text]
        out.append(r)
        text += len(r)
    return table, m, Reads(out)


# ------------------------------------------------------------------------------------------------------------------------ the emulation's input

def steps_file(table, k, key_words, key_bits, option, m, batch, link_model, ranges, rule=GAF_RULES[0], mode=0):
    """sixteen words and the two 16-byte prefixes, then keys, nodes, unitig offsets, sequence offsets, bases, link offsets, link records and
    the ranges (first, n).  mode 0: the ranges; 1: every cut position; 2: garbage"""
    keys = sorted(table)
    rp, sp = rule[0].encode("latin1"), rule[2].encode("latin1")
    recs = np.array(link_model["records"], np.uint32).reshape(-1, 2)
    head = struct.pack("<16Q", key_words, key_bits, len(keys), k, option, len(m["strings"]), batch.n_bases, batch.n_seqs, batch.fixed, len(recs), len(ranges),
                       mode, rule[1] & M64, rule[3] & M64, len(rp), len(sp))
    return (head + rp.ljust(16, b"\0") + sp.ljust(16, b"\0") + LC.words(keys, key_words).tobytes() + m["nodes"].tobytes() + m["offsets"].astype(np.uint64).tobytes()
            + batch.offsets.tobytes() + batch.bases.tobytes() + np.array(link_model["offsets"], np.uint64).tobytes() + recs.tobytes()
            + np.array(ranges, np.uint64).reshape(-1, 2).tobytes())
