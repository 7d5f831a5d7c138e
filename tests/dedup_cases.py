"""A model of bl_scan_read_duplicates (include/biolib_amd.h) in plain Python and numpy, and the named cases that the model test
(test_dedup_model.py), the emulation (test_emu_dedup.py) and the GPU tests (test_gpu_dedup.py) share.  The model is the specification: a
dict over canonicalised key strings.  It knows nothing of a hash; test_dedup_model.py checks it against a restatement with plain loops.

  rule(**changes)                                        -> dict: a bl_dedup_rule, everything off except for the changes
  rule_struct(rule)                                      -> one element of RULE (32 bytes)
  codes(bases)                                           -> int64 [L]: 0 .. 3, 4 for a base the encoder takes as invalid
  batch_model(reads, rule, spans_in=None, scores=None)   -> (records [n_units] of RECORD, spans uint64 [n, 2], stats dict)
  cases()                                                -> {name: Case(reads, rule, spans_in | None, scores | None, read_len)}
  layout(reads)                                          -> dict(bases, offsets) of the batch
"""
import collections
import functools

import numpy as np

U32, U64 = (1 << 32) - 1, (1 << 64) - 1
RECORD = np.dtype([("first", "<u4"), ("kept", "<u4"), ("copies", "<u4"), ("flags", "<u4")])
RULE = np.dtype([("flags", "<u4"), ("hash_bits", "<u4"), ("prefix_len", "<u8"), ("seed", "<u8"), ("reserved", "<u8")])
assert RECORD.itemsize == 16 and RULE.itemsize == 32
PAIRED, CANONICAL = 1, 2
DUPLICATE, EMPTY, REVERSED = 1, 2, 4
STATS = ("n_units", "n_empty", "n_classes", "n_duplicates", "n_reversed", "largest_class", "n_reads_kept", "n_bases_kept")   # then class_hist[16]

# the scans' encoder (bl_scan_core.hpp: encode4): ACGT in either case, U as T; everything else is the fifth letter
CODE = np.full(256, 4, np.int64)
for _c, _letters in enumerate((b"Aa", b"Cc", b"Gg", b"TtUu")):
    CODE[list(_letters)] = _c

Case = collections.namedtuple("Case", "reads rule spans_in scores read_len")


def codes(bases):
    return CODE[np.frombuffer(bytes(bases), np.uint8)]


def rule(**changes):
    r = dict(flags=0, hash_bits=0, prefix_len=0, seed=0, reserved=0)
    assert set(changes) <= set(r), changes
    r.update(changes)
    return r


def rule_struct(r):
    s = np.zeros(1, RULE)
    for k in RULE.names:
        s[k] = r[k]
    return s


def layout(reads):
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    return dict(bases=b"".join(reads), offsets=offsets)


# ---------------------------------------------------------------------------------------------------------------- the model

def clamp(span, L):
    """bl_batch_select's clamp of an input span to a read of L bases; an empty one is (0, 0)"""
    b, e = min(int(span[0]), L), min(int(span[1]), L)
    return (b, e) if e > b else (0, 0)


def read_key(read, span, prefix_len):
    """the key of a read as a string over the letters 0 .. 4, and its clamped span"""
    b, e = clamp(span, len(read)) if span is not None else clamp((0, len(read)), len(read))
    k = codes(read[b:e])
    if prefix_len:
        k = k[:prefix_len]
    return bytes(k.astype(np.uint8)), (b, e)


RC = bytes([3, 2, 1, 0, 4]) + bytes(range(5, 256))


def rc_key(k):
    return k.translate(RC)[::-1]


def batch_model(reads, r, spans_in=None, scores=None):
    paired, canonical = bool(r["flags"] & PAIRED), bool(r["flags"] & CANONICAL)
    per = 2 if paired else 1
    n = len(reads)
    assert n % per == 0
    n_units = n // per
    keys, spans = [], []
    for i, x in enumerate(reads):
        k, s = read_key(x, None if spans_in is None else spans_in[i], r["prefix_len"])
        keys.append(k)
        spans.append(s)
    records = np.zeros(n_units, RECORD)
    out = np.zeros((n, 2), np.uint64)
    classes = {}
    forward = {}
    for u in range(n_units):
        ks = tuple(keys[per * u:per * u + per])
        if any(len(k) == 0 for k in ks):
            records[u] = (u, u, 0, EMPTY)
            for i in range(per * u, per * u + per):
                out[i] = spans[i]
            continue
        forward[u] = ks
        name = ks
        if canonical:
            name = min(ks, ks[::-1]) if paired else min(ks, (rc_key(ks[0]),))
        classes.setdefault(name, []).append(u)
    hist = [0] * 16
    for members in classes.values():
        def score(u):
            return 0 if scores is None else sum(int(scores[i]) for i in range(per * u, per * u + per)) & U64
        kept = max(members, key=lambda u: (score(u), -u))
        hist[min(len(members), 16) - 1] += 1
        for u in members:
            flags = (DUPLICATE if u != kept else 0) | (REVERSED if forward[u] != forward[kept] else 0)
            records[u] = (members[0], kept, len(members), flags)
            if u == kept:
                for i in range(per * u, per * u + per):
                    out[i] = spans[i]
    flags = records["flags"]
    kept_spans = out[:, 1] > out[:, 0]
    stats = dict(n_units=n_units, n_empty=int((flags & EMPTY != 0).sum()), n_classes=len(classes), n_duplicates=int((flags & DUPLICATE != 0).sum()),
                 n_reversed=int((flags & REVERSED != 0).sum()), largest_class=max([len(m) for m in classes.values()], default=0),
                 n_reads_kept=int(kept_spans.sum()), n_bases_kept=int((out[:, 1] - out[:, 0])[kept_spans].sum()), class_hist=hist)
    return records, out, stats


# ---------------------------------------------------------------------------------------------------------------- the named cases

COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(x):
    return bytes(x).translate(COMPLEMENT)[::-1]


def dna(n, seed, letters=b"ACGT"):
    return np.random.default_rng(7000 + seed).choice(np.frombuffer(letters, np.uint8), n).tobytes()


def changed(x, at, to=None):
    """x with the base at `at` replaced by `to`, or by a base that differs"""
    y = bytearray(x)
    y[at] = to if to is not None else (ord("C") if y[at] in b"AaNn" else ord("A"))
    return bytes(y)


# a chunk holds 16 bases, a word 32, sixteen lanes take 512 bases a turn
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, 511, 512, 513, 1023, 1024, 1025, 5000)
HIST_SIZES = tuple(range(1, 17)) + (20,)


def _volume():
    rng = np.random.default_rng(11)
    base = [dna(150, 100 + i) for i in range(752)]
    reads = base + [base[int(j)] for j in rng.integers(0, 752, 250)]   # 1,002 reads, a quarter of them copies
    return [reads[int(i)] for i in rng.permutation(len(reads))]


@functools.lru_cache(maxsize=None)
def cases():
    """(computed once; nobody changes it)"""
    c = {}
    # lengths: a read, its copy and the read with another last base, at every length; two empty reads
    reads = []
    for L in LENGTHS:
        x = dna(L, L)
        reads += [x, x] + ([changed(x, L - 1)] if L else [])
    c["lengths"] = Case(reads, rule(), None, None, 0)
    c["lengths_canonical"] = Case(reads + [revcomp(x) for x in reads[::3]], rule(flags=CANONICAL), None, None, 0)
    # a read starts at every residue mod 32 of the batch: one base, then reads of 33
    three = [dna(33, 40 + i) for i in range(3)]
    c["residues"] = Case([b"G"] + [three[(i * i) % 3] for i in range(40)], rule(), None, None, 0)
    # keys that differ in one place only: the first base, the last base, a trailing A, N against A; every variant twice
    reads = []
    for L in (3, 16, 17, 32, 33, 64, 65, 150, 513):
        x = changed(dna(L, 60 + L), L // 2, ord("A"))
        reads += [x, changed(x, 0), changed(x, L - 1), x + b"A", changed(x, L // 2, ord("N")), changed(x + b"A", L, ord("N"))]
    c["one_difference"] = Case(reads + reads[::-1], rule(), None, None, 0)
    # letters: N n . \0 are one letter, u T t U another, case is ignored
    x = b"ACGTNACGTTGCAN" * 5
    reads = [x, x.lower(), x.replace(b"N", b"."), x.replace(b"N", b"\0"), x.replace(b"N", b"n"), x.replace(b"T", b"u"), x.replace(b"T", b"U"),
             x.replace(b"T", b"t"), x.replace(b"N", b"A"), x.replace(b"T", b"N"), x.replace(b"N", b"-").replace(b"A", b"a")]
    c["letters"] = Case(reads, rule(), None, None, 0)
    # canonical: a read and its reverse complement, a palindrome, an N inside; with and without the flag
    half = dna(37, 70)
    reads = []
    for L in (1, 31, 32, 33, 64, 100, 150, 1025):
        x = dna(L, 80 + L)
        xn = changed(changed(x, L // 3, ord("N")), L - 1, ord("n"))
        reads += [x, revcomp(x), xn, revcomp(xn).replace(b"N", b"."), revcomp(changed(x, 0))]
    reads += [half + revcomp(half), revcomp(half + revcomp(half)), b"ACGT", b"ACGT", b"N", b"n", b"AT", b"TA"]
    c["canonical_off"] = Case(reads, rule(), None, None, 0)
    c["canonical_on"] = Case(reads, rule(flags=CANONICAL), None, list(range(len(reads))), 0)
    # pairs: (s1, s2) against (s1, s3), against (s2, s1), one empty mate, both empty
    s1, s2, s3, s4 = dna(150, 90), dna(150, 91), dna(150, 92), dna(33, 93)
    reads = [s1, s2, s1, s3, s1, s2, s2, s1, s1, b"", b"", s2, b"", b"", s4, s1, s1, s4, s4, s1, revcomp(s2), revcomp(s1), s3, s1, s1, s1, s1, s1, s4 + b"A", s1]
    c["pairs"] = Case(reads, rule(flags=PAIRED), None, None, 0)
    c["pairs_canonical"] = Case(reads, rule(flags=PAIRED | CANONICAL), None, None, 0)
    # prefix_len: equal in the first 50 bases and different behind; a read shorter than the prefix against a longer one that starts with it
    head = dna(50, 94)
    reads = [head + dna(100, 95), head + dna(100, 96), head + dna(7, 97), head[:40], head[:40] + dna(30, 98), head[:40], changed(head, 49) + dna(100, 95), head]
    c["prefix"] = Case(reads, rule(prefix_len=50), None, None, 0)
    c["prefix_pairs"] = Case(reads, rule(prefix_len=50, flags=PAIRED | CANONICAL), None, None, 0)
    # input spans: different reads made equal, equal reads made different, empty and garbage spans
    core = dna(70, 99)
    reads = [dna(9, 1) + core + dna(5, 2), dna(20, 3) + core, core + dna(40, 4), core, core, core, core, core, core, dna(33, 5), dna(33, 5)]
    spans = [(9, 79), (20, 90), (0, 70), (0, 69), (1, 70), (5, 5), (7, 3), (1 << 63, U64), (0, U64), (3, 10 ** 12), (3, 33)]
    c["spans_in"] = Case(reads, rule(), np.array(spans, np.uint64), None, 0)
    c["spans_in_pairs"] = Case(reads + [core], rule(flags=PAIRED | CANONICAL), np.array(spans + [(0, 70)], np.uint64), None, 0)
    # scores: a later member wins, a tie goes to the lower index, the sum of a pair wraps
    a, b = dna(150, 6), dna(64, 7)
    c["scores"] = Case([a, b, a, b, a, b, revcomp(a)], rule(flags=CANONICAL), None, [5, 9, 7, 9, 7, 1, 8], 0)
    c["scores_pairs"] = Case([a, b, a, b, a, b, b, a], rule(flags=PAIRED), None, [U64, 3, 5, 5, U64 - 1, 0, 1 << 63, 1 << 63], 0)
    # class sizes 1 .. 16 and 20: every bin of the histogram
    rng = np.random.default_rng(12)
    reads = [dna(100 + k, 200 + k) for k in HIST_SIZES for _ in range(k)]
    c["class_sizes"] = Case([reads[int(i)] for i in rng.permutation(len(reads))], rule(), None, None, 0)
    # volume: 1,002 reads of 150 bases, fixed-length and ragged (some of them a base shorter)
    reads = _volume()
    c["volume_fixed"] = Case(reads, rule(), None, None, 150)
    c["volume_ragged"] = Case([x[:149] if i % 7 == 0 else x for i, x in enumerate(reads)], rule(), None, None, 0)
    c["volume_pairs_canonical"] = Case([revcomp(x) if i % 5 == 0 else x for i, x in enumerate(reads[:300] + reads[:300][::-1])],
                                       rule(flags=PAIRED | CANONICAL, prefix_len=100), None, [(i * 37) % 11 for i in range(600)], 150)
    c["volume_canonical"] = Case([revcomp(x) if i % 3 == 0 else x for i, x in enumerate(reads[:300])], rule(flags=CANONICAL, seed=7), None, None, 150)
    return c


# the bins of class_hist that the cases fill, by name (test_dedup_model.py checks the claim)
HIST_CLAIMS = {"class_sizes": tuple(range(16)), "volume_fixed": (0, 1), "lengths": (0, 1)}
