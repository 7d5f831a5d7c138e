"""A numpy model of bl_scan_read_quality and bl_spans_intersect (include/biolib_amd.h) and the named cases that the model test
(test_quality_model.py), the emulation (test_emu_quality.py) and the GPU tests (test_gpu_quality.py) share.  The model is the
specification; it is written from the header's text with numpy's cumulative sums, and test_quality_model.py checks it against a
restatement with plain loops.

  rule(**changes)                          -> dict: a bl_quality_rule, neutral except for the changes
  phred_values(qual_bytes, rule)           -> int64 [L]
  trim_model(v, rule)                      -> (b, e)
  read_model(qual_bytes | None, bases, rule) -> dict: the fields of bl_read_quality
  batch_model(reads, rule)                 -> (records [n] of RECORD, spans uint64 [n, 2], stats dict)
  intersect_model(lengths, a, b, paired)   -> uint64 [n, 2]
  reads()                                  -> [(name, bases, qual)]: the named reads, qual as bytes at Phred+33
  rules()                                  -> {name: rule}
  fastq(reads, shift=0) / fasta(reads)     -> bytes: the text of the reads (shift: added to every quality byte, 31 for Phred+64)
"""
from decimal import ROUND_FLOOR, Decimal, getcontext

import numpy as np

U32, U64 = (1 << 32) - 1, (1 << 64) - 1
RECORD = np.dtype([("begin", "<u8"), ("end", "<u8"), ("sum", "<u8"), ("ee", "<u8"), ("n_low", "<u4"), ("n_ambiguous", "<u4"), ("q_min", "u1"),
                   ("q_max", "u1"), ("failed", "<u2"), ("reserved", "<u4")])
FAIL = dict(min_len=1, max_len=2, ambiguous=4, low=8, mean=16, ee=32)
STATS = ("n_reads", "n_reads_kept", "n_bases", "n_bases_kept", "n_too_short", "n_too_long", "n_ambiguous", "n_low", "n_mean", "n_ee")
RULE_WORDS = ("phred_base", "quality_fill", "front_q", "back_q", "maxsum_front_q", "maxsum_back_q", "window_len", "window_q", "low_q", "low_max_num",
              "low_max_den", "mean_q", "max_ambiguous", "reserved", "min_len", "max_len", "max_ee")


def phred_err():
    """BL_PHRED_ERR: floor(2^31 * 10^(-q/10) + 1/2) for q = 0 .. 93, computed in decimal arithmetic"""
    getcontext().prec = 60
    return np.array([int((Decimal(2) ** 31 * Decimal(10) ** (Decimal(-q) / Decimal(10)) + Decimal("0.5")).to_integral_value(rounding=ROUND_FLOOR))
                     for q in range(94)], np.uint64)


PHRED_ERR = phred_err()
# the scans' encoder takes every byte but ACGTU in either case as invalid (bl_scan_core.hpp: encode4)
VALID_BASE = np.zeros(256, bool)
VALID_BASE[list(b"ACGTUacgtu")] = True


def rule(**changes):
    r = dict(phred_base=33, quality_fill=ord("I"), front_q=0, back_q=0, maxsum_front_q=0, maxsum_back_q=0, window_len=0, window_q=0, low_q=0, low_max_num=1,
             low_max_den=1, mean_q=0, max_ambiguous=U32, reserved=0, min_len=0, max_len=0, max_ee=U64)
    assert set(changes) <= set(r), changes
    r.update(changes)
    return r


def rule_words(r):
    return [int(r[k]) for k in RULE_WORDS]


def phred_values(qual, r):
    return np.clip(np.asarray(qual, np.uint8).astype(np.int64) - r["phred_base"], 0, 93)


def trim_steps(v, r):
    """the span after each of the steps: [(b, e) at the start, after A front, A back, B, C's cut, C's trailing walk]"""
    L = len(v)
    b, e = 0, L
    out = [(b, e)]
    # A, edges
    if r["front_q"]:
        hit = np.nonzero(v[b:e] >= r["front_q"])[0]
        b = b + int(hit[0]) if len(hit) else e
    out.append((b, e))
    if r["back_q"]:
        hit = np.nonzero(v[b:e] >= r["back_q"])[0]
        e = b + int(hit[-1]) + 1 if len(hit) else b
    out.append((b, e))
    # B, running sum: both ends on step A's span, in the closed form
    if (r["maxsum_front_q"] or r["maxsum_back_q"]) and e > b:
        b2, e2 = b, e
        if r["maxsum_back_q"]:
            S = np.cumsum((r["maxsum_back_q"] - v[b:e])[::-1])[::-1]  # S[i - b] = the sum over [i, e)
            neg = np.nonzero(S < 0)[0]
            first = int(neg[-1]) + 1 if len(neg) else 0
            cand = S[first:]
            if len(cand) and cand.max() > 0:
                e2 = b + first + int(np.nonzero(cand == cand.max())[0][-1])  # on ties the largest i
        if r["maxsum_front_q"]:
            P = np.cumsum(r["maxsum_front_q"] - v[b:e])
            neg = np.nonzero(P < 0)[0]
            cand = P[:int(neg[0])] if len(neg) else P
            if len(cand) and cand.max() > 0:
                b2 = b + int(np.argmax(cand)) + 1  # on ties the smallest i
        b, e = b2, max(b2, e2)
    out.append((b, e))
    # C, window
    W = r["window_len"]
    cut = False
    if W and e - b >= W:
        c = np.concatenate([[0], np.cumsum(v[b:e])])
        sums = c[W:] - c[:-W]
        bad = np.nonzero(sums < W * r["window_q"])[0]
        if len(bad):
            e = b + int(bad[0])
            cut = True
    out.append((b, e))
    if cut:
        keep = np.nonzero(v[b:e] >= r["window_q"])[0]
        e = b + int(keep[-1]) + 1 if len(keep) else b
    out.append((b, e))
    return out


def trim_model(v, r):
    return trim_steps(v, r)[-1]


def read_model(qual, bases, r):
    """qual: the read's quality bytes, or None (a FASTA index): the fill everywhere"""
    bases = np.frombuffer(bytes(bases), np.uint8)
    q = np.full(len(bases), r["quality_fill"], np.uint8) if qual is None else np.frombuffer(bytes(qual), np.uint8)
    assert len(q) == len(bases)
    v = phred_values(q, r)
    b, e = trim_model(v, r)
    s = v[b:e]
    n = e - b
    rec = dict(begin=b, end=e, sum=int(s.sum()), ee=int(PHRED_ERR[s].sum()), n_low=int((s < r["low_q"]).sum()),
               n_ambiguous=int((~VALID_BASE[bases[b:e]]).sum()), q_min=int(s.min()) if n else 255, q_max=int(s.max()) if n else 0)
    f = 0
    if n < r["min_len"]:
        f |= FAIL["min_len"]
    if r["max_len"] and n > r["max_len"]:
        f |= FAIL["max_len"]
    if rec["n_ambiguous"] > r["max_ambiguous"]:
        f |= FAIL["ambiguous"]
    if rec["n_low"] * r["low_max_den"] > n * r["low_max_num"]:
        f |= FAIL["low"]
    if rec["sum"] < r["mean_q"] * n:
        f |= FAIL["mean"]
    if rec["ee"] > r["max_ee"]:
        f |= FAIL["ee"]
    rec["failed"] = f
    return rec


def batch_model(rs, r, fasta_index=False):
    """rs: [(name, bases, qual)] -> (records, spans, stats)"""
    recs = np.zeros(len(rs), RECORD)
    spans = np.zeros((len(rs), 2), np.uint64)
    st = dict.fromkeys(STATS, 0)
    for i, (_, bases, qual) in enumerate(rs):
        m = read_model(None if fasta_index else qual, bases, r)
        for k, x in m.items():
            recs[i][k] = x
        if m["failed"] == 0:
            spans[i] = (m["begin"], m["end"])
        n = m["end"] - m["begin"]
        kept = m["failed"] == 0 and n > 0
        st["n_reads"] += 1
        st["n_reads_kept"] += kept
        st["n_bases"] += len(bases)
        st["n_bases_kept"] += n if kept else 0
        for bit, name in enumerate(("n_too_short", "n_too_long", "n_ambiguous", "n_low", "n_mean", "n_ee")):
            st[name] += (m["failed"] >> bit) & 1
    return recs, spans, {k: int(x) for k, x in st.items()}


def intersect_model(lengths, a, b=None, paired=False):
    lengths = np.asarray(lengths, np.uint64)
    a = np.minimum(np.asarray(a, np.uint64).reshape(-1, 2), lengths[:, None])
    lo, hi = a[:, 0], a[:, 1]
    if b is not None:
        b = np.minimum(np.asarray(b, np.uint64).reshape(-1, 2), lengths[:, None])
        lo, hi = np.maximum(lo, b[:, 0]), np.minimum(hi, b[:, 1])
    empty = hi <= lo
    if paired:
        assert len(lengths) % 2 == 0
        pair = empty.reshape(-1, 2).any(axis=1)
        empty = np.repeat(pair, 2)
    out = np.stack([lo, hi], axis=1)
    out[empty] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------- the named reads

def dna(n, seed):
    return np.random.default_rng(1000 + seed).choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()


def q33(values):
    return (np.asarray(values, np.int64) + 33).astype(np.uint8).tobytes()


# the lengths at which the kernel changes its body or a lane, a group or a chunk ends: a lane holds 16 positions, the short body 256, a
# wave 1,024 in registers; windows of 4, 64 and 65
LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 66, 150, 255, 256, 257, 1023, 1024, 1025, 2049, 5003)


def reads():
    """[(name, bases, qual)]: realistic reads of every length, then reads built against one step each"""
    rng = np.random.default_rng(7)
    out = []

    def add(name, values, bases=None):
        values = np.asarray(values, np.int64)
        out.append((name.encode(), dna(len(values), len(out)) if bases is None else bases, q33(values)))

    for L in LENGTHS:
        # a good middle between degraded ends, as sequencers make them
        x = np.arange(L)
        v = np.clip(38 - (np.maximum(0, 6 - x) * 5) - np.maximum(0, x - (L - 1 - L // 3)) * (60 / max(L, 1)) + rng.integers(-6, 3, L), 2, 41)
        add("len%d" % L, v)
        add("noise%d" % L, rng.integers(0, 42, L))
    for L in (1, 16, 150, 256, 257, 1024, 1025, 3000):
        add("all_low%d" % L, np.full(L, 2))
        add("all_high%d" % L, np.full(L, 40))
    # one failing window of 4 at every place around a lane's end (16), a group's end (256) and a chunk's end (1,024)
    for L, places in ((150, (12, 13, 14, 15, 16, 146)), (300, (253, 254, 255, 256)), (1500, (1021, 1022, 1023, 1024)), (2500, (2045, 2046, 2047, 2048))):
        for at in places:
            v = np.full(L, 36)
            v[at:at + 4] = (19, 19, 19, 22)
            v[max(at - 2, 0):at] = 18  # the trailing walk has something to take
            add("window_at%d_of%d" % (at, L), v)
    # a window that fails only at the read's last place, and one value short of failing
    v = np.full(150, 30)
    v[-4:] = (19, 20, 20, 20)
    add("window_last", v)
    v[-4:] = (20, 20, 20, 20)
    add("window_none", v)
    # step B, back: ties of the maximum (the sum returns to its best value: the largest i wins), for cutoff 20
    for L in (40, 300, 1100, 2100):
        v = np.full(L, 30)
        v[-6:] = (10, 30, 10, 30, 10, 30)[::-1]  # from the back: +10 -10 +10 -10 +10 -10 -> the best sum 10 three times
        add("maxsum_back_ties%d" % L, v)
        v = np.full(L, 30)
        v[:6] = (10, 30, 10, 30, 10, 30)
        add("maxsum_front_ties%d" % L, v)
    # step B: the sum dips below 0 and recovers behind the stop: what lies further in must not count
    for L in (60, 300, 1100, 2100):
        v = np.full(L, 21)
        v[-3:] = 15           # +15 from the back
        v[-20:-3] = 21        # -17: the sum is -2 at the 20th value from the back: the walk stops
        v[:L - 20] = 2        # a better sum further in, which the walk never sees
        add("maxsum_back_dip%d" % L, v)
        add("maxsum_front_dip%d" % L, v[::-1])
    # step B across a chunk's end: a long bad tail
    for L, tail in ((1100, 200), (2100, 1100)):
        v = np.full(L, 35)
        v[-tail:] = rng.integers(2, 22, tail)
        add("maxsum_back_tail%d" % L, v)
        add("maxsum_front_head%d" % L, v[::-1])
    # edges
    for L in (17, 150, 1030, 2100):
        v = np.full(L, 30)
        v[:L // 3] = 5
        v[-(L // 4):] = 7
        add("edges%d" % L, v)
    # the filters: Ns, long and short, poor
    add("many_n", np.full(150, 35), bases=b"N" * 20 + dna(110, 1) + b"nRYK" * 5)
    add("one_n", np.full(150, 35), bases=dna(75, 2) + b"N" + dna(74, 3))
    add("lowercase_u", np.full(16, 35), bases=b"acgtuACGTU" + b"acgtuA")
    add("all_letters", rng.integers(0, 42, 260), bases=(bytes(range(65, 91)) + bytes(range(97, 123))) * 5)
    add("poor_mean", np.full(150, 14))
    add("half_low", np.tile([10, 36], 75))
    add("high_values", rng.integers(60, 94, 150))   # bytes up to 126
    add("n_at_the_end", np.full(30, 35), bases=dna(29, 9) + b"N")
    assert len(out) % 2 == 0  # (the reads also serve as mates)
    return out


def rules():
    return {
        "neutral": rule(),
        "front": rule(front_q=20),
        "back": rule(back_q=20),
        "edges": rule(front_q=20, back_q=25),
        "maxsum_back": rule(maxsum_back_q=20),
        "maxsum_front": rule(maxsum_front_q=20),
        "maxsum_both": rule(maxsum_front_q=20, maxsum_back_q=20),
        "window1": rule(window_len=1, window_q=20),
        "window4": rule(window_len=4, window_q=20),
        "window64": rule(window_len=64, window_q=25),
        "window65": rule(window_len=65, window_q=25),
        "window_wide": rule(window_len=1500, window_q=30),
        "fastp": rule(window_len=4, window_q=20, low_q=15, low_max_num=2, low_max_den=5, min_len=50),
        "filters": rule(min_len=30, max_len=1024, max_ambiguous=2, low_q=15, low_max_num=1, low_max_den=4, mean_q=25, max_ee=1 << 31),
        "all_steps": rule(front_q=10, back_q=10, maxsum_front_q=18, maxsum_back_q=18, window_len=4, window_q=22, low_q=20, low_max_num=1, low_max_den=2,
                          mean_q=20, max_ambiguous=0, min_len=16, max_len=3000, max_ee=3 << 31),
        "threshold94": rule(front_q=94),
        "fill_low": rule(quality_fill=ord("#"), window_len=4, window_q=20, mean_q=10),
    }


def fastq(rs, shift=0):
    out = []
    for name, bases, qual in rs:
        q = (np.frombuffer(qual, np.uint8).astype(np.int64) + shift).astype(np.uint8).tobytes()
        out.append(b"@" + name + b"\n" + bases + b"\n+\n" + q + b"\n")
    return b"".join(out)


def fasta(rs):
    return b"".join(b">" + name + b"\n" + bases + b"\n" for name, bases, _ in rs)


TEXT_RECORD = np.dtype([("name_begin", "<u8"), ("name_len", "<u4"), ("qual_delta", "<u4")])


def layout(rs, pad=0, newline_at_end=True):
    """what bl_text_index_build keeps of fastq(rs), made on the host for the emulation: dict(text, records, offsets, bases).  The quality
    bytes go in verbatim, so they may be any of the 256 values here.  pad: bytes added to the first name, which moves every later byte."""
    text, recs, offsets, bases = bytearray(), np.zeros(len(rs), TEXT_RECORD), [0], bytearray()
    for i, (name, b, q) in enumerate(rs):
        name = name + b"x" * pad if i == 0 else name
        recs[i]["name_begin"] = len(text) + 1
        recs[i]["name_len"] = len(name)
        recs[i]["qual_delta"] = len(name) + 1 + len(b) + 1 + 2
        text += b"@" + name + b"\n" + b + b"\n+\n" + q + b"\n"
        bases += b
        offsets.append(len(bases))
    if not newline_at_end and len(text):
        del text[-1]
    return dict(text=bytes(text), records=recs, offsets=np.array(offsets, np.uint64), bases=bytes(bases))


def parse_fastq(text):
    """[(name, bases, qual)] of a four-line FASTQ text"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def paired_text(n_pairs, read_len=150, seed=11):
    """interleaved mates with degraded tails and some Ns: (text, reads)"""
    rng = np.random.default_rng(seed)
    rs = []
    for i in range(n_pairs):
        for mate in (1, 2):
            good = int(rng.integers(0, read_len + 1)) if rng.random() < 0.5 else read_len
            v = np.concatenate([rng.integers(30, 41, good), rng.integers(2, 18, read_len - good)])
            bases = bytearray(dna(read_len, 5000 + 2 * i + mate))
            for at in rng.integers(0, read_len, int(rng.integers(0, 4)) if rng.random() < 0.2 else 0):
                bases[at] = ord("N")
            rs.append((b"pair%d/%d" % (i, mate), bytes(bases), q33(v)))
    return fastq(rs), rs
