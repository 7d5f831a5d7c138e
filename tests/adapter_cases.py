"""A numpy model of bl_scan_read_adapters (include/biolib_amd.h) and the named cases that the model test (test_adapter_model.py), the
emulation (test_emu_adapters.py) and the GPU tests (test_gpu_adapters.py) share.  The model is the specification; it is written from the
header's text with numpy's cumulative sums and sliding windows, and test_adapter_model.py checks it against a restatement with plain
loops.

  rule(**changes)                              -> dict: a bl_adapter_rule, everything off except for the changes
  rule_words(rule)                             -> uint32 array: the struct's 154 words
  codes(bases)                                 -> int64 [L]: 0 .. 3, 4 for a base the encoder takes as invalid
  poly_model / pair_model / adapter_model      -> the steps on their own
  batch_model(reads, rule, spans_in=None)      -> (records [n] of RECORD, spans uint64 [n, 2], stats dict)
  cases()                                      -> {name: (reads, rule, spans_in | None)}: reads a list of bytes
  layout(reads)                                -> dict(bases, offsets) of the batch
"""
import numpy as np

U32, U64 = (1 << 32) - 1, (1 << 64) - 1
RECORD = np.dtype([("begin", "<u8"), ("end", "<u8"), ("match_pos", "<u4"), ("insert", "<u4"), ("adapter", "<u2"), ("overlap", "u1"), ("mismatches", "u1"),
                   ("pair_mismatches", "<u2"), ("cut", "u1"), ("reserved", "u1")])
assert RECORD.itemsize == 32
CUT = dict(poly_before=1, pair=2, adapter=4, poly_after=8, too_short=16, pair_skipped=32)
PAIRED = 1
MAX_ADAPTERS, ADAPTER_MAX, PAIR_MAX = 8, 64, 512
STATS = ("n_reads", "n_reads_cut", "n_reads_kept", "n_bases", "n_bases_kept", "n_poly_before", "n_pair", "n_adapter", "n_poly_after", "n_too_short",
         "n_pair_skipped")
RULE = np.dtype([("flags", "<u4"), ("n_adapters", "<u4"), ("adapter_len", "<u4", 8), ("adapters", "S64", 8), ("min_overlap", "<u4"), ("error_num", "<u4"),
                 ("error_den", "<u4"), ("pair_min_overlap", "<u4"), ("pair_error_num", "<u4"), ("pair_error_den", "<u4"), ("pair_max_diff", "<u4"),
                 ("poly_before", "<u4"), ("poly_after", "<u4"), ("poly_min_len", "<u4"), ("poly_per", "<u4"), ("poly_max_mismatch", "<u4"), ("reserved", "<u4"),
                 ("pad", "<u4"), ("min_len", "<u8")])
assert RULE.itemsize == 616

ADAPTERS = {"truseq": b"AGATCGGAAGAGC", "nextera": b"CTGTCTCTTATACACATCT", "small_rna": b"TGGAATTCTCGGGTGCCAAGG"}
TRUSEQ = ADAPTERS["truseq"]

# the scans' encoder (bl_scan_core.hpp: encode4): ACGT in either case, U as T; everything else is invalid
CODE = np.full(256, 4, np.int64)
for _c, _letters in enumerate((b"Aa", b"Cc", b"Gg", b"TtUu")):
    CODE[list(_letters)] = _c


def codes(bases):
    return CODE[np.frombuffer(bytes(bases), np.uint8)]


def poly_mask(letters):
    m = 0
    for ch in bytes(letters):
        assert CODE[ch] < 4
        m |= 1 << int(CODE[ch])
    return m


def rule(**changes):
    r = dict(flags=0, adapters=[], min_overlap=3, error_num=1, error_den=10, pair_min_overlap=30, pair_error_num=1, pair_error_den=5, pair_max_diff=5,
             poly_before=0, poly_after=0, poly_min_len=10, poly_per=8, poly_max_mismatch=5, reserved=0, min_len=0)
    assert set(changes) <= set(r), changes
    r.update(changes)
    return r


def rule_struct(r):
    """the bl_adapter_rule of r as one element of RULE (n_adapters and adapter_len may be overridden for the refusals)"""
    s = np.zeros(1, RULE)
    ads = [bytes(a) for a in r["adapters"]]
    s["flags"] = r["flags"]
    s["n_adapters"] = r.get("n_adapters", len(ads))
    for a, text in enumerate(ads[:MAX_ADAPTERS]):
        s["adapter_len"][0][a] = r.get("adapter_len", {}).get(a, len(text))
        s["adapters"][0][a] = text[:ADAPTER_MAX]
    for k in ("min_overlap", "error_num", "error_den", "pair_min_overlap", "pair_error_num", "pair_error_den", "pair_max_diff", "poly_before", "poly_after",
              "poly_min_len", "poly_per", "poly_max_mismatch", "reserved", "min_len"):
        s[k] = r[k]
    return s


def rule_words(r):
    return rule_struct(r).view(np.uint32).reshape(-1).copy()


# ---------------------------------------------------------------------------------------------------------------- the steps

def poly_model(c, b, e, mask, r):
    """steps 1 and 4 on [b, e) of the codes c: the new e"""
    best = e
    n_span = e - b
    if n_span <= 0:
        return e
    t = np.arange(1, n_span + 1)
    for X in range(4):
        if not (mask >> X) & 1:
            continue
        tail = c[b:e][::-1]                       # tail[t - 1] is the t-th base from the 3' end
        x = np.cumsum(tail != X)
        allowed = t // r["poly_per"] if r["poly_per"] else np.zeros(n_span, np.int64)
        stop = (x > r["poly_max_mismatch"]) | ((t >= r["poly_min_len"]) & (x > allowed))
        hit = np.nonzero(stop)[0]
        n = int(hit[0]) if len(hit) else n_span   # (the stop at t leaves t - 1 bases walked)
        if n < r["poly_min_len"]:
            continue
        at = np.nonzero(c[e - n:e] == X)[0]
        if len(at) and e - n + int(at[0]) < best:
            best = e - n + int(at[0])
    return best


def pair_model(c1, c2, r):
    """step 2 on whole mates: (insert or 0, d(insert), skipped)"""
    M = min(len(c1), len(c2))
    if M > PAIR_MAX:
        return 0, 0, True
    for I in range(M, r["pair_min_overlap"] - 1, -1):
        if I < 1:
            break
        a, m = c1[:I], c2[:I][::-1]
        d = int(((a > 3) | (m > 3) | (a != 3 - m)).sum())
        if d <= min(r["pair_max_diff"], I * r["pair_error_num"] // r["pair_error_den"]):
            return I, d, False
    return 0, 0, False


def adapter_model(c, b, e, r):
    """step 3 on [b, e): (adapter, p, overlap, mismatches) or None"""
    best = None
    n = e - b
    for a, text in enumerate(r["adapters"]):
        ac = codes(text)
        A = len(ac)
        O = min(r["min_overlap"], A)
        if n < O:
            continue
        padded = np.concatenate([c[b:e], np.full(A, 5, np.int64)])   # 5: behind the span, outside every overlap
        win = np.lib.stride_tricks.sliding_window_view(padded, A)[:n - O + 1]
        m = ((win != ac) & (win != 5)).sum(axis=1)
        o = np.minimum(A, n - np.arange(n - O + 1))
        ok = m <= o * r["error_num"] // r["error_den"]
        if not ok.any():
            continue
        score = np.where(ok, o - m, -1)
        at = int(np.argmax(score))                                     # the first of the best: the smaller p
        cand = (int(score[at]), -(b + at), -a)
        if best is None or cand > best[0]:
            best = (cand, (a, b + at, int(o[at]), int(m[at])))
    return None if best is None else best[1]


def clamp_span(span, L):
    if span is None:
        b, e = 0, L
    else:
        b, e = min(int(span[0]), L), min(int(span[1]), L)
    return (0, 0) if e <= b else (b, e)


def read_model(c, span, r, pair):
    """c: the read's codes; pair: step 2's (insert, d, skipped) or None.  The fields of bl_read_adapters and the span that goes out."""
    L = len(c)
    rec = dict(begin=0, end=0, match_pos=U32, insert=0, adapter=0xFFFF, overlap=0, mismatches=0, pair_mismatches=0, cut=0)
    b, e = clamp_span(span, L)
    if e <= b:
        return rec, (0, 0)
    if r["poly_before"]:
        e2 = poly_model(c, b, e, r["poly_before"], r)
        if e2 < e:
            rec["cut"] |= CUT["poly_before"]
        e = e2
    if pair is not None:
        I, d, skipped = pair
        if skipped:
            rec["cut"] |= CUT["pair_skipped"]
        elif I:
            rec["insert"], rec["pair_mismatches"] = I, d
            e2 = max(b, min(e, I))
            if e2 < e:
                rec["cut"] |= CUT["pair"]
            e = e2
    if r["adapters"]:
        hit = adapter_model(c, b, e, r)
        if hit is not None:
            rec["adapter"], rec["match_pos"], rec["overlap"], rec["mismatches"] = hit
            rec["cut"] |= CUT["adapter"]
            e = hit[1]
    if r["poly_after"]:
        e2 = poly_model(c, b, e, r["poly_after"], r)
        if e2 < e:
            rec["cut"] |= CUT["poly_after"]
        e = e2
    rec["begin"], rec["end"] = b, e
    n = e - b
    if n < r["min_len"]:
        rec["cut"] |= CUT["too_short"]
    return rec, ((b, e) if n >= r["min_len"] and n > 0 else (0, 0))


def batch_model(reads, r, spans_in=None, step=read_model, pair_step=pair_model):
    """reads: [bytes] -> (records, spans, stats).  step / pair_step: test_adapter_model.py passes its restatements"""
    n = len(reads)
    recs = np.zeros(n, RECORD)
    spans = np.zeros((n, 2), np.uint64)
    st = dict.fromkeys(STATS, 0)
    st["per_adapter"] = [0] * MAX_ADAPTERS
    cs = [codes(x) for x in reads]
    paired = bool(r["flags"] & PAIRED)
    assert not paired or n % 2 == 0
    for i in range(n):
        pair = None
        if paired:
            pair = pair_step(cs[i & ~1], cs[i | 1], r)
        m, span = step(cs[i], None if spans_in is None else spans_in[i], r, pair)
        for k, x in m.items():
            recs[i][k] = x
        spans[i] = span
        kept = span[1] > 0
        st["n_reads"] += 1
        st["n_reads_cut"] += bool(m["cut"] & 15)
        st["n_reads_kept"] += kept
        st["n_bases"] += len(reads[i])
        st["n_bases_kept"] += span[1] - span[0]
        for bit, name in enumerate(("n_poly_before", "n_pair", "n_adapter", "n_poly_after", "n_too_short", "n_pair_skipped")):
            st[name] += (m["cut"] >> bit) & 1
        if m["adapter"] != 0xFFFF:
            st["per_adapter"][m["adapter"]] += 1
    return recs, spans, {k: ([int(y) for y in x] if isinstance(x, list) else int(x)) for k, x in st.items()}


def apply_spans(reads, spans):
    return [bytes(x[int(b):int(e)]) for x, (b, e) in zip(reads, spans)]


def layout(reads):
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    return dict(bases=b"".join(reads), offsets=offsets)


# ---------------------------------------------------------------------------------------------------------------- the named cases

COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(x):
    return bytes(x).translate(COMPLEMENT)[::-1]


def dna(n, seed, letters=b"ACGT"):
    return np.random.default_rng(5000 + seed).choice(np.frombuffer(letters, np.uint8), n).tobytes()


def planted(L, adapter, p, seed, changed=(), body=b"ACT"):
    """a read of L bases over `body`'s letters with `adapter` written at p (cut by the read's end), its bases `changed` replaced by a
    base that differs"""
    x = bytearray(dna(L, seed, body))
    a = bytearray(adapter)
    for j in changed:
        a[j] = ord("A") if a[j] in b"CcGg" else ord("C")
    x[p:p + len(a)] = a[:max(0, L - p)]
    assert len(x) == L
    return bytes(x)


# the lengths the issue names, with O = 3: a chunk holds 16 bases, a window 32, an adapter 64 at most, step 2 512, a block 1,024
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, 255, 256, 257, 512, 513, 1024, 1025, 5000)
ADAPTER_LENGTHS = (1, 13, 31, 32, 33, 63, 64)


def lengths_case():
    reads = []
    for k, L in enumerate(LENGTHS):
        reads.append(dna(L, k))                                         # whatever chance plants
        if L >= 3:
            reads.append(planted(L, TRUSEQ, L - 3, 100 + k))            # cut by the end at the overlap O
            reads.append(planted(L, TRUSEQ, L - 2, 200 + k))            # and at O - 1: no candidate
            reads.append(planted(L, TRUSEQ, 0, 300 + k))                # at p = 0: an empty result
        if L >= 32:
            reads.append(planted(L, TRUSEQ, L // 2, 400 + k))
            reads.append(planted(L, TRUSEQ, L - 7, 500 + k, changed=(1,)))   # floor(7 / 10) = 0: no candidate at 7, a shorter clean overlap may be
        if L >= 1024:
            for p in (1010, 1011, 1023, 1024):                           # across the block's end
                if p < L:
                    reads.append(planted(L, TRUSEQ, p, 600 + k + p))
    return reads, rule(adapters=[TRUSEQ]), None


def adapter_length_case(A):
    ad = dna(A, 900 + A, b"ACGT")
    allowed = A // 10
    reads = []
    for L in (150, 1100):
        for p in (0, 40, L - A, L - 3, L - 2) + ((1000, 1023 - A // 2, 1024) if L > 1024 else ()):
            if p < 0:
                continue
            reads.append(planted(L, ad, p, len(reads) + A))
        p = 40
        reads.append(planted(L, ad, p, len(reads), changed=range(allowed)))           # mismatches exactly at the floor
        reads.append(planted(L, ad, p, len(reads), changed=range(allowed + 1)))       # and one above
        reads.append(planted(L, ad, p, len(reads), changed=range(A - allowed, A)))    # at the adapter's other end
        x = bytearray(planted(L, ad, p, len(reads)))
        x[p + A // 2] = ord("N")                                                      # an invalid base inside the match
        reads.append(bytes(x))
        x = bytearray(planted(L, ad, p, len(reads)))
        x[p - 1] = ord("N")                                                           # and just outside it, on either side
        x[p + A] = ord("n")
        reads.append(bytes(x))
    return reads, rule(adapters=[ad]), None


def eight_case():
    rnd = [dna(n, 40 + n) for n in (20, 33, 64, 17)]
    ads = [TRUSEQ, ADAPTERS["nextera"], ADAPTERS["small_rna"], rnd[0], rnd[1], rnd[2], ADAPTERS["nextera"][:12], rnd[3]]
    reads = []
    for a, ad in enumerate(ads):
        for L in (150, 300, 1030):
            reads.append(planted(L, ad, L // 3, 10 * a + L))
            reads.append(planted(L, ad, L - len(ad) // 2 - 2, 11 * a + L, body=b"AC"))
    # equal matches for two adapters: Nextera cut by the end at 12 bases is adapter 6 as well; the lower index wins
    reads.append(planted(150, ads[1], 138, 77, body=b"A"))
    # equal matches at two positions: the adapter twice, whole; the smaller p wins
    x = bytearray(dna(150, 78, b"AC"))
    x[30:43] = TRUSEQ
    x[90:103] = TRUSEQ
    reads.append(bytes(x))
    # a later position with more matches wins over an earlier one with fewer
    x = bytearray(dna(150, 79, b"AC"))
    x[20:33] = planted(13, TRUSEQ, 0, 0, changed=(5,))
    x[100:113] = TRUSEQ
    reads.append(bytes(x))
    # lowercase and U
    reads.append(dna(40, 80, b"AC") + TRUSEQ.lower().replace(b"t", b"u") + dna(30, 81, b"AC"))
    return reads, rule(adapters=ads, min_overlap=5), None


def mates(I, L1, L2, seed, errors=0, tail=TRUSEQ, n_at=None):
    """mates of an insert of I bases: each reads min(L, I) of it, then runs into `tail` and random bases"""
    ins = dna(I, seed)
    r1 = bytearray((ins + tail + dna(L1, seed + 1))[:L1])
    r2 = bytearray((revcomp(ins) + tail + dna(L2, seed + 2))[:L2])
    for j in range(errors):
        at = 3 + 5 * j
        r1[at] = ord("A") if r1[at] != ord("A") else ord("C")
    if n_at is not None:
        r1[n_at] = ord("N")
    return bytes(r1), bytes(r2)


def pair_case():
    reads = []
    add = lambda pair: reads.extend(pair)
    add(mates(80, 150, 100, 1))                 # L1 != L2
    add(mates(80, 100, 150, 2))
    add(mates(30, 150, 150, 3))                 # I = pair_min_overlap
    add(mates(29, 150, 150, 4))                 # one below: step 3 alone finds the adapter
    add(mates(150, 150, 150, 5))                # I = min(L1, L2) with equal lengths: an insert, no cut
    add(mates(120, 150, 120, 6))                # I = min(L1, L2) with L1 > L2: only the longer mate is cut
    add(mates(400, 150, 150, 7))                # no read-through
    add(mates(148, 150, 150, 8))                # two bases of adapter: below step 3's overlap, step 2 decides
    add(mates(149, 150, 150, 9, tail=b"GGGGG"))
    add(mates(100, 150, 150, 10, errors=5))     # d exactly pair_max_diff
    add(mates(100, 150, 150, 11, errors=6))     # and one above: step 3 decides
    add(mates(40, 150, 150, 12, errors=8))      # floor(40 / 5) = 8 > pair_max_diff
    add(mates(35, 150, 150, 13, errors=5))      # floor(35 / 5) = 7
    add(mates(100, 150, 150, 14, n_at=50))      # an invalid base in the overlap counts
    add(mates(100, 150, 150, 15, errors=5, n_at=50))
    add((dna(150, 16), dna(150, 17)))           # unrelated mates
    add((planted(150, TRUSEQ, 90, 18), dna(150, 19)))   # step 3 decides the first mate, step 2 leaves the pair alone
    add((b"", dna(150, 20)))
    add((dna(20, 21), revcomp(dna(20, 21))))    # shorter than pair_min_overlap
    add(mates(300, 512, 512, 22))               # the longest pair that is tested
    add(mates(512, 512, 512, 23))
    add(mates(300, 513, 513, 24))               # skipped
    add(mates(300, 513, 400, 25))               # min(L1, L2) = 400: tested
    add(mates(300, 2000, 512, 26))
    add(mates(60, 64, 63, 27))
    add(mates(33, 33, 47, 28))
    return reads, rule(flags=PAIRED, adapters=[TRUSEQ]), None


def poly_reads():
    reads = []
    body = lambda n, k: dna(n, 700 + k, b"ACT")
    for n in (8, 9, 10, 11, 12, 40):                        # tails around poly_min_len (10, and 12 without mismatches); 9 with one mismatch is a tail of 10
        reads.append(body(100, n) + b"G" * n)
    for k in range(20):                                     # one mismatch at every place of a tail of 20
        t = bytearray(b"G" * 20)
        t[19 - k] = ord("A")
        reads.append(body(100, 20 + k) + bytes(t))
    for k in (1, 7, 8, 9, 15, 16, 17):                      # two mismatches: the second is allowed from t = 16 on
        t = bytearray(b"G" * 30)
        t[29] = ord("T")
        t[29 - k] = ord("C")
        reads.append(body(60, 50 + k) + bytes(t))
    t = bytearray(b"G" * 60)                                # six mismatches: one above poly_max_mismatch
    for k in (8, 16, 24, 32, 40, 48):
        t[59 - k] = ord("A")
    reads.append(body(50, 60) + bytes(t))
    for L in (1, 9, 10, 64, 65, 150, 1024, 1025, 5000):     # all-G reads
        reads.append(b"G" * L)
    reads.append(b"g" * 70 + b"N" + b"G" * 30)              # an invalid base is a mismatch
    reads.append(body(1000, 61) + b"G" * 100)               # a tail across the block's end
    reads.append(body(990, 62) + b"G" * 34 + b"A" + b"G" * 40)
    reads.append(body(100, 63) + b"A" * 12)                 # other bases
    reads.append(body(100, 64) + b"T" * 12 + b"G" * 3)
    reads.append(body(100, 65) + b"C" * 15)
    reads.append(body(100, 66) + b"GA" * 10)                # both A and G propose
    reads.append(body(100, 67) + b"G" * 12 + TRUSEQ + body(20, 68))   # poly G in front of the adapter: step 4's
    reads.append(body(100, 69) + b"G" * 12 + TRUSEQ[:6])
    reads.append(body(30, 70))
    return reads


def spans_case():
    reads, _, _ = lengths_case()
    reads = reads + poly_reads()[:30]
    rng = np.random.default_rng(31)
    spans = np.zeros((len(reads), 2), np.uint64)
    for i, x in enumerate(reads):
        L = len(x)
        kind = i % 6
        if kind == 0:
            spans[i] = (0, U64)
        elif kind == 1:
            spans[i] = (min(5, L), max(L, 7) - 7)            # both ends cut; empty for short reads
        elif kind == 2:
            spans[i] = sorted(rng.integers(0, L + 1, 2))
        elif kind == 3:
            spans[i] = (rng.integers(0, L + 10), rng.integers(0, L + 10))   # anything, b > e included
        elif kind == 4:
            spans[i] = (L, L + 3)                            # empty after the clamp
        else:
            spans[i] = (L // 4, L - L // 4)
    return reads, rule(adapters=[TRUSEQ], poly_before=poly_mask(b"G"), poly_after=poly_mask(b"G"), min_len=20), spans


def cases():
    out = {"lengths": lengths_case(), "eight": eight_case(), "pair": pair_case(), "spans_in": spans_case()}
    for A in ADAPTER_LENGTHS:
        out["adapter%d" % A] = adapter_length_case(A)
    pr = poly_reads()
    out["poly_before"] = (pr, rule(poly_before=poly_mask(b"G")), None)
    out["poly_after"] = (pr, rule(adapters=[TRUSEQ], poly_after=poly_mask(b"G")), None)
    out["poly_exact"] = (pr, rule(poly_before=poly_mask(b"G"), poly_per=0, poly_min_len=12), None)
    out["poly_any"] = (pr, rule(poly_before=poly_mask(b"ACGT"), poly_after=poly_mask(b"AG"), adapters=[TRUSEQ], poly_per=1, poly_max_mismatch=2), None)
    out["poly_loose"] = (pr, rule(poly_before=poly_mask(b"G"), poly_min_len=1, poly_per=3, poly_max_mismatch=U32), None)
    reads, r, _ = pair_case()
    out["pair_only"] = (reads, rule(flags=PAIRED), None)
    out["pair_all_steps"] = (reads[:40] + pr[:40], rule(flags=PAIRED, adapters=[TRUSEQ, ADAPTERS["nextera"]], poly_before=poly_mask(b"G"),
                                                        poly_after=poly_mask(b"G"), min_len=31), None)
    out["pair_loose"] = (reads, rule(flags=PAIRED, pair_min_overlap=1, pair_error_num=1, pair_error_den=1, pair_max_diff=U32), None)
    out["error_all"] = (lengths_case()[0][:60], rule(adapters=[TRUSEQ], error_num=1, error_den=1, min_overlap=64), None)
    out["error_none"] = (lengths_case()[0], rule(adapters=[TRUSEQ, ADAPTERS["small_rna"]], error_num=0, error_den=1, min_overlap=1), None)
    return out
