"""CPU-only: the numpy model of bl_scan_read_adapters (adapter_cases.py) against a literal restatement of the header's text with python
loops (the poly walk base by base, d(I) and the adapter's mismatches position by position), the model's invariants, and the condition on
the case set that keeps the emulation and the GPU tests from passing vacuously: every step moves an end somewhere, every bit of `cut` is
both set and clear, every tie rule decides a read, and steps 2 and 3 each decide a read the other leaves alone."""
import numpy as np
import pytest

import adapter_cases as AC


def poly_loops(c, b, e, mask, r):
    best = e
    for X in range(4):
        if not (mask >> X) & 1:
            continue
        x, n = 0, e - b
        for t in range(1, e - b + 1):
            if c[e - t] != X:
                x += 1
            if x > r["poly_max_mismatch"] or (t >= r["poly_min_len"] and x > (t // r["poly_per"] if r["poly_per"] else 0)):
                n = t - 1
                break
        if n >= r["poly_min_len"]:
            for pos in range(e - n, e):
                if c[pos] == X:
                    if pos < best:
                        best = pos
                    break
    return best


def pair_loops(c1, c2, r):
    M = min(len(c1), len(c2))
    if M > 512:
        return 0, 0, True
    found = (0, 0, False)
    for I in range(max(r["pair_min_overlap"], 1), M + 1):
        d = 0
        for i in range(I):
            x, y = c1[i], c2[I - 1 - i]
            if x > 3 or y > 3 or x != 3 - y:
                d += 1
        if d <= r["pair_max_diff"] and d <= I * r["pair_error_num"] // r["pair_error_den"]:
            found = (I, d, False)   # the largest stays
    return found


def adapter_loops(c, b, e, r):
    best, best_key = None, None
    for a, text in enumerate(r["adapters"]):
        ac = [int(x) for x in AC.codes(text)]
        A = len(ac)
        O = min(r["min_overlap"], A)
        for p in range(b, e - O + 1):
            o = min(A, e - p)
            m = sum(1 for j in range(o) if c[p + j] != ac[j])   # (an invalid base is code 4: it differs from every adapter base)
            if m <= o * r["error_num"] // r["error_den"]:
                key = (o - m, -p, -a)
                if best_key is None or key > best_key:
                    best_key, best = key, (a, p, o, m)
    return best


def read_loops(c, span, r, pair):
    c = [int(x) for x in c]
    L = len(c)
    rec = dict(begin=0, end=0, match_pos=AC.U32, insert=0, adapter=0xFFFF, overlap=0, mismatches=0, pair_mismatches=0, cut=0)
    b, e = (0, L) if span is None else (min(int(span[0]), L), min(int(span[1]), L))
    if e <= b:
        return rec, (0, 0)
    if r["poly_before"]:
        e2 = poly_loops(c, b, e, r["poly_before"], r)
        rec["cut"] |= 1 if e2 < e else 0
        e = e2
    if pair is not None:
        I, d, skipped = pair
        if skipped:
            rec["cut"] |= 32
        elif I:
            rec["insert"], rec["pair_mismatches"] = I, d
            if I < e:
                rec["cut"] |= 2 if max(I, b) < e else 0
                e = max(I, b)
    hit = adapter_loops(c, b, e, r)
    if hit:
        rec["adapter"], rec["match_pos"], rec["overlap"], rec["mismatches"] = hit
        rec["cut"] |= 4
        e = hit[1]
    if r["poly_after"]:
        e2 = poly_loops(c, b, e, r["poly_after"], r)
        rec["cut"] |= 8 if e2 < e else 0
        e = e2
    rec["begin"], rec["end"] = b, e
    if e - b < r["min_len"]:
        rec["cut"] |= 16
    return rec, ((b, e) if e - b >= r["min_len"] and e > b else (0, 0))


def same_models(reads, r, spans_in, tag):
    got = AC.batch_model(reads, r, spans_in)
    want = AC.batch_model(reads, r, spans_in, step=read_loops, pair_step=pair_loops)
    bad = np.nonzero(got[0] != want[0])[0]
    assert len(bad) == 0, (tag, [(int(i), reads[i][-40:], got[0][i], want[0][i]) for i in bad[:3]])
    assert np.array_equal(got[1], want[1]) and got[2] == want[2], tag
    return got


@pytest.fixture(scope="module")
def results():
    """the model's answer to every named case, computed once"""
    return {name: AC.batch_model(reads, r, spans) for name, (reads, r, spans) in AC.cases().items()}


@pytest.mark.parametrize("name", sorted(AC.cases()))
def test_model_against_loops(name):
    reads, r, spans = AC.cases()[name]
    if name in ("pair_loose",):
        reads = [x for pair in zip(reads[0::2], reads[1::2]) if max(len(pair[0]), len(pair[1])) <= 600 for x in pair]   # (d(I) by loops is cubic)
    same_models(reads, r, spans, name)


def test_random_reads_and_rules():
    """3,000 seeded random reads under random rules: short alphabets and planted adapters, tails and mates make every step fire"""
    rng = np.random.default_rng(2024)
    n_reads, cuts = 0, 0
    while n_reads < 3000:
        ads = [AC.dna(int(rng.integers(1, 20)), int(rng.integers(0, 1 << 30)), b"ACGT" if rng.random() < 0.7 else b"AC") for _ in range(int(rng.integers(0, 4)))]
        den = int(rng.integers(1, 12))
        pden = int(rng.integers(1, 8))
        r = AC.rule(flags=int(rng.integers(0, 2)), adapters=ads, min_overlap=int(rng.integers(1, 8)), error_num=int(rng.integers(0, den + 1)) if rng.random() < 0.3 else min(1, den),
                    error_den=den, pair_min_overlap=int(rng.integers(1, 40)), pair_error_num=int(rng.integers(0, pden + 1)), pair_error_den=pden,
                    pair_max_diff=int(rng.integers(0, 8)), poly_before=int(rng.integers(0, 16)) if rng.random() < 0.5 else 0,
                    poly_after=int(rng.integers(0, 16)) if rng.random() < 0.5 else 0, poly_min_len=int(rng.integers(1, 14)), poly_per=int(rng.integers(0, 10)),
                    poly_max_mismatch=int(rng.integers(0, 7)), min_len=int(rng.integers(0, 30)))
        reads = []
        for _ in range(10):
            L = int(rng.integers(0, 90))
            letters = (b"ACGT", b"ACGTN", b"AG", b"G")[int(rng.integers(0, 4))]
            x = bytearray(AC.dna(L, int(rng.integers(0, 1 << 30)), letters))
            if ads and L and rng.random() < 0.6:
                ad = ads[int(rng.integers(0, len(ads)))]
                p = int(rng.integers(0, L))
                x[p:p + len(ad)] = ad[:L - p]
            if L and rng.random() < 0.4:
                t = int(rng.integers(1, 25))
                x[max(0, L - t):] = b"GA"[int(rng.integers(0, 2))::2] * min(t, L)
            mate = bytearray(AC.revcomp(x[:int(rng.integers(0, L + 1))]) + AC.dna(int(rng.integers(0, 30)), int(rng.integers(0, 1 << 30))))
            for at in rng.integers(0, max(len(mate), 1), int(rng.integers(0, 3))):
                if len(mate):
                    mate[at] = ord("A")
            reads += [bytes(x), bytes(mate)]
        spans = None
        if rng.random() < 0.5:
            spans = np.array([(rng.integers(0, len(x) + 5), rng.integers(0, len(x) + 5)) for x in reads], np.uint64)
        got = same_models(reads, r, spans, n_reads)
        n_reads += len(reads)
        cuts += got[2]["n_reads_cut"]
    assert cuts > 500


def test_invariants(results):
    for name, (reads, r, spans_in) in AC.cases().items():
        recs, spans, stats = results[name]
        for i, x in enumerate(reads):
            L = len(x)
            b, e = AC.clamp_span(None if spans_in is None else spans_in[i], L)
            rec = recs[i]
            assert b <= rec["begin"] <= rec["end"] <= e <= L or (e == 0 and rec["end"] == 0), (name, i)
            if rec["adapter"] != 0xFFFF:
                assert rec["match_pos"] + rec["overlap"] <= e and rec["end"] <= rec["match_pos"] and rec["cut"] & 4, (name, i)
                assert rec["overlap"] - rec["mismatches"] >= 0 and rec["adapter"] < len(r["adapters"])
            else:
                assert rec["match_pos"] == AC.U32 and rec["overlap"] == 0 and not rec["cut"] & 4
            assert tuple(spans[i]) in ((0, 0), (rec["begin"], rec["end"]))
            assert (tuple(spans[i]) == (0, 0)) == (rec["end"] - rec["begin"] < max(r["min_len"], 1))
        assert stats["n_reads"] == len(reads) and stats["n_bases"] == sum(map(len, reads))
        assert stats["n_bases_kept"] == int((spans[:, 1] - spans[:, 0]).sum()) and sum(stats["per_adapter"]) == stats["n_adapter"]


def test_the_case_set_exercises_everything(results):
    cs = AC.cases()
    seen_set, seen_clear = 0, 0
    for name, (recs, _, _) in results.items():
        for cut in recs["cut"]:
            seen_set |= int(cut)
            seen_clear |= ~int(cut) & 63
    assert seen_set == 63 and seen_clear == 63, "every bit of cut is both set and clear (the four step bits: every step moves an end)"
    for name in ("poly_before", "poly_after", "pair_only", "lengths"):
        bit = dict(poly_before=1, poly_after=8, pair_only=2, lengths=4)[name]
        assert (results[name][0]["cut"] & bit).any(), name
    # the tie rules of step 3, each deciding a read: the same number of matching bases at two positions, and for two adapters
    reads, r, _ = cs["eight"]
    two_positions = two_adapters = later_wins = 0
    for i, x in enumerate(reads):
        c = [int(v) for v in AC.codes(x)]
        rec = results["eight"][0][i]
        if rec["adapter"] == 0xFFFF:
            continue
        best = int(rec["overlap"]) - int(rec["mismatches"])
        for a, text in enumerate(r["adapters"]):
            ac = [int(v) for v in AC.codes(text)]
            for p in range(0, len(c) - min(r["min_overlap"], len(ac)) + 1):
                o = min(len(ac), len(c) - p)
                m = sum(1 for j in range(o) if c[p + j] != ac[j])
                if m <= o * r["error_num"] // r["error_den"] and o - m == best:
                    two_positions += a == rec["adapter"] and p > rec["match_pos"]
                    two_adapters += a > rec["adapter"] and p == rec["match_pos"]
                if m <= o * r["error_num"] // r["error_den"] and o - m < best and p < rec["match_pos"]:
                    later_wins += 1
    assert two_positions and two_adapters and later_wins
    # steps 2 and 3 each decide a read that the other leaves alone
    reads, r, _ = cs["pair"]
    recs = results["pair"][0]
    only2 = (recs["cut"] & 6) == 2
    only3 = ((recs["cut"] & 6) == 4) & (recs["insert"] == 0)
    assert only2.any() and only3.any()
    without3 = AC.batch_model(reads, dict(r, adapters=[]))[0]
    without2 = AC.batch_model(reads, dict(r, flags=0))[0]
    assert (without3["end"][only2] == recs["end"][only2]).all() and (without2["end"][only2] > recs["end"][only2]).any()
    assert (without2["end"][only3] == recs["end"][only3]).all() and (without3["end"][only3] > recs["end"][only3]).any()
    # an insert without a cut (I = min(L1, L2), equal lengths), a mate cut alone (L1 != L2), the skipped pair beside the longest tested one
    assert ((recs["insert"] == 150) & (recs["cut"] & 2 == 0)).any()
    assert any((recs["cut"][i] ^ recs["cut"][i + 1]) & 2 for i in range(0, len(reads), 2))
    lens = np.array([len(x) for x in reads])
    assert ((lens == 512) & (recs["insert"] > 0)).any() and ((lens == 513) & (recs["cut"] & 32 != 0)).any()
    assert ((recs["insert"] == r["pair_min_overlap"])).any() and (recs["pair_mismatches"] == r["pair_max_diff"]).any()
    # poly tails of exactly poly_min_len and one less
    reads, r, _ = cs["poly_before"]
    recs = results["poly_before"][0]
    assert recs["end"][0] == len(reads[0]) and recs["end"][1] == len(reads[1]) - 9 and recs["end"][2] == len(reads[2]) - 10   # 8; 9 and a mismatch; 10
    recs = results["poly_exact"][0]
    assert recs["end"][3] == len(reads[3]) and recs["end"][4] == len(reads[4]) - 12   # without mismatches: 11 stays, 12 goes
    # input spans that cut both ends, are empty, and are garbage
    reads, r, spans_in = cs["spans_in"]
    recs = results["spans_in"][0]
    assert ((recs["begin"] > 0) & (recs["end"] > recs["begin"]) & (recs["cut"] & 15 != 0)).any()
    assert (spans_in[:, 0] > spans_in[:, 1]).any()
    # the lengths and adapter lengths the kernel's forms turn on
    assert {len(x) for x in cs["lengths"][0]} >= set(AC.LENGTHS)
    assert {len(cs["adapter%d" % A][1]["adapters"][0]) for A in AC.ADAPTER_LENGTHS} == {1, 13, 31, 32, 33, 63, 64}
    for A in AC.ADAPTER_LENGTHS:
        recs = results["adapter%d" % A][0]
        assert (recs["overlap"] == A).any() and (recs["adapter"] == 0xFFFF).any() == (A > 1), A
        if A > 1:   # (an adapter of one base matches at the first place that holds it)
            assert (recs["match_pos"] == 0).any() and (recs["match_pos"] == 40).any() and (recs["mismatches"] == A // 10).any() and (recs["overlap"] == 3).any(), A
