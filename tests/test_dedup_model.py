"""CPU-only: the model of bl_scan_read_duplicates (dedup_cases.py) against a literal restatement of the header's text with plain loops
over letters (every unit compared with every earlier one), on every named case and on random reads under random rules; the invariants
of a result; and what the case set has to contain for the other two test files to mean something."""
import numpy as np
import pytest

import dedup_cases as DC

LETTER = {**{ch: "A" for ch in b"Aa"}, **{ch: "C" for ch in b"Cc"}, **{ch: "G" for ch in b"Gg"}, **{ch: "T" for ch in b"TtUu"}}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def restated(reads, r, spans_in=None, scores=None):
    """the header's rule, unit against unit"""
    paired, canonical, P = bool(r["flags"] & 1), bool(r["flags"] & 2), r["prefix_len"]
    per = 2 if paired else 1
    n_units = len(reads) // per
    key, span = [], []
    for i, x in enumerate(reads):
        L = len(x)
        b, e = (0, L) if spans_in is None else (min(int(spans_in[i][0]), L), min(int(spans_in[i][1]), L))
        if e <= b:
            b = e = 0
        span.append((b, e))
        s = "".join(LETTER.get(ch, "N") for ch in x[b:e])
        key.append(s[:P] if P else s)

    def unit(u):
        return [key[per * u + t] for t in range(per)]

    def equal(u, v):
        a, b = unit(u), unit(v)
        if a == b:
            return True
        if not canonical:
            return False
        if paired:
            return a == [b[1], b[0]]
        return a[0] == "".join(COMP[ch] for ch in reversed(b[0]))

    def score(u):
        total = 0
        for t in range(per):
            total = (total + (int(scores[per * u + t]) if scores is not None else 0)) % (1 << 64)
        return total

    records = np.zeros(n_units, DC.RECORD)
    out = np.zeros((len(reads), 2), np.uint64)
    first = {}
    for u in range(n_units):
        if any(k == "" for k in unit(u)):
            records[u] = (u, u, 0, DC.EMPTY)
            continue
        first[u] = u
        for v in range(u):
            if v in first and equal(u, v):
                first[u] = first[v]
                break
    for u, f in first.items():
        members = [v for v in first if first[v] == f]
        kept = members[0]
        for v in members:
            if score(v) > score(kept):
                kept = v
        records[u] = (f, kept, len(members), (DC.DUPLICATE if u != kept else 0) | (DC.REVERSED if unit(u) != unit(kept) else 0))
    for u in range(n_units):
        if not records[u]["flags"] & DC.DUPLICATE:
            for t in range(per):
                out[per * u + t] = span[per * u + t]
    return records, out


def invariants(records, spans, stats, per):
    n_units = len(records)
    for u, rec in enumerate(records):
        if rec["flags"] & DC.EMPTY:
            assert (rec["first"], rec["kept"], rec["copies"], rec["flags"]) == (u, u, 0, DC.EMPTY)
            continue
        members = np.nonzero((records["first"] == rec["first"]) & (records["flags"] & DC.EMPTY == 0))[0]
        assert rec["kept"] in members and rec["first"] == members[0] and rec["copies"] == len(members)
        assert bool(rec["flags"] & DC.DUPLICATE) == (u != rec["kept"])
        if rec["flags"] & DC.DUPLICATE:
            assert not spans[per * u:per * u + per].any()
    assert sum(stats["class_hist"]) == stats["n_classes"]
    assert stats["n_duplicates"] == n_units - stats["n_empty"] - stats["n_classes"]
    assert stats["n_units"] == n_units


@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_model_against_the_restatement(name):
    c = DC.cases()[name]
    records, spans, stats = DC.batch_model(c.reads, c.rule, c.spans_in, c.scores)
    w_records, w_spans = restated(c.reads, c.rule, c.spans_in, c.scores)
    assert np.array_equal(records, w_records) and np.array_equal(spans, w_spans)
    invariants(records, spans, stats, 2 if c.rule["flags"] & 1 else 1)


def test_random_reads_under_random_rules():
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"ACGTacgtUuNn.\0", np.uint8)
    done = 0
    while done < 2000:
        n = int(rng.integers(2, 40)) * 2
        flags = int(rng.integers(0, 4))
        pool = [rng.choice(alphabet[:int(rng.choice([2, 4, 14]))], int(rng.integers(0, 9))).tobytes() for _ in range(6)]
        reads = [pool[int(i)] for i in rng.integers(0, 6, n)]
        reads = [DC.revcomp(x) if rng.random() < 0.3 else x for x in reads]
        spans_in = rng.integers(0, 10, (n, 2)).astype(np.uint64) if rng.random() < 0.5 else None
        scores = [int(x) for x in rng.integers(0, 4, n)] if rng.random() < 0.5 else None
        if scores is not None and rng.random() < 0.3:
            scores[0] = DC.U64
        r = DC.rule(flags=flags, prefix_len=int(rng.choice([0, 0, 3, 5])))
        records, spans, stats = DC.batch_model(reads, r, spans_in, scores)
        w_records, w_spans = restated(reads, r, spans_in, scores)
        assert np.array_equal(records, w_records) and np.array_equal(spans, w_spans), (reads, r, spans_in, scores)
        invariants(records, spans, stats, 2 if flags & 1 else 1)
        done += n


def test_the_case_set_covers_what_the_other_files_rely_on():
    results = {name: DC.batch_model(c.reads, c.rule, c.spans_in, c.scores) for name, c in DC.cases().items()}
    flags = np.concatenate([r[0]["flags"] for r in results.values()])
    for bit in (DC.DUPLICATE, DC.EMPTY, DC.REVERSED):
        assert (flags & bit != 0).any() and (flags & bit == 0).any(), bit
    assert any((r[0]["kept"] != r[0]["first"]).any() for r in results.values()), "a later member wins somewhere"
    for name, bins in DC.HIST_CLAIMS.items():
        for k in bins:
            assert results[name][2]["class_hist"][k] > 0, (name, k)
    assert results["class_sizes"][2]["largest_class"] == 20 and results["class_sizes"][2]["class_hist"][15] == 2
    assert results["volume_fixed"][2]["n_classes"] >= 300 and results["volume_ragged"][2]["n_classes"] >= 300   # more classes than 2^8 groups
    starts = {int(x) % 32 for x in DC.layout(DC.cases()["residues"].reads)["offsets"][:-1]}
    assert starts == set(range(32))
    lengths = {len(x) for x in DC.cases()["lengths"].reads}
    assert {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, 1023, 1024, 1025, 5000} <= lengths
    # the minimal differences really are single differences, and the letters one class
    one = results["one_difference"][0]
    assert (one["copies"] == 2).all()
    letters = results["letters"][0]
    assert (letters["first"][[0, 1, 2, 3, 4, 5, 6, 7, 10]] == 0).all() and (letters["first"][[8, 9]] != 0).all()
    on, off = results["canonical_on"][0], results["canonical_off"][0]
    assert (on["flags"] & DC.REVERSED).any() and not (off["flags"] & DC.REVERSED).any() and results["canonical_on"][2]["n_classes"] < results["canonical_off"][2]["n_classes"]
    assert results["pairs_canonical"][2]["n_classes"] < results["pairs"][2]["n_classes"]
    assert any(len(c.reads) == 1002 for c in DC.cases().values())
