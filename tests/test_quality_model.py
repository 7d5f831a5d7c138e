"""CPU-only: the numpy model of bl_scan_read_quality (quality_cases.py) against a literal restatement of the header's text with python
loops (step B is the sequential walk), the 94 BL_PHRED_ERR literals of bl_quality_core.hpp against decimal arithmetic, the model's
invariants, and the condition on the case set that keeps the emulation and the GPU tests from passing vacuously: every step changes a
span somewhere and every filter bit is both set and clear somewhere."""
import os
import re

import numpy as np
import pytest

import quality_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loops_model(qual, bases, r):
    """the header's text, value by value"""
    v = [min(max(q - r["phred_base"], 0), 93) for q in qual]
    L = len(v)
    b, e = 0, L
    if r["front_q"]:
        while b < e and v[b] < r["front_q"]:
            b += 1
    if r["back_q"]:
        while e > b and v[e - 1] < r["back_q"]:
            e -= 1
    b2, e2 = b, e
    if r["maxsum_back_q"]:
        s, best = 0, 0
        for i in range(e - 1, b - 1, -1):
            s += r["maxsum_back_q"] - v[i]
            if s < 0:
                break
            if s > best:
                best, e2 = s, i
    if r["maxsum_front_q"]:
        s, best = 0, 0
        for i in range(b, e):
            s += r["maxsum_front_q"] - v[i]
            if s < 0:
                break
            if s > best:
                best, b2 = s, i + 1
    b, e = b2, max(b2, e2)
    W = r["window_len"]
    if W:
        for j in range(b, e - W + 1):
            if sum(v[j:j + W]) < W * r["window_q"]:
                e = j
                while e > b and v[e - 1] < r["window_q"]:
                    e -= 1
                break
    n = e - b
    rec = dict(begin=b, end=e, sum=0, ee=0, n_low=0, n_ambiguous=0, q_min=255, q_max=0)
    for j in range(b, e):
        rec["sum"] += v[j]
        rec["ee"] += int(QC.PHRED_ERR[v[j]])
        rec["n_low"] += v[j] < r["low_q"]
        rec["n_ambiguous"] += bases[j] not in b"ACGTUacgtu"
        rec["q_min"] = min(rec["q_min"], v[j])
        rec["q_max"] = max(rec["q_max"], v[j])
    f = 0
    f |= 1 if n < r["min_len"] else 0
    f |= 2 if r["max_len"] != 0 and n > r["max_len"] else 0
    f |= 4 if rec["n_ambiguous"] > r["max_ambiguous"] else 0
    f |= 8 if rec["n_low"] * r["low_max_den"] > n * r["low_max_num"] else 0
    f |= 16 if rec["sum"] < r["mean_q"] * n else 0
    f |= 32 if rec["ee"] > r["max_ee"] else 0
    rec["failed"] = f
    return rec


@pytest.fixture(scope="module")
def reads():
    return QC.reads()


@pytest.mark.parametrize("name", sorted(QC.rules()))
def test_model_equals_the_loops(reads, name):
    r = QC.rules()[name]
    for rname, bases, qual in reads:
        assert QC.read_model(qual, bases, r) == loops_model(qual, bases, r), (name, rname)
        if r["phred_base"] == 33 and len(qual) <= 300:  # the other base, and a FASTA index's fill
            r64 = dict(r, phred_base=64)
            assert QC.read_model(qual, bases, r64) == loops_model(qual, bases, r64), (name, rname, 64)
            assert QC.read_model(None, bases, r) == loops_model(bytes([r["quality_fill"]]) * len(bases), bases, r), (name, rname, "fill")


def test_closed_form_of_step_b_on_random_reads():
    rng = np.random.default_rng(5)
    for _ in range(3000):
        L = int(rng.integers(0, 40))
        qual = (rng.integers(0, 42, L) + 33).astype(np.uint8).tobytes()
        r = QC.rule(front_q=int(rng.integers(0, 30)), back_q=int(rng.integers(0, 30)), maxsum_front_q=int(rng.integers(0, 40)),
                    maxsum_back_q=int(rng.integers(0, 40)), window_len=int(rng.integers(0, 8)), window_q=int(rng.integers(0, 40)))
        assert QC.read_model(qual, b"A" * L, r) == loops_model(qual, b"A" * L, r), (qual, r)


def test_header_literals():
    src = open(os.path.join(ROOT, "biolib_amd", "csrc", "bl_quality_core.hpp")).read()
    body = re.search(r"BL_PHRED_ERR\[94\] = \{(.*?)\};", src, re.S).group(1)
    literals = [int(x) for x in re.findall(r"(\d+)u", body)]
    assert len(literals) == 94
    assert literals == [int(x) for x in QC.phred_err()]
    assert literals[0] == 1 << 31 and literals[10] == 214748365 and literals[93] == 1


def test_ambiguous_rule_is_the_encoders():
    """bl_scan_core.hpp's encode4 over all 256 byte values: valid iff the byte, lowercased, is the letter its code stands for ('u' for 't')"""
    for c in range(256):
        x = (c >> 1) & 3
        x ^= x >> 1
        diff = ((c | 0x20) ^ b"acgt"[x]) & ~(1 if x == 3 else 0) & 0xff
        assert (diff == 0) == bool(QC.VALID_BASE[c]), c


def test_invariants(reads):
    neutral = QC.rule()
    for name, r in QC.rules().items():
        for rname, bases, qual in reads:
            m = QC.read_model(qual, bases, r)
            L = len(bases)
            assert 0 <= m["begin"] <= m["end"] <= L, (name, rname)
            v = QC.phred_values(np.frombuffer(qual, np.uint8), r)[m["begin"]:m["end"]]
            assert m["sum"] == int(v.sum()) and m["n_low"] == int((v < r["low_q"]).sum()) and m["ee"] == sum(int(QC.PHRED_ERR[x]) for x in v)
            assert (m["q_min"], m["q_max"]) == ((int(v.min()), int(v.max())) if len(v) else (255, 0))
    for rname, bases, qual in reads:
        m = QC.read_model(qual, bases, neutral)
        assert (m["begin"], m["end"], m["failed"]) == (0, len(bases), 0), rname
        # steps that are off change nothing: thresholds of steps whose switch is 0
        off = QC.rule(window_len=0, window_q=40)
        assert QC.read_model(qual, bases, off) == m, rname


def test_the_case_set_exercises_every_step_and_filter(reads):
    changed = dict.fromkeys(("A front", "A back", "B front", "B back", "C cut", "C trailing walk"), 0)
    set_, clear = dict.fromkeys(QC.FAIL, 0), dict.fromkeys(QC.FAIL, 0)
    for name, r in QC.rules().items():
        for rname, bases, qual in reads:
            v = QC.phred_values(np.frombuffer(qual, np.uint8), r)
            s = QC.trim_steps(v, r)
            changed["A front"] += s[1] != s[0]
            changed["A back"] += s[2] != s[1]
            changed["B front"] += s[3][0] != s[2][0]
            changed["B back"] += s[3][1] != s[2][1] and s[3][1] > s[3][0]
            changed["C cut"] += s[4] != s[3]
            changed["C trailing walk"] += s[5] != s[4]
            f = QC.read_model(qual, bases, r)["failed"]
            for k, bit in QC.FAIL.items():
                (set_ if f & bit else clear)[k] += 1
    assert all(changed.values()), changed
    assert all(set_.values()) and all(clear.values()), (set_, clear)
    # the bodies: reads on both sides of 256 and of 1,024 positions
    lengths = {len(b) for _, b, _ in reads}
    assert {0, 1, 255, 256, 257, 1023, 1024, 1025} <= lengths and max(lengths) > 5000


def test_intersect_model():
    L = [10, 10, 10, 10, 0, 5]
    a = [[0, 10], [2, 20], [5, 5], [12, 15], [0, 3], [1, 4]]
    b = [[3, 7], [0, 3], [0, 10], [0, 10], [0, 1], [4, 9]]
    assert QC.intersect_model(L, a).tolist() == [[0, 10], [2, 10], [0, 0], [0, 0], [0, 0], [1, 4]]
    assert QC.intersect_model(L, a, b).tolist() == [[3, 7], [2, 3], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert QC.intersect_model(L, a, b, paired=True).tolist() == [[3, 7], [2, 3], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert QC.intersect_model(L, a, None, paired=True).tolist() == [[0, 10], [2, 10], [0, 0], [0, 0], [0, 0], [0, 0]]
