"""The model of bl_select_read_counts and the cases its tests run (test_emu_read_quantiles.py on the host, test_gpu_read_quantiles.py on
the device).  Pure numpy: per sequence the sorted valid counts, indexed at min(m - 1, m * num // den), in uint32 / Python integers.  The
constants that decide which form a sequence takes are read out of biolib_amd/csrc/bl_read_quantiles_core.hpp, so the cases move with
a retuned constant.  The cases are built straight from (counts, valid, offsets) arrays — the call is independent of the scan that
usually fills them — so the counts can be adversarial.  Every sequence carries a name; self_check asserts on the model that it sits
where the name says: which form takes it, and where the rank falls."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "biolib_amd", "csrc", "bl_read_quantiles_core.hpp")
GUARD = 0xC5C5C5C5
U32 = 0xFFFFFFFF


def limits(source=SOURCE):
    """the constants of the two forms, read from the core header; every one must be found"""
    with open(source) as f:
        text = f.read()
    names = {}
    for name, expr in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([^;]+);", text):
        names[name] = int(eval(expr, {"__builtins__": {}}, dict(names)))  # (products of earlier constants)
    for name in ("MAX_Q", "WAVE_SLOTS", "WAVE_MAX", "WAVE_SLOTS_SHORT", "WG_TPB", "WG_UNROLL", "WG_CHUNK"):
        assert name in names, f"{name} not found in {source}"
    assert names["WAVE_MAX"] == 64 * names["WAVE_SLOTS"] and names["WG_CHUNK"] == names["WG_TPB"] * names["WG_UNROLL"]
    return names


LIM = limits()
C = LIM["WAVE_MAX"]                   # the longest sequence of the wave form
SHORT = 64 * LIM["WAVE_SLOTS_SHORT"]  # the longest sequence of the wave form's short body
CHUNK = LIM["WG_CHUNK"]               # positions per step of a workgroup-form pass

# quantile sets: n_q = 4 twice (every quantile of the list between them), n_q = 1, and the same quantile twice
QUANTILES = {
    "ends": ((0, 1), (1, 1), (1, 2), (1, 4)),
    "inner": ((3, 4), (999, 1000), (1, 1000), (1, 2)),
    "median": ((1, 2),),
    "twice": ((1, 2), (1, 2)),
}


def form(length):
    return "wave_short" if length <= SHORT else "wave" if length <= C else "workgroup"


def rank(m, num, den):
    return min(m - 1, m * num // den)


def select(counts, valid, num, den):
    """the model: one sequence, one quantile"""
    v = np.sort(np.asarray(counts, np.uint32)[np.asarray(valid) != 0])
    return int(v[rank(len(v), num, den)]) if len(v) else 0


def expected(counts, valid, offs, first, end, quantiles, guard=GUARD):
    """(quantiles uint32[n_seqs, n_q], n_kmers uint32[n_seqs]); counts / valid cover the whole batch.  The sequences the range cuts
    keep the guard."""
    n_seqs = len(offs) - 1
    q = np.full((n_seqs, len(quantiles)), guard, np.uint32)
    m = np.full(n_seqs, guard, np.uint32)
    for i in range(n_seqs):
        b, e = int(offs[i]), int(offs[i + 1])
        if first <= b and e <= end:
            m[i] = int((valid[b:e] != 0).sum())
            q[i] = [select(counts[b:e], valid[b:e], num, den) for num, den in quantiles]
    return q, m


def fixed_offsets(n_bases, read_len):
    return np.append(np.arange(0, n_bases, read_len, dtype=np.uint64), np.uint64(n_bases))


# ---------------------------------------------------------------------------------------------------------------- the sequences

def _all_valid(values):
    values = np.asarray(values, np.uint64).astype(np.uint32)
    return values, np.ones(len(values), np.uint8)


def _lengths(rng):
    """(name, counts, valid, form expected)"""
    out = []

    def add(name, n, valid=None, want=None):
        counts = rng.integers(0, 1000, n).astype(np.uint32)
        ok = np.ones(n, np.uint8) if valid is None else valid
        counts[ok == 0] = 0  # as the scan writes them
        out.append((name, counts, ok, want or form(n)))

    add("empty_first", 0)
    for n in (1, 2, 3):
        add(f"len{n}", n, want="wave_short")
    add("no_valid", 5, np.zeros(5, np.uint8))
    add("empty_between", 0)
    for n in (63, 64, 65, 127, 128, 129):
        add(f"len{n}", n, want="wave_short")
    for n in (SHORT - 1, SHORT):
        add(f"short{n}", n, want="wave_short")
    add(f"short{SHORT + 1}", SHORT + 1, want="wave")
    for n in (C - 1, C):
        add(f"switch{n}", n, want="wave")
    add(f"switch{C + 1}", C + 1, want="workgroup")
    add("three_constants_and_7", 3 * C + 7, want="workgroup")
    add("chunks_and_5", 3 * CHUNK + 5, want="workgroup")
    add("chunks_exactly", 2 * CHUNK, want="workgroup")
    # valid holes: an N break across the lane edge 63 | 64, only the first / only the last position valid
    hole = np.ones(200, np.uint8)
    hole[58:71] = 0
    add("hole_over_lane_edge", 200, hole)
    for name, n in (("", 100), ("_long", C + 300)):
        only = np.zeros(n, np.uint8)
        only[0] = 1
        add("only_first_valid" + name, n, only.copy())
        only[[0, -1]] = 0, 1
        add("only_last_valid" + name, n, only)
    wide = np.ones(C + 500, np.uint8)
    wide[C - 10:C + 40] = 0
    wide[::7] = 0
    add("holes_long", C + 500, wide)
    return out


def _values(rng):
    """every value pattern at a wave-form and a workgroup-form length; (name, counts, valid, form expected)"""
    out = []
    for tag, n in (("", 150), ("_long", C + 77)):
        want = form(n)
        half = n // 2

        def add(name, values, valid=None):
            counts, ok = _all_valid(values)
            assert len(counts) == n
            out.append((name + tag, counts, ok if valid is None else valid, want))

        add("all_equal", np.full(n, 7))
        add("all_zero", np.zeros(n))
        add("all_ones", np.full(n, U32))
        add("above_2_31", rng.integers(1 << 31, 1 << 32, n))          # the torch trap: negative as int32
        add("around_2_31", rng.integers((1 << 31) - 40, (1 << 31) + 40, n))
        add("bit0_only", 0x12345678 + rng.integers(0, 2, n))
        add("bit31_only", 0x12345678 + (rng.integers(0, 2, n) << 31))
        add("byte1_only", 0x12340078 + (rng.integers(0, 256, n) << 8))
        add("byte2_only", 0x12005678 + (rng.integers(0, 256, n) << 16))
        add("ascending", np.arange(n) * 3 + 1)
        add("descending", (np.arange(n) * 3 + 1)[::-1])
        # two distinct values: the median's rank n // 2 on the last element of the lower run / on the first of the upper run
        add("rank_last_of_lower", rng.permutation(np.where(np.arange(n) <= half, 5, 300)))
        add("rank_first_of_upper", rng.permutation(np.where(np.arange(n) < half, 5, 300)))
        dup = np.concatenate([rng.integers(0, 50, half - 3), np.full(7, 50), rng.integers(51, 90, n - half - 4)])
        add("duplicates_straddle", rng.permutation(dup))
        outlier = rng.integers(1, 60, n)
        outlier[n // 3] = U32
        add("outlier", outlier)
        add("random_full_width", rng.integers(0, 1 << 32, n))
    return out


def batch():
    """One ragged batch of every sequence above, an empty one at either end: dict(names, forms, counts, valid, offs)"""
    rng = np.random.default_rng(20)
    seqs = _lengths(rng) + _values(rng)
    seqs.append(("empty_last", np.zeros(0, np.uint32), np.zeros(0, np.uint8), "wave_short"))
    lengths = [len(s[1]) for s in seqs]
    return dict(names=[s[0] for s in seqs], forms=[s[3] for s in seqs], counts=np.concatenate([s[1] for s in seqs]).astype(np.uint32),
                valid=np.concatenate([s[2] for s in seqs]).astype(np.uint8), offs=np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64))


def seq_index(b, name):
    return b["names"].index(name)


def piece(b, name):
    i = seq_index(b, name)
    lo, hi = int(b["offs"][i]), int(b["offs"][i + 1])
    return b["counts"][lo:hi], b["valid"][lo:hi]


def self_check(b):
    """every sequence sits where its name says"""
    names, offs = b["names"], b["offs"]
    assert len(set(names)) == len(names)
    assert names[0] == "empty_first" and names[-1] == "empty_last" and offs[0] == offs[1] and offs[-1] == offs[-2]
    for i, (name, want) in enumerate(zip(names, b["forms"])):
        assert form(int(offs[i + 1] - offs[i])) == want, name
    assert {"wave_short", "wave", "workgroup"} == set(b["forms"])
    for tag in ("", "_long"):
        c, v = piece(b, "rank_last_of_lower" + tag)
        s = np.sort(c)
        r = rank(len(s), 1, 2)
        assert s[r] == 5 and s[r + 1] == 300, "the median is the last element of the lower run"
        c, v = piece(b, "rank_first_of_upper" + tag)
        s = np.sort(c)
        r = rank(len(s), 1, 2)
        assert s[r] == 300 and s[r - 1] == 5, "the median is the first element of the upper run"
        c, v = piece(b, "duplicates_straddle" + tag)
        s = np.sort(c)
        r = rank(len(s), 1, 2)
        assert s[r - 1] == s[r] == s[r + 1], "duplicates on both sides of the rank"
        c, v = piece(b, "outlier" + tag)
        assert c.max() == U32 and select(c, v, 1, 2) < 60 and select(c, v, 1, 1) == U32 and select(c, v, 3, 4) < 60
        c, v = piece(b, "above_2_31" + tag)
        assert (c >= 1 << 31).all()
        c, v = piece(b, "around_2_31" + tag)
        assert (c < 1 << 31).any() and (c >= 1 << 31).any()
        assert int(np.sort(c.view(np.int32)).view(np.uint32)[len(c) // 2]) != select(c, v, 1, 2), "a signed sort gives another median"
        for name, mask in (("bit0_only", 1), ("bit31_only", 1 << 31), ("byte1_only", 0xFF00), ("byte2_only", 0xFF0000)):
            c, v = piece(b, name + tag)
            assert len(np.unique(c)) > 1 and len(np.unique(c & ~np.uint32(mask))) == 1, name
    c, v = piece(b, "hole_over_lane_edge")
    assert v[58] == 0 and v[63] == 0 and v[64] == 0 and v[70] == 0 and v[57] == 1 and v[71] == 1
    for tag in ("", "_long"):
        assert piece(b, "only_first_valid" + tag)[1].nonzero()[0].tolist() == [0]
        v = piece(b, "only_last_valid" + tag)[1]
        assert v.nonzero()[0].tolist() == [len(v) - 1]
    assert piece(b, "no_valid")[1].sum() == 0 and len(piece(b, "no_valid")[1]) == 5
    # the rank conventions on 1, 2 and 3 values: (1, 2) is sorted[m // 2], (1, 1) is clamped to m - 1
    assert [rank(m, 1, 2) for m in (1, 2, 3)] == [0, 1, 1] and [rank(m, 1, 1) for m in (1, 2, 3)] == [0, 1, 2]
    assert [rank(m, 0, 1) for m in (1, 2, 3)] == [0, 0, 0] and rank(1000, 999, 1000) == 999 and rank(150, 999, 1000) == 149
    assert rank(150, 1, 1000) == 0 and rank(C + 77, 1, 1000) == 1


def ranges(b):
    """(name, first, n): ranges over the batch; self-checked against what the name says"""
    offs = b["offs"]
    n_bases = int(offs[-1])
    a = seq_index(b, "len129")
    z = seq_index(b, "three_constants_and_7")
    w = seq_index(b, "chunks_and_5")
    out = [
        ("whole", 0, 0),
        ("cut_both_ends", int(offs[a]) + 17, int(offs[z]) + 100 - int(offs[a]) - 17),  # first inside len129, the end inside a long sequence
        ("no_whole_sequence", int(offs[w]) + 3, CHUNK),                                 # inside one long sequence
        ("to_the_end", int(offs[a + 1]), 0),                                           # n = 0 from a sequence's first position
        ("from_the_start", 0, int(offs[z + 1])),                                       # ends on a boundary: that sequence is written
    ]
    for name, first, n in out:
        end = n_bases if n == 0 else first + n
        whole = [i for i in range(len(offs) - 1) if first <= offs[i] and offs[i + 1] <= end]
        if name == "cut_both_ends":
            assert offs[a] < first < offs[a + 1] and offs[z] < end < offs[z + 1] and whole == list(range(a + 1, z))
        if name == "no_whole_sequence":
            assert whole == [] and offs[w] < first and end < offs[w + 1]
        if name == "from_the_start":
            assert whole[-1] == z
    return out


def wrong_offsets(offs, rng):
    """a shuffled copy whose last entry is too large: what the call may see from a careless caller"""
    bad = offs.copy()
    rng.shuffle(bad)
    bad[-1] = offs[-1] + 12345
    return bad
