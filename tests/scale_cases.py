"""TEST INFRASTRUCTURE: the sizes, builders and self-checks of the tests that drive the count-table family past every grid cap (pure
numpy; no GPU import).  Each of these kernels hands out work with a capped grid and a stride loop; the named cases of the other tests are
too small to make a loop run a second time.  The caps are read out of the headers that define them, so every size here moves with a
retuned cap, and check_sizes() fails with a message that names the cap where a size no longer exceeds it (or where a cap has grown
so far that the test would no longer be quick).

Tiling rule, as in test_gpu_scan128_many_tiles.py: a block of whole sequences is laid end to end REPS times, the offsets shifted by
r * N.  REPS is even, so XOR digest words cancel; the block sizes are odd, so every repetition meets the lanes and the tiles at another
alignment.  No record crosses a block, so the expected output is the block's output tiled: every expected value comes from a Python
model run on ONE block, or from a closed form.  Nothing expected comes from the library."""
import functools
import os
import re

import numpy as np

import lookup_cases as LC
import read_counts_cases as RC
import read_quantiles_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "biolib_amd", "csrc")
H = RC.H  # positions of a tile of the 128-bit scans
U32 = (1 << 32) - 1
M64 = (1 << 64) - 1
MAX_POSITIONS = 1 << 24  # no tiled batch, table or query list grows beyond this: the tests stay quick

# header -> the names every test here needs from it
CAP_NAMES = {
    "bl_tile128.hpp": ("TILE_GRID_MAX",),
    "bl_read_quantiles_core.hpp": ("WAVE_GRID_MAX", "WG_GRID_MAX", "WG_TPB", "WAVE_MAX"),
    "bl_read_counts_launch.hpp": ("INIT_GRID_MAX", "ITPB"),
    "bl_lookup_core.hpp": ("LOOKUP_GRID_MAX", "HIST_LDS_GRID_MAX", "TABLE_GRID_MAX", "LTPB", "HIST_LDS_BINS", "HIST_LDS_KEYS_MIN", "G"),
}


def constants(header, csrc=CSRC):
    """every `constexpr int NAME = <product of numbers and earlier names>;` of a header"""
    with open(os.path.join(csrc, header)) as f:
        text = f.read()
    names = {}
    for name, expr in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([^;]+);", text):
        try:
            names[name] = int(eval(expr, {"__builtins__": {}}, dict(names)))
        except Exception:  # (an expression over something that is not a constexpr int of this header)
            pass
    return names


def caps(csrc=CSRC):
    """the caps and the constants they multiply, by name; every one must be found"""
    out = {}
    for header, wanted in CAP_NAMES.items():
        found = constants(header, csrc)
        for name in wanted:
            assert name in found, f"{name} not found in {header}"
            out[name] = found[name]
    return out


CAPS = caps()


def smallest_even(enough):
    """the smallest even REPS >= 2 with enough(REPS); gives up (returns None) where the batch would pass MAX_POSITIONS"""
    reps = 2
    while not enough(reps):
        reps += 2
        if reps > MAX_POSITIONS:
            return None
    return reps


# ---------------------------------------------------------------------------------------------- count scans: more than TILE_GRID_MAX tiles

def n_tiles(n_bases):
    return (n_bases + H - 1) // H


def scan_reps(cap=None):
    """the smallest even number of repetitions of the 9,199-base block that gives TILE_GRID_MAX + 4 tiles or more"""
    cap = CAPS if cap is None else cap
    return smallest_even(lambda reps: n_tiles(reps * RC.N) >= cap["TILE_GRID_MAX"] + 4 or reps * RC.N > MAX_POSITIONS)


def tiled_offsets(offs, n, reps):
    """the block's sequences at every repetition's offset, and the total"""
    starts = (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(n) + offs[None, :-1]).ravel()
    return np.append(starts, np.uint64(n * reps))


@functools.lru_cache(maxsize=None)
def scan_case(name, k):
    """the block read_counts_cases.case(name, k, True, False) x REPS: dict(block, reps, seq, offs, total, n_seqs)"""
    c = RC.case(name, k, True, False)
    n = len(c["seq"])
    assert n == RC.N and n % 2 == 1 and n % 16 == 15, "an odd block: every repetition at another alignment"
    assert int(c["offs"][0]) == 0 and int(c["offs"][-1]) == n, "whole sequences: a repetition starts a sequence"
    reps = scan_reps()
    offs = tiled_offsets(c["offs"], n, reps)
    return dict(block=c, reps=reps, seq=np.tile(c["seq"], reps), offs=offs, total=n * reps, n_seqs=len(offs) - 1)


def expected_positions(sc):
    """counts, valid (tiled, one per position) and the result words of Batch.kmer_counts over the whole tiled batch"""
    c, reps = sc["block"], sc["reps"]
    counts, valid, d = LC.expected_scan(c["m"], c["table"], 0, len(c["seq"]))
    assert d["count"] > 0 and d["xor_hash"] > 0 and d["xor_pos"] > 0
    assert reps % 2 == 0  # the XOR words cancel
    words = dict(count=d["count"] * reps & M64, found=d["xor_hash"] * reps & M64, sum_counts=d["xor_pos"] * reps & M64, xor_value=0, aux=0)
    return np.tile(counts, reps), np.tile(valid, reps), words


def expected_tiled_records(sc, min_count, untouched):
    """the records after one INIT call over the whole tiled batch into a buffer whose records all equal `untouched` (one RECORD): the
    block's records tiled; a record the block's own call leaves untouched (an empty first or last sequence) is the identity where it
    lies inside the tiled batch's touched span, and keeps what the buffer held outside it."""
    c, reps = sc["block"], sc["reps"]
    n = len(c["seq"])
    one = RC.expected_records(c["m"], c["table"], c["offs"], 0, n, min_count)
    canary = (one.view(np.uint8).reshape(len(one), 48) == RC.CANARY_BYTE).all(axis=1)
    out = np.tile(one, reps)
    lo, hi = RC.touched(sc["offs"], 0, sc["total"])
    idle = np.tile(canary, reps)
    inside = np.zeros(len(out), bool)
    inside[lo:hi + 1] = True
    out[idle & inside] = RC.IDENTITY
    out[idle & ~inside] = untouched
    assert not (idle & ~inside)[1:-1].any(), "only the batch's first and last record can lie outside the touched span"
    return out, (lo, hi)


def canary_record():
    return np.frombuffer(bytes([RC.CANARY_BYTE]) * 48, RC.RECORD)[0]


def first_differences(got, want, limit=8):
    """indices of the first differing records, for an assertion's message"""
    a = got.view(np.uint8).reshape(-1, 48)
    b = want.view(np.uint8).reshape(-1, 48)
    if a.shape != b.shape:
        return ("shapes", a.shape, b.shape)
    return np.nonzero((a != b).any(axis=1))[0][:limit].tolist()


def three_tile_read_cut(sc):
    """a position inside the read over three tiles (4000 .. 8300 of the ragged block) of a middle repetition"""
    c = sc["block"]
    assert c["name"] == "ragged" and 4000 in c["offs"].tolist() and 8300 in c["offs"].tolist()
    r = sc["reps"] // 2
    cut = r * RC.N + 5234
    i = int(RC.seq_index(sc["offs"], np.array([cut], np.uint64))[0])
    assert int(sc["offs"][i]) == r * RC.N + 4000 and int(sc["offs"][i + 1]) == r * RC.N + 8300 and 0 < r < sc["reps"] - 1
    return cut


# ---------------------------------------------------------------------------------------------- bl_select_read_counts past both caps

def quantile_reps(cap=None):
    """the smallest even number of repetitions of the quantile batch with more than 4 * WAVE_GRID_MAX + 200 sequences"""
    cap = CAPS if cap is None else cap
    b = QC.batch()
    per, n = len(b["offs"]) - 1, len(b["counts"])
    waves = cap["WG_TPB"] // 64
    return smallest_even(lambda reps: reps * per > waves * cap["WAVE_GRID_MAX"] + 200 or reps * n > MAX_POSITIONS)


@functools.lru_cache(maxsize=None)
def quantile_case():
    """read_quantiles_cases.batch() x REPS: dict(block, reps, names, counts, valid, offs) in the shape the GPU test's helpers take"""
    b = QC.batch()
    n = len(b["counts"])
    assert n % 2 == 1 and int(b["offs"][0]) == 0 and int(b["offs"][-1]) == n
    reps = quantile_reps()
    names = [f"{name}@{r}" for r in range(reps) for name in b["names"]]
    return dict(block=b, reps=reps, names=names, counts=np.tile(b["counts"], reps), valid=np.tile(b["valid"], reps), offs=tiled_offsets(b["offs"], n, reps),
                n_long=reps * b["forms"].count("workgroup"))


def long_cap(n_positions, n_seqs, cap=None):
    """entries of the list of long sequences, as the header's comment on it says: disjoint, each longer than WAVE_MAX"""
    cap = CAPS if cap is None else cap
    return min(n_positions // (cap["WAVE_MAX"] + 1), n_seqs)


def expected_quantiles(qc, first, end, quantiles):
    """(quantiles, n_kmers) over [first, end) of the tiled batch: the block's whole-range answer tiled, the guard on every sequence the
    range cuts (the rule of read_quantiles_cases.expected)"""
    b, reps = qc["block"], qc["reps"]
    q, m = QC.expected(b["counts"], b["valid"], b["offs"], 0, len(b["counts"]), quantiles)
    q, m = np.tile(q, (reps, 1)), np.tile(m, reps)
    offs = qc["offs"]
    whole = (offs[:-1] >= np.uint64(first)) & (offs[1:] <= np.uint64(end))
    q[~whole] = QC.GUARD
    m[~whole] = QC.GUARD
    return q, m, whole


def cut_range(qc):
    """(first, n): from a sequence boundary in a middle repetition to a position inside a long sequence of a later one"""
    b, reps = qc["block"], qc["reps"]
    n = len(b["counts"])
    a = QC.seq_index(b, "len129")
    z = QC.seq_index(b, "three_constants_and_7")
    first = (reps // 3) * n + int(b["offs"][a + 1])
    end = (reps - 2) * n + int(b["offs"][z]) + 100
    assert 0 < first < end < len(qc["counts"]) and int(b["offs"][z]) + 100 < int(b["offs"][z + 1])
    return first, end - first


def self_check_quantiles(qc, cap=None):
    cap = CAPS if cap is None else cap
    b = qc["block"]
    QC.self_check(b)
    n_seqs, n = len(qc["offs"]) - 1, len(qc["counts"])
    waves = cap["WG_TPB"] // 64
    assert n_seqs > waves * cap["WAVE_GRID_MAX"], f"WAVE_GRID_MAX: {n_seqs} sequences do not give a wave a second one"
    assert qc["n_long"] > cap["WG_GRID_MAX"], f"WG_GRID_MAX: {qc['n_long']} long sequences do not give a workgroup a second one"
    assert long_cap(n, n_seqs, cap) > cap["WG_GRID_MAX"], "WG_GRID_MAX: the workgroup grid is not at its cap"
    # consecutive long sequences of a block differ in what a stale histogram, prefix or rank would carry over
    longs = [i for i, f in enumerate(b["forms"]) if f == "workgroup"]
    q, m = QC.expected(b["counts"], b["valid"], b["offs"], 0, len(b["counts"]), QC.QUANTILES["inner"])
    for i, j in zip(longs, longs[1:] + longs[:1]):
        pair = (b["names"][i], b["names"][j])
        ci, cj = QC.piece(b, pair[0])[0], QC.piece(b, pair[1])[0]
        assert len(ci) != len(cj) or (ci != cj).any(), pair
        # (one multiset in two orders has one set of answers: the only such pair)
        assert (q[i] != q[j]).any() or m[i] != m[j] or pair == ("ascending_long", "descending_long"), pair
    ors = {b["names"][i]: int(np.bitwise_or.reduce(QC.piece(b, b["names"][i])[0][QC.piece(b, b["names"][i])[1] != 0], initial=0)) for i in longs}
    assert ors["all_zero_long"] == 0 and ors["random_full_width_long"] >> 24 and 0 < ors["all_equal_long"] < 256, "no digit pass, four, one"
    first, cnt = cut_range(qc)
    whole = expected_quantiles(qc, first, first + cnt, QC.QUANTILES["ends"])[2]
    assert 0 < int(whole.sum()) < n_seqs and not whole[0] and not whole[-1]
    return dict(sequences=n_seqs, positions=n, long_sequences=qc["n_long"], long_cap=long_cap(n, n_seqs, cap))


def sawtooth_offsets(b, cap=None):
    """wrong offsets with more passing long spans than the list of long sequences holds: 0, C + 1, 2 (C + 1) .. up to the batch's length,
    then again from 0 — every pair but the falling ones is a span of C + 1 positions inside the range, and the spans overlap"""
    cap = CAPS if cap is None else cap
    n, n_seqs = len(b["counts"]), len(b["offs"]) - 1
    step = cap["WAVE_MAX"] + 1
    per = n // step + 1
    offs = (np.arange(n_seqs + 1, dtype=np.uint64) % np.uint64(per)) * np.uint64(step)
    passing = int((offs[:-1] < offs[1:]).sum())
    assert int(offs.max()) <= n and passing > long_cap(n, n_seqs, cap), "more passing long spans than long_cap holds"
    return offs


def alternating_offsets(b):
    """0, n, 0, n ..: every second pair is the whole batch as one long span"""
    n, n_seqs = len(b["counts"]), len(b["offs"]) - 1
    return np.where(np.arange(n_seqs + 1) % 2 == 0, 0, n).astype(np.uint64)


def check_rows_under_wrong_offsets(b, bad, first, end, quantiles, got_q, got_m):
    """the property the contract fixes where the offsets are wrong: a row whose raw span (b, e) fails first <= b <= e <= end is all
    guard; any other row is all guard or the model's answer on counts[b:e].  Returns (rows written, long rows written)."""
    written = long_written = 0
    for i in range(len(bad) - 1):
        lo, hi = int(bad[i]), int(bad[i + 1])
        row_guard = (got_q[i] == QC.GUARD).all() and got_m[i] == QC.GUARD
        if not (first <= lo <= hi <= end):
            assert row_guard, ("a row outside the range was written", i, lo, hi, got_q[i].tolist(), int(got_m[i]))
            continue
        if row_guard:
            continue
        c, v = b["counts"][lo:hi], b["valid"][lo:hi]
        want = [QC.select(c, v, num, den) for num, den in quantiles]
        assert got_q[i].tolist() == want and int(got_m[i]) == int((v != 0).sum()), (i, lo, hi, got_q[i].tolist(), want, int(got_m[i]))
        written += 1
        long_written += hi - lo > QC.C
    return written, long_written


# ---------------------------------------------------------------------------------------------- lookup and spectrum past their caps

ODD = 0x2545F4914F6CDD1D       # key(i) = i * ODD mod 2^62: multiplication by an odd number is a bijection of the residues
ODD64 = 0x9E3779B97F4A7C15     # two-word keys: low word i * ODD64 mod 2^64 (a bijection: distinct i, distinct keys) ..
ODD2 = 0xD6E8FEB86659FD93      # .. high word i * ODD2 mod 2^38
KEY_BITS_1, KEY_BITS_2 = 62, 102
HIST_BINS = (1, 2, 4096, 8192, 8193, 65536)


def table_size(cap=None):
    cap = CAPS if cap is None else cap
    return cap["HIST_LDS_GRID_MAX"] * cap["HIST_LDS_KEYS_MIN"] + cap["HIST_LDS_KEYS_MIN"] + 1


def query_count(cap=None):
    cap = CAPS if cap is None else cap
    group = cap["LTPB"] * cap["G"]
    return cap["LOOKUP_GRID_MAX"] * group + group + 1


def keys_of(i, key_words):
    """the closed-form keys of the indices i (uint64 array): uint64[len] or uint64[len, 2] (low, high)"""
    i = np.asarray(i, np.uint64)
    with np.errstate(over="ignore"):
        if key_words == 1:
            return (i * np.uint64(ODD)) & np.uint64((1 << KEY_BITS_1) - 1)
        return np.stack([i * np.uint64(ODD64), (i * np.uint64(ODD2)) & np.uint64((1 << (KEY_BITS_2 - 64)) - 1)], axis=1)


@functools.lru_cache(maxsize=None)
def table_counts():
    """counts of the n table keys: seeded, below 70,000, with every edge of every histogram width and of the count's range"""
    n = table_size()
    counts = np.random.default_rng(8).integers(0, 70000, n, dtype=np.uint64).astype(np.uint32)
    edges = sorted({0, 1, U32} | {max(nb + d, 0) for nb in HIST_BINS for d in (-2, -1, 0)})
    counts[np.arange(len(edges)) * 1013 + 5] = np.array(edges, np.uint64).astype(np.uint32)
    counts.setflags(write=False)
    return counts


@functools.lru_cache(maxsize=None)
def query_indices():
    """indices drawn from [0, 2n): about half are in the table (i < n), the others absent"""
    idx = np.random.default_rng(9).integers(0, 2 * table_size(), query_count(), dtype=np.uint64)
    idx.setflags(write=False)
    return idx


def expected_lookup():
    idx, counts, n = query_indices(), table_counts(), table_size()
    return np.where(idx < n, counts[np.minimum(idx, n - 1)], 0).astype(np.uint32)


def expected_histogram(n_bins):
    return np.bincount(np.minimum(table_counts().astype(np.int64), n_bins - 1), minlength=n_bins).astype(np.uint64)


def self_check_tables(cap=None):
    cap = CAPS if cap is None else cap
    n, nq = table_size(cap), query_count(cap)
    for kw in (1, 2):  # distinct keys, checked on a sample and by the bijection argument
        sample = keys_of(np.arange(1 << 16, dtype=np.uint64) * np.uint64(257), kw)
        assert len(np.unique(sample, axis=0)) == len(sample)
    assert ODD % 2 == 1 and ODD64 % 2 == 1 and 2 * n < 1 << 62
    present = float((query_indices() < n).mean())
    assert 0.45 < present < 0.55
    return dict(keys=n, queries=nq)


# ---------------------------------------------------------------------------------------------- every derived size against its cap

def check_sizes(cap=None):
    """every derived size exceeds the cap it is meant to exceed, and no cap has grown so far that a test would stop being quick.
    Each message names the cap.  Returns the sizes, for the record."""
    cap = CAPS if cap is None else cap
    out = {}
    # count scans
    reps = scan_reps(cap)
    total = (reps or 0) * RC.N
    assert reps is not None and total <= MAX_POSITIONS, f"TILE_GRID_MAX = {cap['TILE_GRID_MAX']}: more than {MAX_POSITIONS} positions would be needed"
    assert n_tiles(total) > cap["TILE_GRID_MAX"], f"TILE_GRID_MAX = {cap['TILE_GRID_MAX']}: {n_tiles(total)} tiles give no workgroup a second tile"
    fixed7 = reps * (len(RC.fixed_offsets(RC.N, 7)) - 1)
    threads = cap["INIT_GRID_MAX"] * cap["ITPB"]
    assert fixed7 > threads, f"INIT_GRID_MAX = {cap['INIT_GRID_MAX']}: {fixed7} touched records do not exceed the fill's {threads} threads"
    out["scan"] = dict(reps=reps, positions=total, tiles=n_tiles(total), fixed7_sequences=fixed7, init_threads=threads)
    # quantiles
    b = QC.batch()
    qreps = quantile_reps(cap)
    per, n, longs = len(b["offs"]) - 1, len(b["counts"]), b["forms"].count("workgroup")
    waves = cap["WG_TPB"] // 64
    assert qreps is not None and qreps * n <= MAX_POSITIONS, f"WAVE_GRID_MAX = {cap['WAVE_GRID_MAX']}: more than {MAX_POSITIONS} positions would be needed"
    assert qreps * per > waves * cap["WAVE_GRID_MAX"], f"WAVE_GRID_MAX = {cap['WAVE_GRID_MAX']}: {qreps * per} sequences give no wave a second one"
    assert qreps * longs > cap["WG_GRID_MAX"], f"WG_GRID_MAX = {cap['WG_GRID_MAX']}: {qreps * longs} long sequences give no workgroup a second one"
    assert long_cap(qreps * n, qreps * per, cap) > cap["WG_GRID_MAX"], f"WG_GRID_MAX = {cap['WG_GRID_MAX']}: the workgroup grid stays below it"
    out["quantiles"] = dict(reps=qreps, sequences=qreps * per, positions=qreps * n, long_sequences=qreps * longs, long_cap=long_cap(qreps * n, qreps * per, cap),
                            waves=waves * cap["WAVE_GRID_MAX"])
    # lookup and histogram
    n, nq = table_size(cap), query_count(cap)
    group = cap["LTPB"] * cap["G"]
    assert nq <= MAX_POSITIONS, f"LOOKUP_GRID_MAX = {cap['LOOKUP_GRID_MAX']}: {nq} queries are more than {MAX_POSITIONS}"
    assert nq > cap["LOOKUP_GRID_MAX"] * group, f"LOOKUP_GRID_MAX = {cap['LOOKUP_GRID_MAX']}: {nq} queries give no workgroup a second group"
    assert n <= MAX_POSITIONS, f"HIST_LDS_GRID_MAX = {cap['HIST_LDS_GRID_MAX']}: {n} keys are more than {MAX_POSITIONS}"
    lds = [nb for nb in HIST_BINS if nb <= cap["HIST_LDS_BINS"]]
    assert cap["HIST_LDS_BINS"] in lds and cap["HIST_LDS_BINS"] + 1 in HIST_BINS, f"HIST_LDS_BINS = {cap['HIST_LDS_BINS']}: the widths on either side of it are not run"
    capped = [nb for nb in lds if n > cap["HIST_LDS_GRID_MAX"] * max(nb, cap["HIST_LDS_KEYS_MIN"])]
    assert cap["HIST_LDS_KEYS_MIN"] in capped and 1 in capped, f"HIST_LDS_GRID_MAX = {cap['HIST_LDS_GRID_MAX']}: {n} keys leave the LDS histogram's grid below it"
    assert n > cap["TABLE_GRID_MAX"] * cap["LTPB"], f"TABLE_GRID_MAX = {cap['TABLE_GRID_MAX']}: {n} keys give no thread of the global histogram a second key"
    out["table"] = dict(keys=n, queries=nq, lookup_capacity=cap["LOOKUP_GRID_MAX"] * group, lds_capacity=cap["HIST_LDS_GRID_MAX"] * cap["HIST_LDS_KEYS_MIN"],
                        global_threads=cap["TABLE_GRID_MAX"] * cap["LTPB"])
    return out
