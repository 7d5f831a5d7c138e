"""CPU-only: the bodies of bl_scan_read_counts (biolib_amd/csrc/bl_read_counts_core.hpp: the lane's segments, the wave's segmented scan,
the flushes, the index search and the identity fill) emulated on the host under AddressSanitizer / UBSan (tests/emu/emu_read_counts.cpp)
over record and offset arrays of exactly their lengths, against the Python model (read_counts_cases.py).  Index bugs are to be found
here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import lookup_cases as LC
import read_counts_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
INIT, ACCUMULATE, FILL = 0, 1, 2


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_read_counts.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_read_counts")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


class Files:
    """the batch, table and offsets of one case on disk"""

    def __init__(self, tmp_path, c, key_words):
        self.c = c
        self.batch = tmp_path / "batch.bin"
        self.table = tmp_path / "table.bin"
        self.offsets = tmp_path / "offsets.bin"
        self.batch.write_bytes(RC.batch_file(c["seq"], c["offs"]))
        self.table.write_bytes(RC.table_file(c["table"], key_words, c["k"]))
        self.offsets.write_bytes(c["offs"].tobytes())

    def run(self, exe, min_count, calls, offsets="given"):
        """calls: (first, n, mode) triples -> (result lines as integer lists, RECORD array)"""
        c = self.c
        cmd = [exe, self.batch, self.table, "-" if offsets is None else self.offsets, c["read_len"] if offsets is None else 0, c["k"], int(c["canonical"]),
               int(c["drop_last"]), min_count] + [x for call in calls for x in call]
        run = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        lines = [ln.split() for ln in run.stdout.splitlines()]
        return [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "result"], RC.parse_records(lines)


def check_result(c, got, first, n):
    end = len(c["seq"]) if n == 0 else first + n
    d = LC.expected_scan(c["m"], c["table"], first, end)[2]
    assert got == [first, n, d["count"], d["xor_value"], d["aux"], d["xor_hash"], d["xor_pos"]], (c["name"], c["k"], first, n)


def check_case(exe, files, min_count, offsets="given"):
    """the whole batch and lookup_cases' second range under INIT; three ACCUMULATE ranges cut mid-read that equal the whole"""
    c = files.c
    n_bases = len(c["seq"])
    tag = (c["name"], c["k"], c["canonical"], c["drop_last"], min_count, offsets)
    whole = None
    for first, n in LC.RANGES:
        end = n_bases if n == 0 else first + n
        results, records = files.run(exe, min_count, [(first, n, INIT)], offsets)
        check_result(c, results[0], first, n)
        want = RC.expected_records(c["m"], c["table"], c["offs"], first, end, min_count)
        assert RC.same(records, want), (tag, first, n, np.nonzero(records != want)[0][:8])
        whole = want if n == 0 and first == 0 else whole
    a, b = 4000 + 1234, 8300 + 3  # inside the read over three tiles; inside a read of k + 2 bases (ragged), anywhere (the others)
    results, records = files.run(exe, min_count, [(0, 0, FILL), (b, 0, ACCUMULATE), (0, a, ACCUMULATE), (a, b - a, ACCUMULATE)], offsets)
    for got, (first, n) in zip(results, ((b, 0), (0, a), (a, b - a))):
        check_result(c, got, first, n)
    filled = whole.copy()
    filled[(whole.view(np.uint8) == RC.CANARY_BYTE).reshape(len(whole), 48).all(axis=1)] = RC.IDENTITY  # the untouched: the caller's fill
    assert RC.same(records, filled), (tag, "accumulate", np.nonzero(records != filled)[0][:8])


@pytest.mark.parametrize("k", RC.KS)
def test_cases_hold_the_shapes(k):
    for canonical in (False, True):
        for drop_last in (False, True):
            RC.self_check(RC.case("ragged", k, canonical, drop_last))


@pytest.mark.parametrize("k", RC.KS)
def test_emulated_records_match_model(exe, tmp_path, k):
    runs = 0
    for canonical in (False, True):
        for drop_last in (False, True):
            c = RC.case("ragged", k, canonical, drop_last)
            files = Files(tmp_path, c, 1 if (k <= 32 and not canonical) else 2)  # both key widths where k <= 32 (the search itself: test_emu_lookup.py)
            for min_count in RC.MIN_COUNTS:
                check_case(exe, files, min_count)
                runs += 1
    assert runs == 12


@pytest.mark.parametrize("name", ("single",) + tuple(f"fixed{length}" for length in RC.FIXED))
def test_single_sequence_and_fixed_length_batches(exe, tmp_path, name):
    """with the offsets (bisection) and without them (sequence = position / read_len, or 0)"""
    for k, canonical, drop_last, min_count in ((16, False, True, 2), (33, True, False, 1)):
        c = RC.case(name, k, canonical, drop_last)
        assert c["null_ok"]
        files = Files(tmp_path, c, 2)
        check_case(exe, files, min_count, offsets="given")
        check_case(exe, files, min_count, offsets=None)


def test_wrong_offsets_end_clean(exe, tmp_path):
    """a shuffled offsets array whose last entry is too large: the statistics may be anything, the run ends clean under the sanitizers
    (records and offsets are heap arrays of exactly their lengths) and the digest, which no offset enters, stays right"""
    for k, canonical in ((16, False), (64, True)):
        c = RC.case("ragged", k, canonical, False)
        files = Files(tmp_path, c, 2)
        for seed in range(3):
            files.offsets.write_bytes(RC.wrong_offsets(c["offs"], np.random.default_rng(seed)).tobytes())
            results, records = files.run(exe, 1, [(0, 0, INIT), (37, 8200, ACCUMULATE), (5234, 0, INIT)])
            for got, (first, n) in zip(results, ((0, 0), (37, 8200), (5234, 0))):
                check_result(c, got, first, n)
            assert len(records) == len(c["offs"]) - 1
