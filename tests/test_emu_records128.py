"""CPU-only: the super-k-mer scan that builds 32-byte records inside its record pass (bl_scan_super_kmer_records128), emulated on the
host under AddressSanitizer / UBSan (tests/emu/emu_records128.cpp: the count -> prefix scan -> emit pipeline of emu_scan.cpp with
ScanParams::records128 set).  The emulation poisons the code arrays of every tile and stages exactly what staged_chunks gives, so a
group whose bases lie behind what pass 1 spilled packs poison and differs from the model — which is what the tile-edge ranges of
tests/records128_cases.py are aimed at.  Expected values: superkmer128_model.pack over the oracle's groups."""
import os
import struct
import subprocess

import numpy as np
import pytest

import records128_cases as R
import tie_plant as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
IDS = [f"k{k}-m{m}" for k, m in R.SHAPES]


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_records128.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_records128")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=900)
    return out


def run_jobs(exe, tmp_path, seq, offs, read_len, k, m, canonical, jobs):
    """[(records uint64[g, 4], hashes uint64[g], group ends)] per (first, n) of jobs"""
    offs = np.zeros(0, np.uint64) if offs is None else np.ascontiguousarray(offs, np.uint64)
    src, dst = tmp_path / "batch.in", tmp_path / "records.out"
    src.write_bytes(struct.pack("<8Q", len(seq), len(offs), read_len, k, m, R.SEED, 1 if canonical else 0, len(jobs))
                    + np.asarray([(f, n) for f, n in jobs], np.uint64).tobytes() + offs.tobytes() + np.ascontiguousarray(seq, np.uint8).tobytes())
    run = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    raw = np.frombuffer(dst.read_bytes(), np.uint64)
    out, at = [], 0
    for _ in jobs:
        cnt, ends = int(raw[at]), int(raw[at + 1])
        out.append((raw[at + 2:at + 2 + 4 * cnt].reshape(-1, 4), raw[at + 2 + 4 * cnt:at + 2 + 5 * cnt], ends))
        at += 2 + 5 * cnt
    assert at == len(raw)
    return out


def check(got, want, what):
    recs, hs, ends = got
    assert len(recs) == len(want[0]) == ends, (what, len(recs), len(want[0]), ends)
    bad = np.nonzero((recs != want[0]).any(1))[0]
    assert len(bad) == 0, (what, "first differing records", bad[:5].tolist(), [hex(int(x)) for x in recs[bad[0]]], [hex(int(x)) for x in want[0][bad[0]]])
    assert np.array_equal(hs, want[1]), what


def test_the_tile_length_formula_is_the_emulations(exe):
    """tests/records128_cases.py and the GPU test place groups by tie_plant.plan_pos: it must be what the scan plans"""
    for k, m in R.SHAPES:
        w = k - m + 1
        for first in (0, 1, 17, 5000):
            out = subprocess.run([exe, "plan", str(first), "0", str(R.BIG), "0", str(m), str(w), "1"], capture_output=True, text=True, check=True).stdout.split()
            g = P.plan_pos(P.MODE_SUPERKMER, first, R.BIG, w)
            assert [int(x) for x in out[:4]] == [0, g["origin"], g["stride"], g["n_tiles"]], (k, m, first)
            assert g["stride"] == R.stride_of(w)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,m", R.SHAPES, ids=IDS)
def test_layouts(exe, tmp_path, k, m, canonical):
    """whole batches (one contig of a few tiles, ragged reads with N's, 150-bp reads, a batch shorter than a tile) and a sub-range"""
    for name, make in R.LAYOUTS.items():
        seq, offs, read_len = make(k)
        exp = R.Expect(seq, offs, read_len, k, m, canonical)
        assert len(exp.fp) > (3 if name == "short" else 100), name
        n = len(seq)
        jobs = [(0, 0)] + ([(1234, 5000), (n - 122, 0)] if name == "contig" else []) + ([(150 * 7, 150 * 200)] if name == "reads150" else [])
        if name in ("contig", "short"):  # the batch's end: a group inside its last 122 bases, packed from chunks that end with the batch
            assert int((exp.fp >= n - 122).sum()) >= 1
        for job, got in zip(jobs, run_jobs(exe, tmp_path, seq, offs, read_len, k, m, canonical, jobs)):
            check(got, exp.of_range(*job), (name, job))


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,m", R.SHAPES, ids=IDS)
def test_full_size_groups_at_the_last_positions_a_tile_owns(exe, tmp_path, k, m, canonical):
    import oracle_lib as O

    seq = O.synth(77 + k, R.BIG)
    exp = R.Expect(seq, None, 0, k, m, canonical)
    jobs = R.edge_jobs(exp, k, m)
    assert len(jobs) == 4 * R.EDGE_PICKS
    got = run_jobs(exe, tmp_path, seq, None, 0, k, m, canonical, [(f, n) for f, n, _, _ in jobs])
    for (first, n, placement, g), res in zip(jobs, got):
        want = exp.of_range(first, n)
        check(res, want, (placement, first, n))
        # the picked group is in the answer, whole (2k - m bases) or cut to its first k-mer
        at = int(np.searchsorted(exp.fp[(exp.fp + exp.sz - 1) >= first], exp.fp[g]))
        size = int(res[0][at][3] & np.uint64(63)) + 1
        assert size == (1 if first + n == int(exp.fp[g]) + 1 else k - m + 1), (placement, first, n, size)
