"""CPU-only: the bodies of bl_select_read_counts (biolib_amd/csrc/bl_read_quantiles_core.hpp: the wave form, the workgroup form, the
dispatch between them and the search for the range's sequences) emulated on the host under AddressSanitizer / UBSan
(tests/emu/emu_read_quantiles.cpp) over arrays of exactly their lengths, against the numpy model (read_quantiles_cases.py).  Index
bugs are to be found here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import read_quantiles_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_read_quantiles.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_read_quantiles")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


@pytest.fixture(scope="module")
def batch():
    b = QC.batch()
    QC.self_check(b)
    return b


def run(exe, tmp_path, counts, valid, offs, n_seqs, first, n, quantiles, read_len=0, grid=3, offsets_file=None):
    """the emulated call over counts[first:end], valid[first:end] -> (quantiles [n_seqs, n_q], n_kmers [n_seqs])"""
    n_bases = len(counts)
    end = n_bases if n == 0 else first + n
    (tmp_path / "counts.bin").write_bytes(np.ascontiguousarray(counts[first:end], np.uint32).tobytes())
    (tmp_path / "valid.bin").write_bytes(np.ascontiguousarray(valid[first:end], np.uint8).tobytes())
    if offs is not None:
        (tmp_path / "offsets.bin").write_bytes(np.ascontiguousarray(offs, np.uint64).tobytes())
    cmd = [exe, tmp_path / "counts.bin", tmp_path / "valid.bin", "-" if offs is None else tmp_path / "offsets.bin", read_len, n_bases, n_seqs, first, n, grid,
           len(quantiles)] + [x for q in quantiles for x in q]
    r = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [[int(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("seq ")]
    assert [row[0] for row in rows] == list(range(n_seqs))
    got = np.array([row[1:] for row in rows], np.uint32).reshape(n_seqs, 1 + len(quantiles))
    return got[:, 1:], got[:, 0]


def same(b, got, want, tag):
    for what, g, w in (("quantiles", got[0], want[0]), ("n_kmers", got[1], want[1])):
        bad = np.nonzero((g != w).reshape(len(w), -1).any(axis=1))[0]
        assert len(bad) == 0, (tag, what, [(b["names"][i], g[i].tolist(), w[i].tolist()) for i in bad[:6]])


def test_constants_and_cases(batch):
    assert QC.LIM["MAX_Q"] == 4 and QC.SHORT < QC.C  # (the cases are built from whatever else the header says)
    assert [QC.form(n) for n in (QC.SHORT, QC.SHORT + 1, QC.C, QC.C + 1)] == ["wave_short", "wave", "wave", "workgroup"]
    assert len(batch["names"]) == 60


@pytest.mark.parametrize("qname", sorted(QC.QUANTILES))
def test_every_sequence_and_quantile(exe, tmp_path, batch, qname):
    b, q = batch, QC.QUANTILES[qname]
    n_seqs = len(b["offs"]) - 1
    got = run(exe, tmp_path, b["counts"], b["valid"], b["offs"], n_seqs, 0, 0, q)
    same(b, got, QC.expected(b["counts"], b["valid"], b["offs"], 0, len(b["counts"]), q), qname)
    assert (got[1] != QC.GUARD).all(), "the whole batch: every sequence is written, the empty ones too"


def test_ranges_keep_the_guard_on_cut_sequences(exe, tmp_path, batch):
    b, q = batch, QC.QUANTILES["ends"]
    n_seqs, n_bases = len(b["offs"]) - 1, len(b["counts"])
    for name, first, n in QC.ranges(b):
        end = n_bases if n == 0 else first + n
        for grid in (1, 7):
            got = run(exe, tmp_path, b["counts"], b["valid"], b["offs"], n_seqs, first, n, q, grid=grid)
            same(b, got, QC.expected(b["counts"], b["valid"], b["offs"], first, end, q), (name, grid))
        if name == "no_whole_sequence":
            assert (got[0] == QC.GUARD).all() and (got[1] == QC.GUARD).all()


def test_fixed_length_and_single_sequence_without_offsets(exe, tmp_path):
    rng = np.random.default_rng(5)
    q = QC.QUANTILES["inner"]
    for read_len, n_bases in ((150, 150 * 40 + 77), (QC.C + 1, 3 * (QC.C + 1)), (64, 640)):
        counts = rng.integers(0, 300, n_bases).astype(np.uint32)
        valid = (rng.random(n_bases) < 0.9).astype(np.uint8)
        offs = QC.fixed_offsets(n_bases, read_len)
        n_seqs = len(offs) - 1
        for first, n in ((0, 0), (read_len + 1, 0), (read_len, 5 * read_len + 3), (2 * read_len, n_bases - 2 * read_len)):
            end = min(n_bases, n_bases if n == 0 else first + n)
            want = QC.expected(counts, valid, offs, first, end, q)
            for given in (None, offs):
                got = run(exe, tmp_path, counts, valid, given, n_seqs, first, end - first if n else 0, q, read_len=read_len)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (read_len, first, n, given is None)
    # one sequence: written only by the range that holds all of it
    n_bases = 2 * QC.CHUNK + 11
    counts = rng.integers(0, 1 << 32, n_bases).astype(np.uint32)
    valid = np.ones(n_bases, np.uint8)
    offs = np.array([0, n_bases], np.uint64)
    for first, n in ((0, 0), (1, 0), (0, n_bases - 1)):
        want = QC.expected(counts, valid, offs, first, n_bases if n == 0 else first + n, q)
        got = run(exe, tmp_path, counts, valid, None, 1, first, n, q, read_len=0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (first, n)
        assert (got[1][0] == QC.GUARD) == (first != 0 or n != 0)


def test_wrong_offsets_end_clean(exe, tmp_path, batch):
    """a shuffled offsets array whose last entry is too large: the results may be anything, the run ends clean under the sanitizers
    (every array is a heap array of exactly its length)"""
    b = batch
    n_seqs = len(b["offs"]) - 1
    for seed in range(4):
        bad = QC.wrong_offsets(b["offs"], np.random.default_rng(seed))
        for first, n in ((0, 0), (4321, 20_000)):
            got = run(exe, tmp_path, b["counts"], b["valid"], bad, n_seqs, first, n, QC.QUANTILES["ends"])
            assert got[0].shape == (n_seqs, 4)


@pytest.mark.parametrize("kind", ("alternating", "sawtooth"))
def test_overlapping_long_spans_end_clean(exe, tmp_path, batch, kind):
    """wrong offsets whose passing spans overlap: the whole batch as every second span, and more long spans than the list of long
    sequences holds (the surplus is dropped).  Clean under the sanitizers, and every row is the guard or the model's answer for its span."""
    import scale_cases as S

    b, q = batch, QC.QUANTILES["ends"]
    n_seqs, n = len(b["offs"]) - 1, len(b["counts"])
    bad = S.alternating_offsets(b) if kind == "alternating" else S.sawtooth_offsets(b)
    for grid in (1, 3):
        got = run(exe, tmp_path, b["counts"], b["valid"], bad, n_seqs, 0, 0, q, grid=grid)
        written, long_written = S.check_rows_under_wrong_offsets(b, bad, 0, n, q, got[0], got[1])
        assert long_written <= S.long_cap(n, n_seqs)
