"""CPU-only: the bodies of bl_text_index_build and bl_batch_format (biolib_amd/csrc/bl_format_core.hpp: the index rows, the record
lengths, the write with its wave search, window path and run-by-run assembly) emulated on the host under AddressSanitizer / UBSan
(tests/emu/emu_format.cpp) over arrays of exactly their lengths — text, bases, offsets, records and an output of exactly n_bytes —
against the Python specification (format_cases.py).  Index bugs are to be found here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import format_cases as FC
import parse_cases as PC
from test_format_model import round_trip_texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_format.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_format")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def run_index(exe, tmp_path, text):
    (tmp_path / "text.bin").write_bytes(text)
    r = subprocess.run([exe, "index", str(tmp_path / "text.bin"), str(len(text)), str(tmp_path / "ix")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    n, fastq = (int(x) for x in r.stdout.split())
    return np.fromfile(tmp_path / "ix.records", FC.RECORD_DTYPE), np.fromfile(tmp_path / "ix.offsets", np.uint64), bool(fastq), n


def run_format(exe, tmp_path, c, capacity=None, index=None):
    """the emulated call on case c -> (text or None at a capacity refusal, n_bytes, n_records, paths, chunks)"""
    text = c["text"] or b""
    records, ioffs, fastq = index if index is not None else FC.index_model(text)
    files = dict(bases=c["bases"], offsets=c["offsets"], text=np.frombuffer(text, np.uint8) if text else None, records=records if text else None,
                 ioffsets=ioffs if text else None, source=c["source_index"], spans=c["spans"], tags=c["tags"])
    args = []
    for name, arr in files.items():
        if arr is None:
            args.append("-")
        else:
            (tmp_path / (name + ".bin")).write_bytes(np.ascontiguousarray(arr).tobytes())
            args.append(tmp_path / (name + ".bin"))
    r = c["rule"]
    flags = (1 if r["skip_empty"] else 0) | (2 if r["tag_length"] else 0)
    args += [len(c["bases"]), len(c["offsets"]) - 1, 0, len(text), len(records) if text else 0, 0 if c["spans"] is None else len(c["spans"]), 1 if fastq else 0,
             1 if r["fmt"] == "fastq" else 0, flags, r["line_width"], r["quality_fill"], r["prefix"].hex() or "-", r["label"].hex() or "-", r["first_number"],
             FC.U64 if capacity is None else capacity, tmp_path / "out.bin"]
    if (tmp_path / "out.bin").exists():
        os.unlink(tmp_path / "out.bin")
    p = subprocess.run([exe, "format"] + [str(x) for x in args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    words = p.stdout.split()
    if words[0] == "capacity":
        assert not (tmp_path / "out.bin").exists()
        return None, int(words[1]), int(words[2]), None, None
    n_bytes, n_records, reg, mem, window, pieces = (int(x) for x in words)
    out = (tmp_path / "out.bin").read_bytes()
    assert len(out) == n_bytes
    return out, n_bytes, n_records, (reg, mem), (window, pieces)


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_cases(exe, tmp_path, name):
    c = FC.cases()[name]
    want, want_records = FC.format_model(c)
    got, n_bytes, n_records, paths, chunks = run_format(exe, tmp_path, c)
    assert (n_bytes, n_records) == (len(want), want_records), name
    assert got == want, (name, next(i for i in range(len(want)) if got[i] != want[i]))
    assert paths == FC.wave_paths(FC.record_offsets(c)), (name, "register waves, memory waves")
    if name in ("many_tiny", "many_tiny_generated"):
        assert paths[1] >= 1, "more than 64 records begin inside a wave: looked up in memory"
    if name in ("lengths", "lengths_generated", "alignments"):
        assert paths[0] >= 1 and chunks[0] > 0 and chunks[1] > 0, "waves that keep their records in registers; chunks of both kinds"


def test_both_lookups_and_both_chunk_paths_are_taken(exe, tmp_path):
    reg = mem = window = pieces = 0
    for name in ("lengths", "many_tiny", "alignments_trimmed", "line_width_60"):
        _, _, _, p, ch = run_format(exe, tmp_path, FC.cases()[name])
        reg, mem, window, pieces = reg + p[0], mem + p[1], window + ch[0], pieces + ch[1]
    assert reg > 0 and mem > 0 and window > 0 and pieces > 0, (reg, mem, window, pieces)


def test_capacity_refusal(exe, tmp_path):
    for name in ("one_base", "lengths", "spans_keep_empty"):
        c = FC.cases()[name]
        want, want_records = FC.format_model(c)
        assert run_format(exe, tmp_path, c, capacity=len(want) - 1)[:3] == (None, len(want), want_records)
        assert run_format(exe, tmp_path, c, capacity=0)[:3] == (None, len(want), want_records)
        assert run_format(exe, tmp_path, c, capacity=len(want))[0] == want


@pytest.mark.parametrize("name", sorted(n for n, c in FC.cases().items() if c["text"]))
def test_index_rows(exe, tmp_path, name):
    """index_line over the parser's line arrays gives the model's records and offsets, and the writer on them the model's text"""
    c = FC.cases()[name]
    records, offs, fastq, n = run_index(exe, tmp_path, c["text"])
    want_records, want_offs, want_fastq = FC.index_model(c["text"])
    assert n == len(want_records) and fastq == want_fastq, name
    assert np.array_equal(records, want_records) and np.array_equal(offs, want_offs), name
    assert run_format(exe, tmp_path, c, index=(records, offs, fastq))[0] == FC.format_model(c)[0], name


def test_round_trip_of_the_parsers_texts(exe, tmp_path):
    """index -> format gives an LF-terminated FASTQ text and a uniformly wrapped FASTA text back byte for byte"""
    for name, width in round_trip_texts().items():
        text = PC.CASES[name]
        c = FC.case(text, fmt="fastq" if text[:1] == b"@" else "fasta", line_width=width)
        index = run_index(exe, tmp_path, text)[:3]
        assert run_format(exe, tmp_path, c, index=index)[0] == text, name


def test_every_alignment_of_a_short_record(exe, tmp_path):
    """one indexed FASTQ record behind a first one of every length mod 16: name, sequence, quality and output start at every alignment,
    arrays exactly as long as their contents"""
    for pad in range(16):
        for L in (0, 1, 15, 16, 17, 35):
            text = FC.fastq_text([FC.name(pad, pad), FC.name(5, L)], [FC.dna(3, pad), FC.dna(L, L)])
            c = FC.case(text)
            assert run_format(exe, tmp_path, c)[0] == text, (pad, L)
            c = FC.case(text[:-1], fmt="fasta", tag_length=True)  # the text's last byte is the last quality byte
            assert run_format(exe, tmp_path, c)[0] == FC.format_model(c)[0], (pad, L)


def test_garbage_arrays_end_clean(exe, tmp_path):
    """shuffled, out-of-range offsets, a random source index and random spans: the result is whatever the clamping rules make of them —
    the model applies the same rules — and the run ends clean under the sanitizers"""
    base = FC.cases()["alignments"]
    n = len(base["offsets"]) - 1
    for seed in range(4):
        rng = np.random.default_rng(seed)
        offs = base["offsets"].copy()
        rng.shuffle(offs[1:-1])
        offs[rng.integers(1, n, 3)] = [FC.U64, len(base["bases"]) + 1, 0]
        source = rng.integers(0, 2 * n, n).astype(np.uint64)
        source[rng.integers(0, n, 2)] = [FC.U64, 2**63]
        spans = rng.integers(0, 80, (n, 2)).astype(np.uint64)
        spans[rng.integers(0, n, 3), 0] = [FC.U64, 2**63, len(base["text"])]
        for c in (dict(base, offsets=offs), dict(base, source_index=source), dict(base, spans=spans), dict(base, offsets=offs, source_index=source, spans=spans)):
            got = run_format(exe, tmp_path, c)
            assert got[0] == FC.format_model(c)[0], seed
