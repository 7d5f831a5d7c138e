"""CPU-only: the per-thread bodies of the count-table calls (biolib_amd/csrc/bl_lookup_core.hpp: prefix, index fill, the grouped search
for both key widths, the thread of the fused scan) emulated lane by lane on the host under AddressSanitizer / UBSan
(tests/emu/emu_lookup.cpp), against that program's own std::lower_bound loop, against Python dicts and — the scan — against the Python
model.  Index bugs are to be found here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import lookup_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_lookup.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_lookup")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def _run(*cmd):
    run = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return [ln.split() for ln in run.stdout.splitlines()]


def test_cases_cover_the_shapes():
    cases = LC.table_cases()
    for kw in (1, 2):
        mine = [c for c in cases if c[1] == kw]
        assert {len(c[3]) for c in mine} >= set(LC.SIZES)
        assert {64 * kw, 2} <= {c[2] for c in mine}
        assert any((1 << (64 * kw)) - 1 in c[3] for c in mine) and any(0 in c[3] for c in mine)
    for name, kw, kb, table, queries, options in cases:
        assert set(table) <= set(queries) and set(options) == {0, 1, 24, -1}
        if table:
            assert any(q not in table for q in queries), name
        if kb < 64 * kw:
            assert any(q >> kb for q in queries), name


@pytest.mark.parametrize("key_words", (1, 2))
def test_emulated_search_matches_lower_bound_and_dict(exe, tmp_path, key_words):
    for name, kw, kb, table, queries, options in LC.table_cases():
        if kw != key_words:
            continue
        path = tmp_path / "table.bin"
        path.write_bytes(LC.table_file(kw, kb, table, queries, options))
        lines = _run(exe, "table", path)
        assert len(lines) == 2 * len(options), name
        want = [table.get(q, 0) for q in queries]
        seen = set()
        for option, head, counts in zip(options, lines[0::2], lines[1::2]):
            assert head[0] == "P" and int(head[1]) == option and counts[0] == "counts"
            p = int(head[2])
            assert 0 <= p <= min(kb, 24) and (option < 0 or p == min(option, kb, 24)), (name, option, p)
            assert [int(x) for x in counts[1:]] == want, (name, option)
            seen.add(p)
        assert {0, 1, min(kb, 24)} <= seen, name


@pytest.mark.parametrize("k", LC.SCAN_KS)
def test_emulated_scan_thread_matches_model(exe, tmp_path, k):
    ranges = [str(x) for r in LC.RANGES for x in r]
    runs = 0
    for k_, canonical, drop_last, seq, offs, m, tables in LC.scan_cases((k,)):
        batch = tmp_path / "batch.bin"
        batch.write_bytes(LC.struct.pack("<QQ", len(seq), len(offs) - 1) + offs.tobytes() + seq.tobytes())
        for table in tables:
            for kw in ((1, 2) if k <= 32 else (2,)):
                # the automatic index, and a forced one that splits the k-mers' top bits (clamped to 2k for k = 1)
                for option in ((-1, 12) if (kw == 2 or k == 1) else (-1,)):
                    tf = tmp_path / "table.bin"
                    tf.write_bytes(LC.table_file(kw, 2 * k, table, [], [option]))
                    lines = _run(exe, "scan", batch, tf, k, int(canonical), int(drop_last), *ranges)
                    assert len(lines) == 3 * len(LC.RANGES)
                    for (first, n), head, counts, valid in zip(LC.RANGES, lines[0::3], lines[1::3], lines[2::3]):
                        end = len(seq) if n == 0 else first + n
                        w_counts, w_valid, d = LC.expected_scan(m, table, first, end)
                        assert [int(x) for x in head[1:]] == [first, n, d["count"], d["xor_value"], d["aux"], d["xor_hash"], d["xor_pos"]], (k, canonical, drop_last)
                        assert np.array_equal(np.array(counts[1:], np.uint32), w_counts) and np.array_equal(np.array(valid[1:], np.uint8), w_valid)
                        assert d["count"] > 0
                    runs += 1
    assert runs >= 4
