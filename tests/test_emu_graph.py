"""CPU-only: the bodies of bl_table_adjacency and bl_table_unitigs (biolib_amd/csrc/bl_graph_core.hpp: key check, mask pass with its
lockstep lower-bound searches, link pass, pointer doubling, cycle cut, placement, emission) emulated on the host under AddressSanitizer /
UBSan (tests/emu/emu_graph.cpp) over arrays of exactly their lengths, against the Python model (graph_cases.py).  Index bugs are to be
found here, not on the GPU.  The program is a stand-alone executable: nothing is preloaded."""
import os
import subprocess

import numpy as np
import pytest

import graph_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_graph.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_graph")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def run(exe, tmp_path, table, k, key_words, key_bits, option):
    path = tmp_path / "table.bin"
    path.write_bytes(GC.table_file(table, k, key_words, key_bits, option))
    r = subprocess.run([exe, str(path)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:].decode(errors="replace") + r.stderr[-4000:].decode(errors="replace")
    out = {}
    for line in r.stdout.split(b"\n"):
        if line:
            name, _, rest = line.partition(b" ")
            out[name.decode()] = rest
    return out


def same(got, m, tag):
    assert np.array_equal(np.array([int(x, 16) for x in got["mask"].split()], np.uint8), m["mask"]), (tag, "mask")
    assert np.array_equal(np.array([int(x, 16) for x in got["links"].split()], np.uint32), m["links"]), (tag, "links")
    assert dict(zip(GC.STAT_NAMES, (int(x) for x in got["stats"].split()))) == m["stats"], (tag, got["stats"], m["stats"])
    nodes = np.array([int(x) for x in got["nodes"].split()], np.uint32).view(GC.NODE)
    assert np.array_equal(nodes, m["nodes"]), (tag, "nodes")
    assert np.array_equal(np.array([int(x) for x in got["offsets"].split()], np.uint64), m["offsets"]), (tag, "offsets")
    assert np.array_equal(np.array([int(x) for x in got["sums"].split()], np.uint64), m["sums"]), (tag, "sums")
    assert got["bases"] == m["bases"].tobytes(), (tag, "bases")
    lens = set(len(s) for s in m["strings"])
    assert int(got["rounds"].split()[2]) == (lens.pop() if len(lens) == 1 and len(m["strings"]) > 1 else 0), (tag, "fixed length only where all are")


@pytest.mark.parametrize("k", GC.KS)
def test_named_cases(exe, tmp_path, k):
    for name, table in GC.cases(k):
        m = GC.model(table, k)
        for key_words, key_bits in GC.widths(k):
            for option in GC.OPTIONS:
                same(run(exe, tmp_path, table, k, key_words, key_bits, option), m, (name, k, key_words, option))


@pytest.mark.parametrize("n_keys", GC.PATH_LENGTHS)
def test_path_lengths(exe, tmp_path, n_keys):
    table = GC.path_case(n_keys)
    m = GC.model(table, 31)
    for key_words in (1, 2):
        got = run(exe, tmp_path, table, 31, key_words, 62, 1 + 3 * key_words)
        same(got, m, (n_keys, key_words))
        assert int(got["rounds"].split()[0]) <= max(n_keys - 1, 1).bit_length() + 1, "doubling: about log2 of the longest chain"


def test_a_path_of_seventy_thousand_keys(exe, tmp_path):
    table = GC.path_case(GC.LONG_PATH)
    m = GC.model(table, 31)
    assert m["stats"]["longest_unitig"] > GC.LONG_PATH // 2
    got = run(exe, tmp_path, table, 31, 1, 62, 12)
    same(got, m, "long")
    assert int(got["rounds"].split()[0]) <= 18


def test_refusals_and_bad_keys(exe, tmp_path):
    t31 = GC.path_case(5)
    for k, kw, kb in ((0, 1, 62), (2, 1, 62), (30, 1, 62), (65, 2, 128), (64, 2, 128), (33, 2, 64), (33, 1, 64), (31, 1, 60)):
        assert "refused" in run(exe, tmp_path, t31, k, kw, kb, 4), (k, kw, kb)
    # 2^31 keys or more: refused by the same function in front of everything (the file holds the five head words only)
    import struct

    for n, refused in (((1 << 31) - 1, False), (1 << 31, True), (1 << 32, True)):
        (tmp_path / "head.bin").write_bytes(struct.pack("<5Q", 1, 62, n, 31, 4))
        r = subprocess.run([exe, str(tmp_path / "head.bin"), "check"], capture_output=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == (b"refused 4" if refused else b"accepted"), (n, r.stdout)
    keys = sorted(t31)
    # a key above its own reverse complement, and a key with a bit above 2k: the first such slot is named
    big = GC.rc(keys[2], 31)
    got = run(exe, tmp_path, {**t31, big: 1}, 31, 1, 62, 4)
    assert got == {"bad": str(sorted(keys + [big]).index(big)).encode()}
    got = run(exe, tmp_path, {3: 1, (1 << 10) | 1: 2}, 5, 1, 62, 4)
    assert got == {"bad": b"1"}
