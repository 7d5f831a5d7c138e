"""CPU-only: the bodies of bl_unitigs_mark and bl_table_remove_unitigs (biolib_amd/csrc/bl_clean_core.hpp: the chain of gathers that marks
a unitig, the 128-bit keep order, the tiles, ballots and ranks of the compaction) emulated on the host under AddressSanitizer / UBSan
(tests/emu/emu_clean.cpp) over arrays of exactly their lengths, against the Python model (clean_cases.py).  Index bugs are to be found
here, not on the GPU.  The program is a stand-alone executable: nothing is preloaded."""
import os
import subprocess

import numpy as np
import pytest

import clean_cases as CC
import graph_cases as GC
import lookup_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_clean.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_clean")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def run(exe, tmp_path, arrays, r, table=None, m=None, key_words=1, key_bits=62, mode="normal"):
    path = tmp_path / "clean.bin"
    path.write_bytes(CC.clean_file(arrays, r, table, m, key_words, key_bits))
    p = subprocess.run([exe, str(path), mode], capture_output=True, timeout=600)
    assert p.returncode == 0 and b"FAILED" not in p.stdout, p.stdout[-2000:].decode(errors="replace") + p.stderr[-4000:].decode(errors="replace")
    out = {}
    for line in p.stdout.split(b"\n"):
        if line:
            name, _, rest = line.partition(b" ")
            out[name.decode()] = rest.split()
    return out


def table_words(table, key_words):
    keys = sorted(table)
    return [int(w) for w in LC.words(keys, key_words).reshape(-1)], [table[x] for x in keys]


def same(got, arrays, r, table, m, key_words, tag, mode="normal"):
    marks, st = CC.mark_arrays(*arrays, r)
    assert [int(x) for x in got["marks"]] == marks, (tag, "marks")
    assert dict(zip(CC.STAT_NAMES, (int(x) for x in got["stats"]))) == st, (tag, got["stats"], st)
    used = [int(x) for x in got["used"]]
    assert used == ([1] * len(marks) if mode == "all" else [0] * len(marks) if mode == "none" else marks), (tag, "used")
    if table is not None:
        want_keys, want_counts = table_words(CC.remove(table, m, used), key_words)
        assert [int(x, 16) for x in got["keys"]] == want_keys and [int(x) for x in got["counts"]] == want_counts, (tag, "the table")


@pytest.mark.parametrize("k", CC.KS)
def test_every_case(exe, tmp_path, k):
    for name, table, r in CC.all_cases(k):
        m = GC.model(table, k)
        arrays = CC.arrays_of(m, k)
        for key_words, key_bits in GC.widths(k):  # (k = 31: one- and two-word keys)
            same(run(exe, tmp_path, arrays, r, table, m, key_words, key_bits), arrays, r, table, m, key_words, (name, k, key_words))


@pytest.mark.parametrize("n_unitigs", (3, 63, 64, 65, 255, 256, 257))
def test_spur_paths_across_the_tile_seams(exe, tmp_path, n_unitigs):
    """paths with planted spurs: thousands of keys, so that kept runs and dropped runs (the spurs' keys lie anywhere in key order) cross
    the seams of tiles of 64, 128 and 512 keys; and the same with every key dropped and none"""
    table = CC.spur_path(n_unitigs)
    m = GC.model(table, 31)
    assert len(m["strings"]) == n_unitigs
    arrays, r = CC.arrays_of(m, 31), CC.default_rule(31)
    assert CC.mark_arrays(*arrays, r)[1]["n_tips"] == (n_unitigs - 1) // 2
    for key_words in (1, 2):
        for mode in ("normal", "all", "none"):
            got = run(exe, tmp_path, arrays, r, table, m, key_words, 62, mode)
            same(got, arrays, r, table, m, key_words, (n_unitigs, key_words, mode), mode)
            if mode == "all":
                assert got["keys"] == [] and got["counts"] == []


@pytest.mark.parametrize("n_keys", (63, 64, 65, 127, 128, 129, 511, 512, 513, 1024, 1025))
def test_key_counts_around_every_tile_size(exe, tmp_path, n_keys):
    """a path of exactly n_keys keys cut into unitigs of 1 .. 7 keys by hand (nodes, offsets and marks need no graph): every second unitig
    marked, so that a marked run lies across every seam"""
    table = GC.path_case(n_keys)
    keys = sorted(table)
    rng = np.random.default_rng(n_keys)
    nodes, u = np.zeros(n_keys, GC.NODE), 0
    i = 0
    while i < n_keys:
        run_len = int(rng.integers(1, 8))
        nodes["unitig"][i:i + run_len] = u
        i, u = i + run_len, u + 1
    m = dict(keys=keys, nodes=nodes)
    # an array set whose islands are marked alternately: unitig v is one key long where v is even (an island that goes), 99 where odd
    offsets, links, link_offsets = [0], [], [0] * (2 * u + 1)
    for v in range(u):
        offsets.append(offsets[-1] + (1 if v % 2 == 0 else 99) + 30)
    arrays, r = (offsets, [1] * u, link_offsets, links), CC.rule(31, isolated=1)
    for key_words in (1, 2):
        got = run(exe, tmp_path, arrays, r, table, m, key_words, 62)
        assert [int(x) for x in got["marks"]] == [CC.ISLAND if v % 2 == 0 else CC.KEEP for v in range(u)]
        same(got, arrays, r, table, m, key_words, (n_keys, key_words))


@pytest.mark.parametrize("seed", range(4))
def test_products_beyond_64_bits(exe, tmp_path, seed):
    for make in (CC.synthetic_tips, CC.synthetic_bubble):
        offsets, sums, link_offsets, links, r = make(seed)
        arrays = (offsets, sums, link_offsets, links)
        same(run(exe, tmp_path, arrays, r), arrays, r, None, None, 1, (make.__name__, seed))


def test_refusals(exe, tmp_path):
    arrays = ([0, 31], [1], [0, 0, 0], [])
    for k in (0, 1, 2, 30, 64, 65):
        assert "refused" in run(exe, tmp_path, arrays, CC.rule(k, tips=3)), k
    assert run(exe, tmp_path, arrays, dict(CC.rule(31), flags=8))["refused"] == [b"2"]
    assert "marks" in run(exe, tmp_path, arrays, CC.rule(31, tips=3))


@pytest.mark.parametrize("k", CC.KS)
def test_garbage_link_offsets_link_words_nodes_and_marks(exe, tmp_path, k):
    """trusted for content, not for safety: link offsets beyond the records and out of order, `to` words at and beyond the ends, unitig
    numbers at and above n_unitigs, any mark bytes — no access outside the arrays' stated sizes (the sanitizers), and the marks and the
    kept keys are still what the model says of those arrays.  Every case of test_every_case again: every k, every rule set (each rule
    alone, so the branches of a flag that is off run on such arrays too, and all together), both key widths"""
    for name, table, r in CC.all_cases(k):
        m = GC.model(table, k)
        offsets, sums, _, records = CC.arrays_of(m, k)
        for key_words, key_bits in GC.widths(k):
            got = run(exe, tmp_path, (offsets, sums, [0] * (2 * len(sums) + 1), records), r, table, m, key_words, key_bits, "garbage")
            link_offsets = [int(x) for x in got["g_link_offsets"]]
            words = [int(x) for x in got["g_links"]]
            links = list(zip(words[0::2], words[1::2]))
            marks, st = CC.mark_arrays(offsets, sums, link_offsets, links, r)
            assert [int(x) for x in got["marks"]] == marks, (name, key_words)
            assert dict(zip(CC.STAT_NAMES, (int(x) for x in got["stats"]))) == st, name
            used = [int(x) for x in got["used"]]
            g_nodes = np.zeros(len(table), GC.NODE)
            g_nodes["unitig"] = [int(x) for x in got["g_nodes"]]
            want_keys, want_counts = table_words(CC.remove(table, dict(keys=m["keys"], nodes=g_nodes), used), key_words)
            assert [int(x, 16) for x in got["keys"]] == want_keys and [int(x) for x in got["counts"]] == want_counts, (name, key_words)
