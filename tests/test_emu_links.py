"""CPU-only: the bodies of bl_unitig_links and bl_unitigs_format_gfa (biolib_amd/csrc/bl_links_core.hpp: end keys, the end search with its
lockstep lower-bound searches, the parked words, emission; bl_gfa_core.hpp: line lengths, the wave's search, windows and pieces) emulated
on the host under AddressSanitizer / UBSan (tests/emu/emu_links.cpp) over arrays of exactly their lengths, against the Python model
(links_cases.py).  Index bugs are to be found here, not on the GPU.  The program is a stand-alone executable: nothing is preloaded."""
import os
import subprocess

import numpy as np
import pytest

import graph_cases as GC
import links_cases as LK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_links.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_links")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def run(exe, tmp_path, table, k, key_words, key_bits, option, m, rule=LK.RULES[0], sweep=False, garbage=False):
    path = tmp_path / "links.bin"
    path.write_bytes(LK.links_file(table, k, key_words, key_bits, option, m, *rule))
    r = subprocess.run([exe, str(path), str(tmp_path / "text")] + (["sweep"] if sweep else ["garbage"] if garbage else []), capture_output=True, timeout=600)
    assert r.returncode == 0 and b"FAILED" not in r.stdout, r.stdout[-2000:].decode(errors="replace") + r.stderr[-4000:].decode(errors="replace")
    out = {}
    for line in r.stdout.split(b"\n"):
        if line:
            name, _, rest = line.partition(b" ")
            out[name.decode()] = rest
    for f in (0, 1):
        p = tmp_path / ("text%d.gfa" % f)
        if p.exists():
            out["text%d" % f] = p.read_bytes()
            p.unlink()
    return out


def same(got, m, k, rule, tag):
    for f in (0, 1):
        want = LK.links(m, k, once=bool(f))
        assert np.array_equal(np.array([int(x) for x in got["links%d" % f].split()], np.uint32).reshape(-1, 2), want["array"]), (tag, f, "links")
        assert [int(x) for x in got["offsets%d" % f].split()] == want["offsets"], (tag, f, "offsets")
        assert dict(zip(LK.LINK_STAT_NAMES, (int(x) for x in got["stats%d" % f].split()))) == want["stats"], (tag, f, got["stats%d" % f], want["stats"])
        assert got["text%d" % f] == LK.GfaText(LK.gfa_lines(m, want["records"], k, *rule)).bytes(), (tag, f, "text")


@pytest.mark.parametrize("k", LK.KS)
def test_named_cases(exe, tmp_path, k):
    for c, (name, table) in enumerate(GC.cases(k)):
        m = GC.model(table, k)
        for key_words, key_bits in GC.widths(k):
            for o, option in enumerate(GC.OPTIONS):
                rule = LK.RULES[(c + o) % len(LK.RULES)]
                same(run(exe, tmp_path, table, k, key_words, key_bits, option, m, rule), m, k, rule, (name, k, key_words, option))


@pytest.mark.parametrize("name", ["all_keys", "dense_300_of_512", "dense_5000_of_8192"])
def test_dense_cases(exe, tmp_path, name):
    k, table, m = LK.dense_model(name)
    for option in (0, 6):
        same(run(exe, tmp_path, table, k, 1, 2 * k, option, m), m, k, LK.RULES[0], (name, option))


@pytest.mark.parametrize("n_forks", (0, 15, 16, 63, 64))
def test_forked_paths(exe, tmp_path, n_forks):
    """ends and records around a wave and a workgroup: 4f + 2 ends and 4f records"""
    table = LK.forked_path(n_forks)
    m = GC.model(table, 31)
    for key_words in (1, 2):
        got = run(exe, tmp_path, table, 31, key_words, 62, 1 + 3 * key_words, m, LK.RULES[2])
        same(got, m, 31, LK.RULES[2], (n_forks, key_words))
        windows, pieces = (int(x) for x in got["chunks0"].split())
        assert windows > 0 and pieces > 0, "both kinds of chunk"


def test_every_residue_of_the_boundary(exe, tmp_path):
    """one unitig with two links (a pure cycle): the sixteen prefix lengths put the place where the segment lines end and the link lines
    begin, and the text's end, at every residue mod 16"""
    table = dict(GC.cases(31))["pure_cycle"]
    m = GC.model(table, 31)
    assert len(m["strings"]) == 1
    got = run(exe, tmp_path, table, 31, 1, 62, 4, m, sweep=True)
    assert int(got["residues"]) == 0xFFFF


def test_refusals(exe, tmp_path):
    t31 = GC.path_case(5)
    m = GC.model(t31, 31)
    for k, kw, kb in ((1, 1, 62), (0, 1, 62), (2, 1, 62), (30, 1, 62), (65, 2, 128), (64, 2, 128), (33, 2, 64), (33, 1, 64), (31, 1, 60)):
        assert "refused" in run(exe, tmp_path, t31, k, kw, kb, 4, m), (k, kw, kb)
    assert run(exe, tmp_path, t31, 1, 1, 62, 4, m)["refused"] == b"5", "k = 1 by the links' own rule"


@pytest.mark.parametrize("k", (5, 31, 33))
def test_garbage_nodes_offsets_and_link_words(exe, tmp_path, k):
    """trusted for content, not for safety: unitig numbers at and above n_unitigs, any rank, offsets in any order and beyond the bases, any
    link words — no access outside the arrays' stated sizes (the sanitizers), and the text still is what gfa_byte says"""
    for name, table in list(GC.cases(k)) + ([("dense", LK.dense_model("dense_300_of_512")[1])] if k == 5 else []):
        m = GC.model(table, k)
        for key_words, key_bits in GC.widths(k):
            got = run(exe, tmp_path, table, k, key_words, key_bits, 1, m, LK.RULES[1], garbage=True)
            assert "residues" in got, name
