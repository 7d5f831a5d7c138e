"""CPU-only: the bodies of bl_scan_read_edits and bl_batch_apply_edits (biolib_amd/csrc/bl_correct_core.hpp: the state pass on the scan's
tile, the run pass, the wave's test of the three alternatives, compaction, apply) emulated on the host under AddressSanitizer / UBSan
(tests/emu/emu_correct.cpp) over arrays of exactly their lengths, against the Python model (correct_cases.py).  Index bugs are to be found
here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import correct_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_correct.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_correct")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def write_inputs(tmp_path, bases, offs, table, k):
    bases = CC.as_bytes(bases)
    offs = np.ascontiguousarray(offs, np.uint64)
    with open(tmp_path / "batch.bin", "wb") as f:
        f.write(np.array([len(bases), len(offs) - 1], np.uint64).tobytes() + offs.tobytes() + bases.tobytes())
    keys, counts = CC.table_arrays(table, k)
    with open(tmp_path / "table.bin", "wb") as f:
        f.write(np.array([1 if k <= 32 else 2, 2 * k, len(counts), 0, 1], np.uint64).tobytes() + np.array([-1], np.int64).tobytes())
        f.write(keys.tobytes() + counts.astype(np.uint64).tobytes())


def run(exe, tmp_path, k, canonical, min_count, min_support, ranges, capacity=-1):
    """-> list of (stats dict, EDIT array, stored) per range, and the applied bytes"""
    cmd = [exe, tmp_path / "batch.bin", tmp_path / "table.bin", k, int(canonical), min_count, min_support, capacity] + [x for r in ranges for x in r]
    r = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out, applied = [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "range":
            out.append((dict(zip(CC.STAT_NAMES, (int(x) for x in w[3:9]))), [], int(w[9])))
        elif w[0] == "edit":
            out[-1][1].append(tuple(int(x) for x in w[1:]) + (0,))
        else:
            applied = np.frombuffer(bytes.fromhex(w[1]) if len(w) > 1 else b"", np.uint8)
    return [(s, np.array(e, dtype=CC.EDIT) if e else np.zeros(0, CC.EDIT), n) for s, e, n in out], applied


def same_edits(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (tag, int(bad[0]), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("canonical", (False, True), ids=("forward", "canonical"))
@pytest.mark.parametrize("k", CC.KS)
def test_named_cases_in_three_layouts(exe, tmp_path, k, canonical):
    c = CC.cases(k, canonical)
    for kind in CC.LAYOUTS:
        L = CC.layout(c, kind)
        write_inputs(tmp_path, L["bases"], L["offs"], c["table"], k)
        for min_support in sorted({1, min(2, k), k}):
            want, stats, _ = CC.model(L["bases"], L["offs"], k, c["table"], c["min_count"], min_support, canonical)
            (got,), applied = run(exe, tmp_path, k, canonical, c["min_count"], min_support, [(0, 0)])
            assert got[0] == stats, (kind, min_support, got[0], stats)
            same_edits(got[1], want, (kind, min_support))
            assert np.array_equal(applied, CC.apply_model(L["bases"], want)), (kind, "a repeated pos and a pos behind the batch change nothing")
        if k >= 5 and kind == "offsets":
            assert stats["n_low_support"] > 0 and stats["n_edits"] > 0 and stats["n_misfit"] > 0


def test_the_cases_meet_every_class():
    """what the named reads are for: every class, both anchors, support 1 and k (a self-check of the cases, not of the code)"""
    c = CC.cases(31, True)
    L = CC.layout(c, "offsets")
    edits, stats, detail = CC.model(L["bases"], L["offs"], 31, c["table"], c["min_count"], 1, True)
    assert all(stats[name] > 0 for name in CC.STAT_NAMES if name != "n_low_support"), stats
    assert set(edits["anchor"]) == {0, 1} and edits["support"].min() == 1 and edits["support"].max() == 31
    by_read = {}
    for q, a, b, cls in detail:
        by_read.setdefault(c["names"][q], []).append(cls)
    assert by_read["runs_k_km1_kp1"] == ["edit", "misfit", "misfit"] or by_read["runs_k_km1_kp1"].count("misfit") >= 2, by_read["runs_k_km1_kp1"]
    assert by_read["ambiguous"] == ["ambiguous"] and by_read["alt_below_min_count"] == ["no_base"] and by_read["alt_at_min_count"] == ["edit"]
    assert by_read["two_errors_km1_apart"] == ["misfit"] and by_read["two_errors_kp1_apart"] == ["edit", "edit"]
    assert by_read["length_k"] == ["misfit"] and "length_km1" not in by_read and by_read["weak_tail"] == ["edit"] and by_read["weak_head"] == ["edit"]
    lower = edits[[i for i, e in enumerate(edits) if chr(e["from"]).islower()]]
    assert len(lower) >= 2 and all(chr(t).islower() for t in lower["to"])
    assert any(chr(f) in "Uu" for f in edits["from"]) and not any(chr(t) in "Uu" for t in edits["to"])


@pytest.mark.parametrize("k,canonical", ((5, False), (31, True), (33, True)))
def test_every_cut_of_a_short_batch(exe, tmp_path, k, canonical):
    """two ranges concatenate and add up to the one-call answer: every cut of a batch of up to 700 bases (k = 5), every seventh cut and
    the three around each read boundary of a longer one (k = 31, 33); test_gpu_correct.py takes every cut at k = 5 and 15"""
    c = CC.cases(k, canonical)
    keep = [i for i, name in enumerate(c["names"]) if not name.startswith("every_base") or name.endswith(("_p0", "_p3", f"_p{k}", f"_p{k + 2}"))]
    reads = [c["reads"][i] for i in keep]
    bases = CC.as_bytes("".join(reads))
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    n = len(bases)
    cuts = range(1, n) if n <= 700 else sorted(set(range(1, n, 7)) | set(int(o) + d for o in offs[1:-1] for d in (-1, 0, 1)))
    write_inputs(tmp_path, bases, offs, c["table"], k)
    want, stats, _ = CC.model(bases, offs, k, c["table"], c["min_count"], 1, canonical)
    assert len(want) > 4
    ranges = [(0, 0)] + [r for cut in cuts for r in ((0, cut), (cut, 0))]
    got, _ = run(exe, tmp_path, k, canonical, c["min_count"], 1, ranges)
    assert got[0][0] == stats
    same_edits(got[0][1], want, "whole")
    for i, cut in enumerate(cuts):
        (s1, e1, _), (s2, e2, _) = got[1 + 2 * i], got[2 + 2 * i]
        assert {name: s1[name] + s2[name] for name in CC.STAT_NAMES} == stats, cut
        same_edits(np.concatenate([e1, e2]), want, cut)
        w1, ws1, _ = CC.model(bases, offs, k, c["table"], c["min_count"], 1, canonical, 0, cut)
        assert s1 == ws1 and len(e1) == len(w1), (cut, "the model's range rule")


def test_capacity_stops_the_stores(exe, tmp_path):
    c = CC.cases(31, False)
    L = CC.layout(c, "offsets")
    write_inputs(tmp_path, L["bases"], L["offs"], c["table"], 31)
    want, stats, _ = CC.model(L["bases"], L["offs"], 31, c["table"], c["min_count"], 1, False)
    for cap in (0, 1, len(want) - 1, len(want), len(want) + 5):
        (got,), _ = run(exe, tmp_path, 31, False, c["min_count"], 1, [(0, 0)], capacity=cap)  # (the output array holds exactly cap records)
        assert got[0] == stats and got[2] == min(cap, len(want))
        same_edits(got[1], want[:cap], cap)


def test_an_empty_table_and_a_batch_shorter_than_k(exe, tmp_path):
    c = CC.cases(5, False)
    L = CC.layout(c, "offsets")
    write_inputs(tmp_path, L["bases"], L["offs"], {}, 5)
    (got,), _ = run(exe, tmp_path, 5, False, 1, 1, [(0, 0)])
    assert got[0]["n_runs"] == got[0]["n_misfit"] > 0 and got[0]["n_edits"] == 0 and got[0] == CC.model(L["bases"], L["offs"], 5, {}, 1)[1]
    write_inputs(tmp_path, b"ACG", [0, 3], c["table"], 5)
    (got,), applied = run(exe, tmp_path, 5, False, 3, 1, [(0, 0)])
    assert got[0] == dict.fromkeys(CC.STAT_NAMES, 0) and bytes(applied) == b"ACG"
