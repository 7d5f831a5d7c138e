"""CPU-only: the four stages of the count-table algebra (biolib_amd/csrc/bl_table_ops_core.hpp: partition, count pass, scan of the tile
totals, write pass) emulated lane by lane on the host under AddressSanitizer / UBSan (tests/emu/emu_table_ops.cpp) over heap arrays of
exactly the needed lengths, against the dict model of tests/table_ops_cases.py: keys, counts, every statistics word, and the write pass's
total against the count pass's.  Index bugs are to be found here, not on the GPU."""
import os
import subprocess

import pytest

import table_ops_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
STATS = ("n_a_only", "n_b_only", "n_both", "n_out", "sum_min", "sum_max", "sum_out")


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_table_ops.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_table_ops")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def _run(exe, path):
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert len(lines) % 3 == 0
    return list(zip(lines[0::3], lines[1::3], lines[2::3]))


def test_geometry_is_read_from_the_header():
    g = TC.geometry()
    assert g["TPB"] % 64 == 0 and all(g["TILE"][w] == g["TPB"] * g["ITEMS"][w] and 2 <= g["ITEMS"][w] <= 32 for w in (1, 2))


def test_cases_cover_the_shapes_and_sit_where_they_say():
    cases = TC.cases()
    for case in cases:
        TC.check_case(case)
    for kw in (1, 2):
        mine = [c for c in cases if c["key_words"] == kw]
        for kb in TC.KEY_BITS[kw]:
            got = {c["sizes"] for c in mine if c["key_bits"] == kb and "sizes" in c}
            want = {s for s in TC.sizes(kw) if s[0] + s[1] - (min(s) // 2 if min(s) > 1 else 0) <= (1 << kb)}
            assert got == want and {(0, 0), (0, 1), (1, 0), (1, 1)} <= got, (kw, kb)
            if kb > 2:
                assert got == set(TC.sizes(kw))
            # keys 0 and 2^key_bits - 1 are present
            assert any(0 in c["a"] or 0 in (c["b"] or {}) for c in mine if c["key_bits"] == kb)
            assert any((1 << kb) - 1 in c["a"] or (1 << kb) - 1 in (c["b"] or {}) for c in mine if c["key_bits"] == kb)
        T = TC.geometry()["TILE"][kw]
        assert {T - 1, T, T + 1, 3 * T + 1, 4097 + 63} <= {sum(c["sizes"]) for c in mine if "sizes" in c}
        planted = [d for c in mine for d in c["planted"]]
        I = TC.geometry()["ITEMS"][kw]
        assert any(d % T == 0 for d in planted) and any(d % I == 0 and d % T != 0 for d in planted)
        assert any(c["same"] for c in mine) and any(c["b"] is None and not c["same"] for c in mine)
    # every op with every mode it takes, on the planted, random and counts cases at least
    for case in cases:
        if case["kind"] in ("planted", "random", "counts", "words"):
            assert set(TC.OP_MODES) <= {(op, mode) for op, mode, lo, hi in case["rules"]}, case["name"]
    counts = [c for c in cases if c["kind"] == "counts"][0]
    a, b = counts["a"], counts["b"]
    assert any(a[x] + b[x] == TC.U32 for x in a if x in b) and any(a[x] + b[x] > TC.U32 for x in a if x in b)
    assert any(a[x] < b[x] for x in a if x in b) and any(a[x] == b[x] for x in a if x in b) and any(a[x] == b[x] + 1 for x in a if x in b)
    assert any(x not in b for x in a) and 0 in a.values() and 0 in b.values()
    assert any(TC.model(a, b, op, mode, lo, hi)[0] == {} for op, mode, lo, hi in counts["rules"])


def test_model_on_a_hand_worked_pair():
    a, b = {1: 2, 5: 7, 9: 1}, {5: 3, 9: 4, 12: 6}
    assert TC.model(a, b, TC.UNION, TC.SUM)[0] == {1: 2, 5: 10, 9: 5, 12: 6}
    assert TC.model(a, b, TC.INTERSECT, TC.MIN)[0] == {5: 3, 9: 1}
    assert TC.model(a, b, TC.SUBTRACT, TC.LEFT)[0] == {1: 2}
    out, st = TC.model(a, b, TC.COUNT_SUBTRACT, TC.LEFT, 3, 9)
    assert out == {5: 4} and st == dict(n_a_only=1, n_b_only=1, n_both=2, n_out=1, sum_min=4, sum_max=2 + 7 + 4 + 6, sum_out=4)
    assert TC.merged({3: 1, 5: 1}, {3: 1, 4: 1}) == [(3, 0), (3, 1), (4, 1), (5, 0)]


@pytest.mark.parametrize("key_words", (1, 2))
def test_emulated_stages_match_the_model(exe, tmp_path, key_words):
    ran = 0
    for case in TC.cases():
        if case["key_words"] != key_words:
            continue
        path = tmp_path / "case.bin"
        path.write_bytes(TC.emu_file(case))
        results = _run(exe, path)
        assert len(results) == len(case["rules"]), case["name"]
        a = case["a"]
        b = a if case["same"] else case["b"]
        for (op, mode, lo, hi), (head, keys, counts) in zip(case["rules"], results):
            want, stats = TC.model(a, b, op, mode, lo, hi)
            assert head[0] == "stats" and head[9] == "ok", (case["name"], op, mode, head)
            assert [int(x) for x in head[1:8]] == [stats[s] for s in STATS], (case["name"], op, mode, lo, hi)
            assert int(head[8]) == stats["n_out"], (case["name"], "the write pass's total")
            assert [int(x, 16) for x in keys[1:]] == sorted(want), (case["name"], op, mode, lo, hi)
            assert [int(x) for x in counts[1:]] == [want[x] for x in sorted(want)], (case["name"], op, mode, lo, hi)
            ran += 1
    assert ran > 200


def test_emulated_capacity_check_and_refusals(exe, tmp_path):
    case = dict([c for c in TC.cases() if c["kind"] == "random"][0])
    a, b = case["a"], case["b"]
    n_union, n_both = len(set(a) | set(b)), len(set(a) & set(b))
    assert n_both < n_union
    # the limit is the number of keys a table cannot hold: a union of exactly that many is refused, the smaller intersection passes;
    # a mode the op does not take, an unknown op, an unknown mode and crossed bounds are refused before anything runs
    case["rules"] = [(TC.UNION, TC.SUM, 0, TC.U32), (TC.INTERSECT, TC.MIN, 0, TC.U32), (TC.SUBTRACT, TC.SUM, 0, TC.U32), (TC.COUNT_SUBTRACT, TC.RIGHT, 0, TC.U32),
                     (4, TC.LEFT, 0, TC.U32), (TC.UNION, 5, 0, TC.U32), (TC.UNION, TC.SUM, 3, 2)]
    path = tmp_path / "case.bin"
    path.write_bytes(TC.emu_file(case, limit=n_union))
    results = _run(exe, path)
    _, stats = TC.model(a, b, TC.UNION, TC.SUM)
    head, keys, counts = results[0]
    assert head[9] == "capacity" and [int(x) for x in head[1:8]] == [stats[s] for s in STATS] and keys == ["keys"] and counts == ["counts"]
    assert results[1][0][9] == "ok" and int(results[1][0][4]) == n_both and len(results[1][1]) == 1 + n_both
    assert [r[0][9] for r in results[2:]] == ["invalid"] * 5
    path.write_bytes(TC.emu_file(case, limit=n_union + 1))
    assert _run(exe, path)[0][0][9] == "ok"
