"""CPU-only: the partition step and the tile body of the merge-path intersection kernel for 16-byte keys, and the search form
(biolib_amd/csrc/bl_setops128_core.hpp), emulated lane by lane on the host under AddressSanitizer / UBSan (tests/emu/emu_setops128.cpp)
against that program's own two-finger walk and against Python sets.  Index bugs are to be found here, not on the GPU."""
import os
import struct
import subprocess

import pytest

import setops128_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_setops128.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_setops128")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def _run(exe, tmp_path, a, b, *extra):
    path = tmp_path / "sets.bin"
    path.write_bytes(struct.pack("<QQ", len(a), len(b)) + S.to_array(a).tobytes() + S.to_array(b).tobytes())
    run = subprocess.run([exe, str(path), *extra], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    w = run.stdout.split()
    assert w[0::2] == ["merge", "search", "walk"]
    return [int(x) for x in w[1::2]]


def test_cases_cover_the_shapes():
    names = [n for n, _, _ in S.cases()]
    assert len(names) == len(set(names))
    sizes = {(len(a), len(b)) for _, a, b in S.cases()}
    assert set(S.SIZES) <= sizes and (S.T + 1, S.T) in sizes and (3 * S.T + 18, 3 * S.T + 17) in sizes


def test_emulated_kernels_match_walk_and_python_sets(exe, tmp_path):
    for name, a, b in S.cases():
        exp = len(set(a) & set(b))
        assert _run(exe, tmp_path, a, b) == [exp, exp, exp], name
        assert _run(exe, tmp_path, b, a) == [exp, exp, exp], name + " swapped"


def test_inputs_with_duplicates_stay_inside_the_arrays(exe, tmp_path):
    """no count is asserted: the contract leaves it open; the sanitizers check every index"""
    for name, a, b in S.with_duplicates():
        _run(exe, tmp_path, a, b, "nocheck")
        _run(exe, tmp_path, b, a, "nocheck")
