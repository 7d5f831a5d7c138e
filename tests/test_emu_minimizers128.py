"""CPU-only: the per-thread bodies of bl_scan_minimizers128 (biolib_amd/csrc/bl_minimizers128_core.hpp) emulated on the host under
AddressSanitizer / UBSan (tests/emu/emu_minimizers128.cpp): a workgroup's phases lane by lane with host arrays for LDS, against that
program's own `unsigned __int128` evaluation of the rule and against the Python model's count and digest words.  Index bugs are to be
found here, not on the GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import minimizers128_model as M
from range_cases import batch128

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SEED, ORIGIN = 0x9E3779B9, 1_000_000_007  # fixed in emu_minimizers128.cpp
H = 4096  # window starts per tile
# (unit, w): w = 1, 2, 15, 16, 17, 33, 63, 64 — both window forms, their threshold, the largest halo; and one ordinary shape
SHAPES = ((33, 1), (64, 2), (48, 15), (33, 16), (51, 17), (64, 33), (40, 63), (64, 64), (17, 11))


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_minimizers128.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_minimizers128")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


make_batch = batch128  # (shared with the range sweep: tests/range_cases.py)


@pytest.mark.parametrize("unit,w", SHAPES)
def test_emulated_workgroup_matches_plain_rule_and_model(exe, tmp_path, unit, w):
    rng = np.random.default_rng(3000 + 64 * unit + w)
    seq, offs = make_batch(unit, rng)
    path = tmp_path / "batch.bin"
    path.write_bytes(struct.pack("<QQ", len(seq), len(offs) - 1) + offs.tobytes() + seq.tobytes())
    models = {(c, d): M.scan(seq.tobytes(), offs, unit, w, SEED, c, d, 16) for c in (False, True) for d in (False, True)}
    for first, n in ((0, 0), (37, 8200)):  # the whole batch; a range that is not 16-aligned and ends inside a tile
        run = subprocess.run([exe, str(path), str(unit), str(w), str(first), str(n)], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        lines = [ln.split() for ln in run.stdout.splitlines()]
        assert len(lines) == 4 and all(ln[0] == "min" for ln in lines)
        end = len(seq) if n == 0 else first + n
        for ln in lines:
            canon, drop = bool(int(ln[1])), bool(int(ln[2]))
            want = M.minimizers(models[canon, drop], first, end, ORIGIN)
            assert [int(x) for x in ln[3:8]] == [want[key] for key in ("count", "xor_value", "aux", "xor_hash", "xor_pos")], (unit, w, first, ln[:3])
            assert want["count"] > 0
