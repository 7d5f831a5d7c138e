"""CPU-only: the per-thread bodies of the 128-bit k-mer scans (biolib_amd/csrc/bl_kmers128_core.hpp) emulated lane by lane on the host
under AddressSanitizer / UBSan (tests/emu/emu_kmers128.cpp), against that program's own `unsigned __int128` loop and against the
Python model's digests.  Index bugs are to be found here, not on the GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import kmers128_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SEED, ORIGIN = 0x9E3779B9, 1_000_000_007  # fixed in emu_kmers128.cpp
H = 4096  # positions per tile
KS = (1, 16, 17, 32, 33, 47, 48, 49, 63, 64)


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_kmers128.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_kmers128")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def make_batch(k, rng):
    """two tiles and a ragged end; reads of length k-1, k, k+1 (and 1, 150); breaks at the first and the last base of a tile; bytes >= 0x80"""
    n = 2 * H + 1007
    seq = rng.choice(np.frombuffer(b"ACGTacgtUu", np.uint8), n)
    lens = [k + 1, k, max(k - 1, 1), 1, 150]
    offs = [0]
    for length in lens:
        offs.append(offs[-1] + length)
    offs += [H - 3, H + k, 2 * H - 1, 2 * H + 500, n]
    offs = np.array(sorted(set(offs)), np.uint64)
    seq[[H, 2 * H - 1, 2 * H, 3000, 3001, n - 1 - 2 * k]] = ord("N")  # tile 1's first and last base, tile 2's first
    seq[5000] = 0x80
    seq[5200] = 0xFF
    return seq, offs


@pytest.mark.parametrize("k", KS)
def test_emulated_threads_match_plain_loop_and_model(exe, tmp_path, k):
    rng = np.random.default_rng(1000 + k)
    seq, offs = make_batch(k, rng)
    path = tmp_path / "batch.bin"
    path.write_bytes(struct.pack("<QQ", len(seq), len(offs) - 1) + offs.tobytes() + seq.tobytes())
    threshold = 1 << 62
    for first, n in ((0, 0), (37, 8200)):  # the whole batch; a range that is not 16-aligned and ends inside a tile
        run = subprocess.run([exe, str(path), str(k), str(first), str(n), str(threshold)], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        lines = [ln.split() for ln in run.stdout.splitlines()]
        assert len(lines) == 8
        end = len(seq) if n == 0 else first + n
        for ln in lines:
            canon, drop = bool(int(ln[1])), bool(int(ln[2]))
            got = [int(x) for x in ln[3:]]
            m = M.scan(seq.tobytes(), offs, k, SEED, canon, drop)
            if ln[0] == "dense":
                d = M.digest(m, first, end)
                assert got == [d["count"], d["xor_value"], d["aux"], d["xor_hash"], d["sum_hash"]], (k, first, ln[:3])
                assert d["count"] > 0
            else:
                s = M.sample(m, threshold, first, end, ORIGIN)
                assert got == [s["count"], s["xor_value"], s["aux"], s["xor_hash"], s["xor_pos"]], (k, first, ln[:3])
