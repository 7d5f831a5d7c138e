"""CPU-only: bl_bgzf_deflate's per-wave bodies (biolib_amd/csrc/bl_deflate_core.hpp: the parse, the code build, the emitter, the gather)
emulated on the host under AddressSanitizer / UBSan (tests/emu/emu_deflate.cpp, a stand-alone program) over a text array of exactly its
length at every alignment 0..15 of its first byte and an output of exactly bl_bgzf_bound, against the Python specification
(deflate_cases.py): the bytes, the member table and the counters.  The program also inflates its own output with zlib."""
import os
import subprocess

import numpy as np
import pytest

import deflate_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
MEMBER_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("src_len", "<u4"), ("isize", "<u4"), ("crc", "<u4"), ("reserved", "<u4")])


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_deflate.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_deflate")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out, "-lz"], timeout=600)
    return out


def run(exe, tmp_path, text, eof):
    (tmp_path / "text.bin").write_bytes(text)
    p = subprocess.run([exe, str(tmp_path / "text.bin"), str(len(text)), "1" if eof else "0", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    n_out, n_members, stored, fixed, dynamic, limited, max_len, min_len, max_dist, min_dist = (int(x) for x in p.stdout.split())
    out = (tmp_path / "out.bgzf").read_bytes()
    members = np.fromfile(tmp_path / "out.members", MEMBER_DTYPE)
    assert len(out) == n_out and len(members) == n_members
    return out, members, dict(forms=[stored, fixed, dynamic], limited=limited, max_len=max_len, min_len=min_len, max_dist=max_dist, min_dist=min_dist)


@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_cases(exe, tmp_path, name):
    text, eof = DC.cases()[name]
    want, want_counters, want_table = DC.bgzf_model(text, eof)
    got, members, counters = run(exe, tmp_path, text, eof)
    assert len(got) == len(want) and got == want, (name, next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None))
    assert counters == want_counters, name
    assert [(int(m["src_off"]), int(m["dst_off"]), int(m["src_len"]), int(m["isize"]), int(m["crc"])) for m in members] == want_table, name
    assert not members["reserved"].any()
