"""A tile of the read-tiled pass 1 that is not staged (no bad chunk: its lanes read their dwords from the batch's packed copy) is bit for
bit the tile staged in LDS, the predicate that chooses never calls a tile with a bad staged chunk clean, and nothing reads outside the
packed arrays: tests/emu/emu_direct.cpp runs the phases both ways, thread by thread on the host, under the sanitizers.  CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
# the flags of emu_selftest in tests/emu/Makefile
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter"]


def test_direct_codes_equal_staged_codes(tmp_path):
    exe = str(tmp_path / "emu_direct")
    subprocess.check_call([CXX, *FLAGS, os.path.join(EMU_DIR, "emu_direct.cpp"), "-o", exe])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr, out.stderr
    assert " 0 mismatches" in out.stdout, out.stdout
