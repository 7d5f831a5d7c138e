"""Staging a tile from a batch's packed copy (2-bit codes + one bad bit per 16-base chunk) is bit for bit staging it from the ASCII
bases: tests/emu/emu_packed.cpp runs phase_load_frl and phase_load both ways, thread by thread on the host, under the sanitizers.
CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
# the flags of emu_selftest in tests/emu/Makefile
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter"]


def test_packed_staging_equals_ascii_staging(tmp_path):
    exe = str(tmp_path / "emu_packed")
    subprocess.check_call([CXX, *FLAGS, os.path.join(EMU_DIR, "emu_packed.cpp"), "-o", exe])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr, out.stderr
    assert " 0 mismatches" in out.stdout, out.stdout
