#!/usr/bin/env python3
"""Writes tests/golden/spill128/: the bytes the REFERENCE writes for a list of 128-bit k-mers.

    python tests/golden/make_spill128_golden.py PROGRAM

  keys.npy              canonical 41-mers of a synthetic sequence with two breaks (tests/kmers128_model.py), uint64[n, 2] (low, high),
                        in position order: unsorted, and a repeated stretch gives duplicates
  tmp.run_first_0.bin   the run file emem::external_memory_vector<__uint128_t>(1 << 30, dir, "first") leaves after those keys were
                        pushed and minimize() was called: the sorted keys, raw 16-byte little-endian elements
  vector.bin            io::basic_store of the std::vector<__uint128_t> holding the sorted keys: size_t count, then the elements

PROGRAM is a throwaway driver built against the reference's headers with the dialect its own CMake build selects (gnu++17, where
std::is_fundamental<__uint128_t> holds), outside the repository and never committed.  It is called as
    PROGRAM keys.raw tmp_dir out_run out_vector
reads raw 16-byte keys from keys.raw, pushes them into that vector, copies the run file to out_run while the vector is alive, checks
that iterating the vector yields every key in ascending order, and stores the sorted keys to out_vector.
This script holds none of the reference's text; it checks the two files against numpy's idea of the sorted keys before it keeps them."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmers128_model as M  # noqa: E402

OUT = os.path.join(HERE, "spill128")
K = 41


def make_keys():
    rng = np.random.default_rng(4141)
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), 2600)
    s[700] = ord("N")
    s[1903] = ord("n")
    s = np.concatenate([s, s[100:600]])  # a repeated stretch: 460 k-mers occur twice
    m = M.scan(s.tobytes(), np.array([0, len(s)], np.uint64), K, 0, True, False)
    idx = np.nonzero(m["valid"])[0]
    return np.stack([m["lo"][idx], m["hi"][idx]], axis=1).astype(np.uint64)


def sorted_keys(keys):
    return keys[np.lexsort((keys[:, 0], keys[:, 1]))]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    os.makedirs(OUT, exist_ok=True)
    keys = make_keys()
    exp = sorted_keys(keys)
    assert len(np.unique(keys, axis=0)) < len(keys) and not np.array_equal(keys, exp)
    with tempfile.TemporaryDirectory() as d:
        raw = os.path.join(d, "keys.raw")
        keys.tofile(raw)
        run, vec = os.path.join(d, "run.bin"), os.path.join(d, "vector.bin")
        os.mkdir(os.path.join(d, "tmp"))
        subprocess.run([sys.argv[1], raw, os.path.join(d, "tmp"), run, vec], check=True)
        run_bytes, vec_bytes = open(run, "rb").read(), open(vec, "rb").read()
    assert run_bytes == exp.tobytes(), "the reference's run file is not the sorted keys as raw 16-byte elements"
    assert vec_bytes == np.uint64(len(keys)).tobytes() + exp.tobytes(), "the reference's stored vector is not count + raw elements"
    np.save(os.path.join(OUT, "keys.npy"), keys)
    open(os.path.join(OUT, "tmp.run_first_0.bin"), "wb").write(run_bytes)
    open(os.path.join(OUT, "vector.bin"), "wb").write(vec_bytes)
    print("keys", len(keys), "run bytes", len(run_bytes), "vector bytes", len(vec_bytes))


if __name__ == "__main__":
    main()
