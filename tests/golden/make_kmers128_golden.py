"""Writes tests/golden/kmers128.json: fixtures of the 128-bit k-mer scans (bl_scan_kmers128, kmer_view<__uint128_t>).

Run where the reference has been built (oracle/_ref/libbiolib_ref.so, `make -C oracle ref`):
    python tests/golden/make_kmers128_golden.py [path of a program that prints the reference's forward k-mers]

  hash_kats   [lo, hi, seed, hash] from the LIVE reference hash::hash64::hash<__uint128_t> (ref_hash64_u128)
  string      200 bases with two breaks
  scans       the model's (tests/kmers128_model.py) k-mers of the string at k = 33, 48, 64, forward and canonical, hash seed 42
  items       what iterating wrapper::kmer_view<__uint128_t> over the string yields under the reference's protocol
              (kmer_view.hpp:172-202): [position, id, lo, hi] or [position, id, null, null] for a break, in loop order
              (`it != cend()` stops before the last k-mer, quirk Q1), and `last`: the item still readable after the loop
  reference_forward_checked / reference_forward_note
              the optional argument is a throwaway program (built outside the repository, never committed) that iterates the
              reference's own kmer_view<__uint128_t>, non-canonical, and prints "position lo hi" per k-mer, the last one included;
              its forward values are compared with the model's here and the outcome recorded
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmers128_model as M  # noqa: E402
import oracle_lib as O  # noqa: E402

KS = (33, 48, 64)
SEED = 42


def protocol_items(seq, k, m):
    """the reference's iteration protocol over one view: m = the model's dense scan (drop_last False) of the string"""
    n = len(seq)
    good = [c in M.CODE for c in seq]
    consumed = run = 0
    ident = 0

    def find_first():
        nonlocal consumed, run
        while consumed != n and run < k:
            run = run + 1 if good[consumed] else 0
            consumed += 1
        if run < k:  # the reference would step past the end here (Q2): the fixture avoids it
            raise AssertionError("fixture triggers Q2")

    def item():
        p = consumed - k
        if run == 0:
            return [p, ident, None, None]
        assert m["valid"][p]
        return [p, ident, int(m["lo"][p]), int(m["hi"][p])]

    items = []
    find_first()
    while consumed != n:
        items.append(item())
        ident += 1
        if run == 0:
            find_first()
        else:
            run = run + 1 if good[consumed] else 0
            consumed += 1
    return items, item()


def main():
    ref = O.ref()
    assert ref is not None, "build the reference first: make -C oracle ref"
    rng = np.random.default_rng(128)
    ones = (1 << 64) - 1
    kats = []
    keys = [(0, 0), (1, 0), (0, 1), (ones, 0), (0, ones), (ones, ones), (0x0123456789ABCDEF, 0xFEDCBA9876543210)]
    keys += [(int(rng.integers(0, ones, dtype=np.uint64)), int(rng.integers(0, ones, dtype=np.uint64))) for _ in range(41)]
    seeds = [0, 1, 42, 0xFFFFFFFF, 1 << 32, (1 << 32) + 42, ones]  # seeds >= 2^32: only their low 32 bits count
    for i, (lo, hi) in enumerate(keys):
        for seed in (seeds if i < 7 else [seeds[i % len(seeds)]]):
            kats.append([lo, hi, seed, int(ref.ref_hash64_u128(lo, hi, seed))])
    assert len(kats) >= 64
    # truncation shows: seed and seed + 2^32 give the same hash
    assert ref.ref_hash64_u128(5, 6, 42) == ref.ref_hash64_u128(5, 6, (1 << 32) + 42)

    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), 200)
    s[66] = ord("N")
    s[70] = ord("n")
    string = s.tobytes()
    offs = np.array([0, len(string)], np.uint64)
    scans, items = {}, {}
    for k in KS:
        scans[str(k)], items[str(k)] = {}, {}
        for name, canon in (("forward", False), ("canonical", True)):
            m = M.scan(string, offs, k, SEED, canon, False)
            idx = np.nonzero(m["valid"])[0]
            scans[str(k)][name] = dict(positions=[int(i) for i in idx], lo=[int(x) for x in m["lo"][idx]], hi=[int(x) for x in m["hi"][idx]],
                                       hashes=[int(x) for x in m["hashes"][idx]])
            loop, last = protocol_items(string, k, m)
            items[str(k)][name] = dict(loop=loop, last=last)
    # the protocol function against the live reference where the reference is defined (k <= 32, either strand)
    for canon in (False, True):
        m = M.scan(string, offs, 31, SEED, canon, False)
        loop, last = protocol_items(string, 31, m)
        want = O.kmer_items(string, 31, canon, False, lib=ref)
        assert [(p, i, lo) for p, i, lo, _ in loop] == want, "protocol model differs from the reference at k = 31"

    checked, note = False, "no reference program given"
    if len(sys.argv) > 1:
        bad = []
        for k in KS:
            out = subprocess.run([sys.argv[1], string.decode(), str(k)], capture_output=True, text=True, check=True).stdout
            got = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
            f = scans[str(k)]["forward"]
            if got != list(zip(f["positions"], f["lo"], f["hi"])):
                bad.append(k)
        checked = not bad
        note = ("forward k-mers of the reference's kmer_view<__uint128_t> (non-canonical, last k-mer included) equal the model's at k = 33, 48, 64"
                if checked else f"the reference's forward k-mers DIFFER from the model's at k = {bad}; the model's contract stands")
    out = dict(hash_kats=kats, string=string.decode(), seed=SEED, scans=scans, items=items, reference_forward_checked=checked, reference_forward_note=note)
    with open(os.path.join(HERE, "kmers128.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote kmers128.json:", len(kats), "hash KATs;", note)


if __name__ == "__main__":
    main()
