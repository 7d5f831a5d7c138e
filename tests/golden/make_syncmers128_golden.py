"""Writes tests/golden/syncmers128.json: fixtures of bl_scan_syncmers128 (syncmer_sampler over kmer_view<__uint128_t>).

    python tests/golden/make_syncmers128_golden.py [path of a program that runs the reference's sampler and extractor]

  strings     s200: the 200-base string with two breaks of kmers128.json; s600: 600 bases, no break
  seed        0, the seed the reference's extractor hashes with (kmer_view.hpp:272)
  cases       cases[string][k,s][forward|canonical], all from the model (tests/syncmers128_model.py, 16-byte keys):
                positions, offsets   every k-mer of the string and its extractor offset
                closed, open         the syncmer positions at start/end offsets {0, W-1} and {2, 5} (every k-mer, the last included)
  reference_forward_checked / reference_forward_note
              the optional argument is a throwaway program (built outside the repository from the reference's headers, never
              committed): `prog string k s start_offset end_offset` runs minimizer_position_extractor and syncmer_sampler over the
              reference's kmer_view<__uint128_t>, non-canonical, and prints "position offset" per k-mer (the last one included) and
              "count n", the number of elements the sampler yields (it stops before the last k-mer: quirk Q1).  Both are compared
              with the model's forward results here and the outcome recorded.  On the forward strand the reference wins: a
              difference is a mistake in the rule, to be fixed there.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import syncmers128_model as M  # noqa: E402

SHAPES = ((33, 11), (48, 17), (64, 32), (64, 1))
SEED = 0


def offset_sets(k, s):
    w = k - s + 1
    return dict(closed=(0, w - 1), open=(2, 5))


def main():
    with open(os.path.join(HERE, "kmers128.json")) as f:
        s200 = json.load(f)["string"]
    s600 = np.random.default_rng(600).choice(np.frombuffer(b"ACGT", np.uint8), 600).tobytes().decode()
    strings = dict(s200=s200, s600=s600)
    cases, bad, compared = {}, [], 0
    for name, text in strings.items():
        cases[name] = {}
        offs = np.array([0, len(text)], np.uint64)
        for k, s in SHAPES:
            entry = cases[name][f"{k},{s}"] = {}
            for strand, canon in (("forward", False), ("canonical", True)):
                m = M.scan(text.encode(), offs, k, s, SEED, canon, False, 16)
                idx = np.nonzero(m["valid"])[0]
                e = dict(positions=[int(i) for i in idx], offsets=[int(x) for x in m["offset"][idx]])
                for key, (a, b) in offset_sets(k, s).items():
                    e[key] = dict(offsets=[a, b], positions=[int(p) for p in M.syncmers(m, a, b)["positions"]])
                entry[strand] = e
                # the strided evaluation against the rule, word for word, on every k-mer
                for p, o in zip(e["positions"], e["offsets"]):
                    v = int(m["lo"][p]) | (int(m["hi"][p]) << 64)
                    assert M.extractor_offset(v, k, s, SEED, 16)[0] == o, (name, k, s, strand, p)
            if len(sys.argv) > 1:
                f = entry["forward"]
                last = len(text) - k  # the sampler's range stops before it (Q1)
                for key, (a, b) in offset_sets(k, s).items():
                    out = subprocess.run([sys.argv[1], text, str(k), str(s), str(a), str(b)], capture_output=True, text=True, check=True).stdout.split("\n")
                    got = [tuple(int(x) for x in ln.split()) for ln in out if ln and not ln.startswith("count")]
                    cnt = [int(ln.split()[1]) for ln in out if ln.startswith("count")][0]
                    compared += 1
                    if got != list(zip(f["positions"], f["offsets"])) or cnt != len([p for p in f[key]["positions"] if p != last]):
                        bad.append((name, k, s, key))
    checked = compared > 0 and not bad
    if compared == 0:
        note = "no reference program given"
    elif checked:
        note = ("offsets of the reference's minimizer_position_extractor over kmer_view<__uint128_t> (non-canonical, last k-mer included) and the element "
                "counts of its syncmer_sampler equal the model's on both strings at (k, s) = (33,11), (48,17), (64,32), (64,1), closed and open offsets")
    else:
        note = f"the reference DIFFERS from the model at {bad}: fix the rule"
    out = dict(strings=strings, seed=SEED, cases=cases, reference_forward_checked=checked, reference_forward_note=note)
    with open(os.path.join(HERE, "syncmers128.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote syncmers128.json;", note)


if __name__ == "__main__":
    main()
