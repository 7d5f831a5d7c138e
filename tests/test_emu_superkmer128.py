"""CPU-only: the per-thread bodies of the 32-byte super-k-mer record and the counter's table (biolib_amd/csrc/bl_superkmer128_core.hpp)
emulated on the host under AddressSanitizer / UBSan (tests/emu/emu_superkmer128.cpp): pack, expand, k-mer and minimizer extraction and
the slot protocol of one wave with a host array as LDS, against that program's own `unsigned __int128` evaluation and against the
Python model (tests/superkmer128_model.py).  Index bugs are to be found here, not on the GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import superkmer128_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SEED = 0x9E3779B9  # fixed in emu_superkmer128.cpp
SHAPES = ((33, 32), (64, 6), (64, 32), (48, 17), (63, 4), (40, 9), (31, 15))
EDGE_BASES = (1, 32, 33, 64, 65, 96, 97, 122)  # each word boundary of the record


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_superkmer128.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_superkmer128")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


def _hash64(v, seed):
    return int(O.hash64_np(np.array([v], np.uint64), seed)[0])


def run_count(exe, tmp_path, recs, k, m, canonical):
    recs = np.ascontiguousarray(recs, np.uint64).reshape(-1, 4)
    path = tmp_path / "recs.bin"
    path.write_bytes(struct.pack("<Q", len(recs)) + recs.tobytes())
    run = subprocess.run([exe, "count", str(path), str(k), str(m), str(int(canonical))], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = dict(kmers={})
    for ln in run.stdout.splitlines():
        f = ln.split()
        if f[0] == "expand":
            out["n_kmers"], out["xor"] = int(f[1]), int(f[2]) | (int(f[3]) << 64)
        elif f[0] == "minhash":
            out["minhash"] = int(f[1])
        elif f[0] == "path":
            out["path"] = f[1]
        elif f[0] == "rounds":
            out["rounds"] = [int(x) for x in f[1:]]
        elif f[0] == "kmer":
            key = int(f[1]) | (int(f[2]) << 64)
            assert key not in out["kmers"], "one k-mer in two slots"
            out["kmers"][key] = int(f[3])
    return out


def check_against_model(got, recs, k, m, canonical):
    want = M.expand(recs, k, canonical)
    x = 0
    for v in want:
        x ^= v
    assert got["n_kmers"] == len(want) and got["xor"] == x
    mh = 0
    for rec in recs:
        mh ^= _hash64(M.minimizer_of(rec, k, m, canonical), SEED)
    assert got["minhash"] == mh
    fate = M.bucket_fate(recs, k, canonical)
    assert got["path"] == fate["path"]
    if fate["path"] == "table":
        assert got["rounds"] == fate["rounds"]
        assert got["kmers"] == M.expected_counts(recs, k, canonical)
    return fate


def edge_records(k, rng):
    strings = ["".join("ACGT"[c] for c in rng.integers(0, 4, b)) for b in EDGE_BASES if k <= b <= k + 63]
    return M.records_from_bases(strings, k, [int(rng.integers(0, 64)) for _ in strings]) if strings else np.zeros((0, 4), np.uint64)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,m", SHAPES)
def test_groups_of_a_batch_and_of_every_word_boundary(exe, tmp_path, k, m, canonical):
    rng = np.random.default_rng(128 * k + m)
    seq = O.synth(k + m, 900)
    seq[[200, 611]] = ord("N")
    offs = np.array([0, 150, 300, 301, 300 + k, 900], np.uint64)
    mn, fp, mp, sz, hs = M.groups(seq, offs, k, m, SEED, canonical, _hash64)
    recs = np.concatenate([edge_records(k, rng), M.pack(seq, fp, sz, k, mp)])
    assert len(recs) > 10
    fate = check_against_model(run_count(exe, tmp_path, recs, k, m, canonical), recs, k, m, canonical)
    if fate["path"] != "table":  # the batch's k-mers exceed one table: a prefix that fits, so that the table path is held against the model too
        keep = int(np.searchsorted(np.cumsum([M.record_size(r) for r in recs]), M.limits()["CT_CAP"], side="right"))
        assert check_against_model(run_count(exe, tmp_path, recs[:keep], k, m, canonical), recs[:keep], k, m, canonical)["path"] == "table"


def test_groups_of_one_base(exe, tmp_path):
    recs = M.records_from_bases(["A", "C", "G", "T", "ACGT" * 16], 1, [0, 0, 0, 0, 63])  # k = 1: one base per k-mer, 64 k-mers at most
    for canonical in (False, True):
        assert check_against_model(run_count(exe, tmp_path, recs, 1, 1, canonical), recs, 1, 1, canonical)["path"] == "table"


def test_inconsistent_record_bits_terminate(exe, tmp_path):
    """size and mm_pos that k and m do not allow, and base bits where a record has none: the bodies read zeros, never out of bounds"""
    rng = np.random.default_rng(7)
    recs = rng.integers(0, 1 << 64, (40, 4), dtype=np.uint64, endpoint=False)
    recs[0] = 2**64 - 1
    for k, m in ((64, 32), (33, 1)):
        got = run_count(exe, tmp_path, recs, k, m, True)
        want = M.expand(recs, k, True)
        assert got["n_kmers"] == len(want) and got["path"] == M.bucket_fate(recs, k, True)["path"]


def test_buckets_at_the_table_limits(exe, tmp_path):
    lim = M.limits()
    names = {"full_2_rounds_table", "full_2_rounds_fallback", "full_2_rounds_canonical_table", "total_eq_cap", "total_eq_cap_plus_1", "recs_limit_plus_1",
             "chain_of_CT_FULL_wraps", "canonical_cluster_with_duplicates", "k59_polyT_max_with_neighbour", "k59_polyT_one_record_more"}
    cases = [c for c in M.all_count_cases(lim) if c["name"] in names]
    assert len(cases) == len(names)
    for case in cases:
        M.check_case(case, lim)
        got = run_count(exe, tmp_path, case["records"], case["k"], case["m"], case["canonical"])
        fate = check_against_model(got, case["records"], case["k"], case["m"], case["canonical"])
        assert fate["path"] == case["path"], case["name"]
        if case["path"] == "table":
            assert len(got["kmers"]) == case["distinct"]
            if "top_count" in case:
                assert max(got["kmers"].values()) == case["top_count"]


def test_poly_t_at_k_64(exe, tmp_path):
    recs = M.records_from_bases(["T" * 122, "T" * 64], 64, 0)
    got = run_count(exe, tmp_path, recs, 64, 32, False)
    assert got["path"] == "table" and got["kmers"] == {2**128 - 1: 60}  # all ones in both words: a key like any other
    assert run_count(exe, tmp_path, recs, 64, 32, True)["kmers"] == {0: 60}


@pytest.mark.parametrize("n_bases,origin", [(1000, 0), (1000, 10**12 + 7), (5, 0), (5, 10**12 + 7)])
def test_pack_clipping(exe, tmp_path, n_bases, origin):
    rng = np.random.default_rng(n_bases + origin % 1000)
    seq = rng.choice(np.frombuffer(b"ACGTacgtUuN", np.uint8), n_bases)
    fps, sizes, mms, ks = [], [], [], []
    for k in (1, 31, 33, 59, 64):
        pos = [0, 1, n_bases - 1, n_bases, n_bases + 1, max(n_bases - 130, 0), max(n_bases - 64, 0), 2**64 - 1, 2**64 - 122, 2**63]
        fp = [(origin + p) & M.M64 if p < 2**62 else (origin - (2**64 - p)) & M.M64 for p in pos]
        for b in EDGE_BASES:
            if k <= b <= k + 63:
                for p in fp + [(origin + max(n_bases - b, 0)) & M.M64, (origin + max(n_bases - b + 1, 0)) & M.M64]:
                    fps.append(p); sizes.append(b - k + 1); mms.append(int(rng.integers(0, 64))); ks.append(k)
    for k in sorted(set(ks)):
        sel = [i for i, kk in enumerate(ks) if kk == k]
        fp = np.array([fps[i] for i in sel], np.uint64)
        sz = np.array([sizes[i] for i in sel], np.uint8)
        mp = np.array([mms[i] for i in sel], np.uint8)
        src, dst = tmp_path / "pack.in", tmp_path / "pack.out"
        src.write_bytes(struct.pack("<QQQQ", n_bases, origin, len(fp), k) + fp.tobytes() + sz.tobytes() + mp.tobytes() + seq.tobytes())
        run = subprocess.run([exe, "pack", str(src), str(dst)], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr[-4000:]
        got = np.frombuffer(dst.read_bytes(), np.uint64).reshape(-1, 4)
        want = M.pack_clipped(seq, fp.tolist(), sz.tolist(), k, mp.tolist(), origin)
        assert np.array_equal(got, want), (k, np.nonzero((got != want).any(1))[0][:5])
        assert (want[:, :3].any(1)).sum() > 0 or n_bases < k  # some groups do lie in the batch
