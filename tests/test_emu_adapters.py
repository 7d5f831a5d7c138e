"""CPU-only: the bodies of bl_scan_read_adapters (biolib_amd/csrc/bl_adapters_core.hpp: the chunks staged from the packed copy and from
ASCII, the funnel-shifted windows, the mismatch counts, the poly walk's stop, the reverse complement and d(I)) emulated on the host under
AddressSanitizer / UBSan (tests/emu/emu_adapters.cpp, a stand-alone program, nothing preloaded) over arrays of exactly their lengths,
against the numpy model (adapter_cases.py).  Index bugs are to be found here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import adapter_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
RAN = ("packed", "ascii", "behind", "reversed", "diff", "key", "poly")


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_adapters.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_adapters")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


@pytest.fixture(scope="module")
def results():
    """the model's answer to every named case, computed once and left unchanged"""
    return {name: AC.batch_model(reads, r, spans) for name, (reads, r, spans) in AC.cases().items()}


def run(exe, tmp_path, reads, r, spans_in=None, packed=True, offsets=True, read_len=0, rule_bytes=None):
    """the emulated call -> (records, spans, stats, which bodies ran), or the message of a refused rule"""
    lay = AC.layout(reads)
    if isinstance(offsets, np.ndarray):
        lay["offsets"] = offsets
        offsets = True
    n = len(lay["offsets"]) - 1 if offsets else len(reads)
    (tmp_path / "bases.bin").write_bytes(lay["bases"])
    (tmp_path / "offsets.bin").write_bytes(lay["offsets"].tobytes())
    (tmp_path / "rule.bin").write_bytes(AC.rule_struct(r).tobytes() if rule_bytes is None else rule_bytes)
    if spans_in is not None:
        (tmp_path / "spans.bin").write_bytes(np.ascontiguousarray(spans_in, np.uint64).tobytes())
    cmd = [exe, tmp_path / "bases.bin", tmp_path / "offsets.bin" if offsets else "-", read_len, n, tmp_path / "spans.bin" if spans_in is not None else "-",
           tmp_path / "rule.bin", 1 if packed else 0, tmp_path / "out"]
    res = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    if res.stdout.startswith("invalid"):
        return res.stdout.strip()
    words = [int(x) for x in res.stdout.split()]
    recs = np.fromfile(tmp_path / "out.records", AC.RECORD)
    spans = np.fromfile(tmp_path / "out.spans", np.uint64).reshape(-1, 2)
    assert len(recs) == n and len(spans) == n
    stats = dict(zip(AC.STATS, words[7:18]))
    stats["per_adapter"] = words[18:26]
    return recs, spans, stats, dict(zip(RAN, words[:7]))


def same(got, want, reads, tag):
    recs, spans, stats, _ = got
    w_recs, w_spans, w_stats = want
    bad = np.nonzero(recs != w_recs)[0]
    assert len(bad) == 0, (tag, [(int(i), len(reads[i]), recs[i], w_recs[i]) for i in bad[:4]])
    assert np.array_equal(spans, w_spans), tag
    assert stats == w_stats, tag


@pytest.mark.parametrize("name", sorted(AC.cases()))
def test_named_cases(exe, tmp_path, results, name):
    """every case from the packed copy and from ASCII; every body ran somewhere (summed below)"""
    reads, r, spans_in = AC.cases()[name]
    for packed in (True, False):
        got = run(exe, tmp_path, reads, r, spans_in, packed)
        same(got, results[name], reads, (name, packed))
        ran = got[3]
        assert (ran["packed"] > 0) == packed and (packed or ran["ascii"] > 0) and ran["behind"] > 0
        assert (ran["key"] > 0) == bool(r["adapters"]) and (ran["poly"] > 0) == bool(r["poly_before"] | r["poly_after"])
        assert (ran["diff"] > 0) == bool(r["flags"] & 1) and (ran["reversed"] > 0) == bool(r["flags"] & 1)


@pytest.mark.parametrize("name", sorted(AC.cases()))
def test_all_byte_values(exe, tmp_path, name):
    """every case again with all 256 byte values as bases: one base in sixteen replaced, the adapters' traces left in between"""
    rng = np.random.default_rng(23)
    reads, r, spans_in = AC.cases()[name]
    rs = []
    for k, x in enumerate(reads):
        y = np.frombuffer(x, np.uint8).copy()
        if len(y) >= 256 and k % 4 == 0:
            y[:256] = rng.permutation(256)
        else:
            where = rng.random(len(y)) < 0.06
            y[where] = rng.integers(0, 256, int(where.sum()))
        rs.append(y.tobytes())
    rs += [bytes(range(256)), bytes(range(255, -1, -1))]
    if spans_in is not None:
        spans_in = np.concatenate([spans_in, np.array([(0, AC.U64), (3, 250)], np.uint64)])
    assert len({b for x in rs for b in x}) == 256
    want = AC.batch_model(rs, r, spans_in)
    for packed in (True, False):
        got = run(exe, tmp_path, rs, r, spans_in, packed)
        same(got, want, rs, (name, packed))
        assert got[3]["ascii"] > 0 and (got[3]["packed"] > 0) == packed, "bad chunks come from ASCII, clean ones from the packed copy"


def test_every_residue_of_the_batch(exe, tmp_path):
    """a read starts at every residue mod 32 of the batch: a first read of 0 .. 31 bases moves all the others"""
    picked = {}
    for name in ("lengths", "pair", "spans_in"):
        reads, r, spans_in = AC.cases()[name]
        keep = [i for i in range(0, len(reads), 2) if len(reads[i]) <= 1100 or len(reads[i]) == 5000][:24]
        idx = [j for i in keep for j in (i, i + 1)]
        picked[name] = ([reads[i] for i in idx], r, None if spans_in is None else spans_in[idx])
    seen = set()
    for name, (reads, r, spans_in) in picked.items():
        want = AC.batch_model(reads, r, spans_in)
        for pad in range(32):
            front = [AC.dna(pad, pad), b""]   # (two reads: mates stay mates)
            rs = front + reads
            sp = None if spans_in is None else np.concatenate([np.zeros((2, 2), np.uint64), spans_in])
            seen |= {int(x) % 32 for x in AC.layout(rs)["offsets"][2:-1]}
            recs, spans, stats, _ = run(exe, tmp_path, rs, r, sp, packed=True)
            bad = np.nonzero(recs[2:] != want[0])[0]
            assert len(bad) == 0 and np.array_equal(spans[2:], want[1]), (name, pad, bad[:4])
    assert seen == set(range(32))


def test_fixed_length_reads_and_no_slack(exe, tmp_path):
    """reads of one length without offsets (the last read ends with the batch: n_bases is no multiple of 16 and nothing lies behind it),
    and ragged batches whose last read ends at n_bases, for the packed copy's last chunk and the ASCII window's end"""
    for L, n in ((150, 7), (33, 10), (16, 4), (1, 5)):
        reads = [AC.planted(L, AC.TRUSEQ, (7 * k) % L, k) for k in range(n - 2)] + [AC.dna(L, 99)[:-1] + b"N", AC.dna(L - 1, 98) + b"G"]
        r = AC.rule(flags=AC.PAIRED if n % 2 == 0 else 0, adapters=[AC.TRUSEQ, AC.ADAPTERS["nextera"]], poly_after=4, poly_min_len=1, pair_min_overlap=1)
        want = AC.batch_model(reads, r)
        for packed in (True, False):
            same(run(exe, tmp_path, reads, r, None, packed, offsets=False, read_len=L), want, reads, (L, packed))
    for tail in (b"", b"A", AC.planted(15, AC.TRUSEQ, 2, 1), AC.planted(17, AC.TRUSEQ, 4, 2), AC.dna(16, 3), b"G" * 31, b"N"):
        reads = [AC.dna(40, 4), tail]
        r = AC.rule(flags=AC.PAIRED, adapters=[AC.TRUSEQ], poly_before=4, poly_after=15, poly_min_len=2, pair_min_overlap=1)
        want = AC.batch_model(reads, r)
        for packed in (True, False):
            same(run(exe, tmp_path, reads, r, None, packed), want, reads, (tail, packed))


def test_wrong_offsets_and_spans_end_clean(exe, tmp_path):
    """offsets and input spans that point anywhere: the run ends clean under the sanitizers, and the records are the model's for the reads
    that the clamped offsets describe (blsel::read_extent: both boundaries clamped to n_bases, a read that ends before it starts is empty)"""
    rng = np.random.default_rng(3)
    reads, r, _ = AC.cases()["pair_all_steps"]
    n = len(reads)
    n_bases = sum(map(len, reads))
    for k in range(4):
        offsets = rng.integers(0, n_bases + 500, n + 1).astype(np.uint64)
        if k % 2 == 0:
            offsets = np.sort(offsets)
        spans = rng.integers(0, 1 << 63, (n, 2), dtype=np.uint64) if k < 2 else rng.integers(0, 300, (n, 2)).astype(np.uint64)
        bases = b"".join(reads)
        bounds = np.minimum(offsets, np.uint64(n_bases)).astype(np.int64)
        described = [bases[bounds[i]:max(bounds[i], bounds[i + 1])] for i in range(n)]
        assert any(len(x) == 0 for x in described) and any(len(x) > 100 for x in described)
        want = AC.batch_model(described, r, spans)
        for packed in (True, False):
            got = run(exe, tmp_path, reads, r, spans, packed, offsets=offsets)
            assert not isinstance(got, str)
            same(got, want, described, (k, packed))


def test_refuses_bad_rules(exe, tmp_path):
    reads = [AC.dna(30, 1), AC.dna(30, 2), AC.dna(30, 3)]
    good = AC.rule(adapters=[AC.TRUSEQ])
    assert not isinstance(run(exe, tmp_path, reads, good), str)

    def refused(what, r=good, **fields):
        s = AC.rule_struct(r)
        for k, x in fields.items():
            s[k] = x
        msg = run(exe, tmp_path, reads, r, rule_bytes=s.tobytes())
        assert isinstance(msg, str) and what in msg, (what, msg)

    refused("flag", flags=2)
    refused("even", flags=1)
    refused("n_adapters", n_adapters=9)
    refused("1 .. 64", adapter_len=[0] + [0] * 7)
    refused("1 .. 64", adapter_len=[65] + [0] * 7)
    refused("ACGTUacgtu", AC.rule(adapters=[b"ACGN"]))
    refused("ACGTUacgtu", AC.rule(adapters=[AC.TRUSEQ, b"ACG\x00"]))
    refused("min_overlap", min_overlap=0)
    refused("error_den", error_den=0)
    refused("error_num", error_num=11)
    refused("pair_error_den", pair_error_den=0)
    refused("pair_error_num", pair_error_num=6)
    refused("poly mask", poly_before=16)
    refused("poly mask", poly_after=16)
    refused("poly_min_len", poly_before=4, poly_min_len=0)
    refused("reserved", reserved=1)
    msg = run(exe, tmp_path, reads + [b"ACGT"], AC.rule(flags=1, pair_min_overlap=0))
    assert isinstance(msg, str) and "pair_min_overlap" in msg
    # what is no mistake: min_overlap 0 without adapters, pair_min_overlap 0 without the flag, poly_min_len 0 without a mask
    assert not isinstance(run(exe, tmp_path, reads, AC.rule(min_overlap=0, pair_min_overlap=0, poly_min_len=0)), str)
