"""CPU-only: the bodies of bl_scan_read_duplicates (biolib_amd/csrc/bl_dedup_core.hpp: the key words from the packed copy and from ASCII,
their reversal, the hash's parts, the marks and heads of a round, the comparison with the head, the members' entries and the records)
emulated on the host under AddressSanitizer / UBSan (tests/emu/emu_dedup.cpp, a stand-alone program, nothing preloaded) over arrays of
exactly their lengths, against the model (dedup_cases.py).  Index bugs are to be found here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import dedup_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
RAN = ("packed", "ascii", "reversed", "hash", "compare", "head", "singleton", "finish")
WORK = ("n_mixed_groups", "rounds")


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_dedup.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_dedup")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


@pytest.fixture(scope="module")
def results():
    """the model's answer to every named case, computed once and left unchanged"""
    return {name: DC.batch_model(c.reads, c.rule, c.spans_in, c.scores) for name, c in DC.cases().items()}


def run(exe, tmp_path, reads, r, spans_in=None, scores=None, packed=True, offsets=True, read_len=0, n_seqs=None):
    """the emulated call -> (records, spans, stats, work, which bodies ran), or the message of a refused rule"""
    lay = DC.layout(reads)
    if isinstance(offsets, np.ndarray):
        lay["offsets"] = offsets
        offsets = True
    n = n_seqs if n_seqs is not None else (len(lay["offsets"]) - 1 if offsets else len(reads))
    (tmp_path / "bases.bin").write_bytes(lay["bases"])
    (tmp_path / "offsets.bin").write_bytes(lay["offsets"].tobytes())
    (tmp_path / "rule.bin").write_bytes(DC.rule_struct(r).tobytes())
    if spans_in is not None:
        (tmp_path / "spans.bin").write_bytes(np.ascontiguousarray(spans_in, np.uint64).tobytes())
    if scores is not None:
        (tmp_path / "scores.bin").write_bytes(np.array([int(x) for x in scores], np.uint64).tobytes())
    cmd = [exe, tmp_path / "bases.bin", tmp_path / "offsets.bin" if offsets else "-", read_len, n, tmp_path / "spans.bin" if spans_in is not None else "-",
           tmp_path / "scores.bin" if scores is not None else "-", tmp_path / "rule.bin", 1 if packed else 0, tmp_path / "out"]
    res = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    if res.stdout.startswith("invalid"):
        return res.stdout.strip()
    words = [int(x) for x in res.stdout.split()]
    recs = np.fromfile(tmp_path / "out.records", DC.RECORD)
    spans = np.fromfile(tmp_path / "out.spans", np.uint64).reshape(-1, 2)
    per = 2 if r["flags"] & 1 else 1
    assert len(recs) == n // per and len(spans) == n
    k = len(RAN)
    stats = dict(zip(DC.STATS[1:], words[k:k + 7]), n_units=n // per, class_hist=words[k + 7:k + 23])
    return recs, spans, stats, dict(zip(WORK, words[k + 23:k + 25])), dict(zip(RAN, words[:k]))


def same(got, want, tag):
    recs, spans, stats = got[:3]
    w_recs, w_spans, w_stats = want
    bad = np.nonzero(recs != w_recs)[0]
    assert len(bad) == 0, (tag, [(int(i), recs[i], w_recs[i]) for i in bad[:4]])
    assert np.array_equal(spans, w_spans), tag
    assert stats == w_stats, (tag, stats, w_stats)


def run_case(exe, tmp_path, c, packed=True, **changes):
    r = dict(c.rule, **changes)
    return run(exe, tmp_path, c.reads, r, c.spans_in, c.scores, packed, offsets=not c.read_len, read_len=c.read_len)


@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_named_cases(exe, tmp_path, results, name):
    """every case from the packed copy and from ASCII"""
    c = DC.cases()[name]
    for packed in (True, False):
        got = run_case(exe, tmp_path, c, packed)
        same(got, results[name], (name, packed))
        ran = got[4]
        assert (ran["packed"] > 0) == packed and (packed or ran["ascii"] > 0) and ran["hash"] > 0 and ran["finish"] == got[2]["n_units"]
        assert (ran["reversed"] > 0) == (c.rule["flags"] == DC.CANONICAL)


@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_all_byte_values(exe, tmp_path, name):
    """every case again with all 256 byte values as bases: the same bytes planted in every copy of a read, so that the classes stay"""
    c = DC.cases()[name]
    if c.read_len:
        reads = [bytes(range(106, 256)) if i % 9 == 0 else (bytes(range(0, 150)) if i % 9 == 1 else x) for i, x in enumerate(c.reads)]
    else:
        table = {}
        for x in c.reads:
            if x not in table:
                rng = np.random.default_rng(len(table))
                y = np.frombuffer(x, np.uint8).copy()
                where = rng.random(len(y)) < 0.06
                y[where] = rng.integers(0, 256, int(where.sum()))
                table[x] = y.tobytes()
        reads = [table[x] for x in c.reads] + [bytes(range(256)), bytes(range(255, -1, -1))] * 2
    spans_in = None if c.spans_in is None else np.concatenate([c.spans_in, np.array([(0, DC.U64), (3, 250)] * 2, np.uint64)])
    scores = None if c.scores is None else list(c.scores) + [1, 2, 3, 4] * (0 if c.read_len else 1)
    assert len({b for x in reads for b in x}) == 256
    want = DC.batch_model(reads, c.rule, spans_in, scores)
    for packed in (True, False):
        got = run(exe, tmp_path, reads, c.rule, spans_in, scores, packed, offsets=not c.read_len, read_len=c.read_len)
        same(got, want, (name, packed))
        assert got[4]["ascii"] > 0 and (got[4]["packed"] > 0) == packed, "bad chunks come from ASCII, clean ones from the packed copy"


def test_every_residue_of_the_batch(exe, tmp_path):
    """a read starts at every residue mod 32 of the batch: a first pair of 0 .. 31 bases moves all the others"""
    seen = set()
    for name in ("lengths_canonical", "pairs_canonical", "one_difference"):
        c = DC.cases()[name]
        reads = [x for x in c.reads if len(x) <= 1100][:60]
        reads = reads[:len(reads) & ~1]
        for pad in range(32):
            rs = [DC.dna(pad, pad), b""] + reads   # (two reads: mates stay mates; an empty unit in front)
            want = DC.batch_model(rs, c.rule)
            seen |= {int(x) % 32 for x in DC.layout(rs)["offsets"][2:-1]}
            same(run(exe, tmp_path, rs, c.rule), want, (name, pad))
    assert seen == set(range(32))


def test_fixed_length_reads_and_no_slack(exe, tmp_path):
    """reads of one length without offsets (the last read ends with the batch: n_bases is no multiple of 16 and nothing lies behind it),
    and ragged batches whose last read ends at n_bases, for the packed copy's last chunk and the ASCII window's end"""
    for L, n in ((150, 8), (33, 10), (16, 4), (1, 6), (47, 6)):
        reads = [DC.dna(L, k % 3) for k in range(n - 2)] + [DC.dna(L, 1)[:-1] + b"N", DC.revcomp(DC.dna(L, 1))]
        for flags in (0, DC.CANONICAL, DC.PAIRED | DC.CANONICAL):
            r = DC.rule(flags=flags)
            want = DC.batch_model(reads, r)
            for packed in (True, False):
                same(run(exe, tmp_path, reads, r, None, None, packed, offsets=False, read_len=L), want, (L, flags, packed))
    for tail in (b"", b"A", DC.dna(15, 2), DC.dna(17, 4), DC.dna(16, 3), b"G" * 31, b"N", DC.dna(40, 4)):
        reads = [DC.dna(40, 4), tail, DC.dna(40, 4), tail]
        for flags in (0, DC.CANONICAL, DC.PAIRED):
            r = DC.rule(flags=flags)
            want = DC.batch_model(reads, r)
            for packed in (True, False):
                same(run(exe, tmp_path, reads, r, None, None, packed), want, (tail, flags, packed))


def test_wrong_offsets_and_spans_end_clean(exe, tmp_path):
    """offsets and input spans that point anywhere: the run ends clean under the sanitizers, and the records are the model's for the reads
    that the clamped offsets describe (blsel::read_extent: both boundaries clamped to n_bases, a read that ends before it starts is empty)"""
    rng = np.random.default_rng(3)
    c = DC.cases()["volume_ragged"]
    reads = c.reads[:60]
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
        r = DC.rule(flags=k, prefix_len=(0, 40)[k % 2])
        want = DC.batch_model(described, r, spans)
        for packed in (True, False):
            got = run(exe, tmp_path, reads, r, spans, None, packed, offsets=offsets)
            assert not isinstance(got, str)
            same(got, want, (k, packed))


def test_refuses_bad_rules(exe, tmp_path):
    reads = [DC.dna(30, 1), DC.dna(30, 2), DC.dna(30, 3)]
    assert not isinstance(run(exe, tmp_path, reads, DC.rule(hash_bits=96)), str)

    def refused(what, n_seqs=None, **fields):
        msg = run(exe, tmp_path, reads, DC.rule(**fields), offsets=n_seqs is None, read_len=1 if n_seqs else 0, n_seqs=n_seqs)
        assert isinstance(msg, str) and what in msg, (what, msg)

    refused("flag", flags=4)
    refused("flag", flags=1 << 31)
    refused("even", flags=DC.PAIRED)
    refused("hash_bits", hash_bits=97)
    refused("reserved", reserved=1)
    refused("2^32", n_seqs=1 << 32)
    refused("2^32", n_seqs=1 << 33, flags=DC.PAIRED)
    msg = run(exe, tmp_path, reads + [reads[0]], DC.rule(flags=DC.PAIRED | DC.CANONICAL, hash_bits=1, seed=DC.U64, prefix_len=DC.U64))
    assert not isinstance(msg, str)


@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_hash_bits_change_the_work_only(exe, tmp_path, results, name):
    """96, 8 and 1 bits and another seed: the same records, spans and statistics; the groups mix exactly where they must"""
    c = DC.cases()[name]
    n_classes = results[name][2]["n_classes"]
    for bits, seed in ((96, 0), (8, 0), (1, 0), (0, 12345), (1, 99)):
        got = run_case(exe, tmp_path, c, True, hash_bits=bits, seed=seed)
        same(got, results[name], (name, bits, seed))
        work = got[3]
        if bits in (0, 96):
            assert work["n_mixed_groups"] == 0 and work["rounds"] == 1
        if bits == 8 and n_classes >= 300:
            assert work["n_mixed_groups"] > 0 and work["rounds"] > 1
        if bits == 1 and n_classes >= 3:
            assert work["n_mixed_groups"] > 0 and work["rounds"] >= (n_classes + 1) // 2


def test_every_body_ran(exe, tmp_path):
    total = dict.fromkeys(RAN, 0)
    for name, packed, bits in (("lengths_canonical", True, 0), ("pairs_canonical", False, 1), ("volume_fixed", True, 8)):
        got = run_case(exe, tmp_path, DC.cases()[name], packed, hash_bits=bits)
        for k, x in got[4].items():
            total[k] += x
    assert all(total[k] > 0 for k in RAN), total
