"""CPU-only: the bodies of bl_scan_read_quality and bl_spans_intersect (biolib_amd/csrc/bl_quality_core.hpp: the funnel-shifted loads of
the quality line and the bases, the masks, the running sums, the window, the statistics and filters) emulated on the host under
AddressSanitizer / UBSan (tests/emu/emu_quality.cpp, a stand-alone program, nothing preloaded) over arrays of exactly their lengths,
against the numpy model (quality_cases.py).  Index bugs are to be found here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import quality_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_quality.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_quality")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


@pytest.fixture(scope="module")
def reads():
    return QC.reads()


def run_quality(exe, tmp_path, lay, rule, fastq=True, with_records=True):
    """the emulated call -> (records, spans, stats, (short fours, wave reads, swept reads))"""
    n = len(lay["offsets"]) - 1
    (tmp_path / "text.bin").write_bytes(lay["text"])
    (tmp_path / "records.bin").write_bytes(lay["records"].tobytes())
    (tmp_path / "offsets.bin").write_bytes(lay["offsets"].tobytes())
    (tmp_path / "bases.bin").write_bytes(lay["bases"])
    cmd = [exe, "quality", tmp_path / "text.bin", tmp_path / "records.bin", tmp_path / "offsets.bin", tmp_path / "bases.bin", n, 1 if fastq else 0,
           1 if with_records else 0, tmp_path / "out"] + QC.rule_words(rule)
    r = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    if r.stdout.strip() == "invalid":
        return None
    words = [int(x) for x in r.stdout.split()]
    recs = np.fromfile(tmp_path / "out.records", QC.RECORD)
    spans = np.fromfile(tmp_path / "out.spans", np.uint64).reshape(-1, 2)
    assert len(recs) == n and len(spans) == n
    return recs, spans, dict(zip(QC.STATS, words[3:])), tuple(words[:3])


def same(got, want, rs, tag):
    recs, spans, stats, _ = got
    w_recs, w_spans, w_stats = want
    for i in range(len(rs)):
        assert recs[i] == w_recs[i], (tag, rs[i][0], len(rs[i][1]), recs[i], w_recs[i])
    assert np.array_equal(spans, w_spans), tag
    assert stats == w_stats, tag


@pytest.mark.parametrize("name", sorted(QC.rules()))
def test_named_cases(exe, tmp_path, reads, name):
    r = QC.rules()[name]
    got = run_quality(exe, tmp_path, QC.layout(reads), r)
    same(got, QC.batch_model(reads, r), reads, name)
    short, wave, sweep = got[3]
    assert short > 0 and wave > 0 and sweep > 0, "both forms and the short body ran"


@pytest.mark.parametrize("name", sorted(QC.rules()))
def test_spans_alone(exe, tmp_path, reads, name):
    """a call without records takes only the statistics its filters need: the spans and the totals are the same"""
    r = QC.rules()[name]
    _, spans, stats, _ = run_quality(exe, tmp_path, QC.layout(reads), r, with_records=False)
    _, w_spans, w_stats = QC.batch_model(reads, r)
    assert np.array_equal(spans, w_spans) and stats == w_stats, name


@pytest.mark.parametrize("name", ["all_steps", "fastp", "filters", "edges", "maxsum_both", "window65"])
def test_all_byte_values(exe, tmp_path, reads, name):
    """every case again, its quality bytes and bases replaced by all 256 byte values, for both Phred bases"""
    rng = np.random.default_rng(21)
    rs = []
    for rname, bases, qual in reads:
        L = len(bases)
        q = rng.integers(0, 256, L).astype(np.uint8)
        q[:min(L, 256)] = rng.permutation(256)[:min(L, 256)]
        rs.append((rname, rng.integers(0, 256, L).astype(np.uint8).tobytes(), q.tobytes()))
    assert len({x for _, _, q in rs for x in q}) == 256 and len({x for _, b, _ in rs for x in b}) == 256
    for base in (33, 64):
        r = dict(QC.rules()[name], phred_base=base)
        same(run_quality(exe, tmp_path, QC.layout(rs), r), QC.batch_model(rs, r), rs, (name, base))


def test_every_residue_of_the_quality_line(exe, tmp_path, reads):
    """the quality lines start at every residue mod 16 of the text, and the last ends with the text or one byte in front of its end"""
    rs = [x for x in reads if len(x[1]) in (0, 1, 15, 16, 17, 65, 150, 257, 1025)][:40] + [x for x in reads if x[0] == b"len5003"]
    r = QC.rules()["all_steps"]
    want = QC.batch_model(rs, r)
    seen = set()
    for pad in range(16):
        for newline in (True, False):
            lay = QC.layout(rs, pad, newline)
            seen |= {int(x["name_begin"] + x["qual_delta"]) % 16 for x in lay["records"][1:]}
            same(run_quality(exe, tmp_path, lay, r), want, rs, (pad, newline))
    assert seen == set(range(16))
    # a text that ends inside the last quality line: the fill behind it, and no byte behind the text is read
    lay = QC.layout(rs)
    lay["text"] = lay["text"][:-1000]
    cut = [(n, b, (q[:len(q) - 999] + bytes([r["quality_fill"]]) * 999) if i == len(rs) - 1 else q) for i, (n, b, q) in enumerate(rs)]
    same(run_quality(exe, tmp_path, lay, r), QC.batch_model(cut, r), rs, "cut text")


def test_fasta_index_gives_the_fill(exe, tmp_path, reads):
    for name in ("filters", "fill_low", "window4"):
        r = QC.rules()[name]
        lay = QC.layout(reads)
        lay["records"] = np.zeros(0, QC.TEXT_RECORD)
        same(run_quality(exe, tmp_path, lay, r, fastq=False), QC.batch_model(reads, r, fasta_index=True), reads, name)


def test_wrong_offsets_and_records_end_clean(exe, tmp_path, reads):
    """offsets and index records that point anywhere: the run ends clean under the sanitizers"""
    rng = np.random.default_rng(3)
    lay = QC.layout(reads)
    n = len(reads)
    for _ in range(3):
        bad = dict(lay)
        bad["offsets"] = np.sort(rng.integers(0, len(lay["bases"]) + 500, n + 1)).astype(np.uint64)
        recs = lay["records"].copy()
        recs["name_begin"] = rng.integers(0, len(lay["text"]) + 100, n)
        recs["qual_delta"] = rng.integers(0, 6000, n)
        bad["records"] = recs
        assert run_quality(exe, tmp_path, bad, QC.rules()["all_steps"]) is not None


def test_refuses_bad_rules(exe, tmp_path, reads):
    lay = QC.layout(reads[:4])
    assert run_quality(exe, tmp_path, lay, QC.rule()) is not None
    for change in (dict(phred_base=34), dict(quality_fill=32), dict(quality_fill=127), dict(front_q=95), dict(back_q=95), dict(maxsum_front_q=95),
                   dict(maxsum_back_q=95), dict(window_q=95), dict(low_q=95), dict(mean_q=95), dict(window_len=65536), dict(low_max_den=0),
                   dict(low_max_num=2, low_max_den=1), dict(reserved=1)):
        assert run_quality(exe, tmp_path, lay, QC.rule(**change)) is None, change


def run_intersect(exe, tmp_path, offsets, read_len, n_bases, a, b, paired):
    n = len(a)
    (tmp_path / "a.bin").write_bytes(np.ascontiguousarray(a, np.uint64).tobytes())
    if b is not None:
        (tmp_path / "b.bin").write_bytes(np.ascontiguousarray(b, np.uint64).tobytes())
    if offsets is not None:
        (tmp_path / "offsets.bin").write_bytes(np.ascontiguousarray(offsets, np.uint64).tobytes())
    cmd = [exe, "intersect", "-" if offsets is None else tmp_path / "offsets.bin", tmp_path / "a.bin", "-" if b is None else tmp_path / "b.bin", read_len,
           n_bases, n, 1 if paired else 0, tmp_path / "out.bin"]
    r = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.fromfile(tmp_path / "out.bin", np.uint64).reshape(-1, 2)


def test_intersect(exe, tmp_path):
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 300, 200)
    lengths[:6] = (0, 0, 1, 1, 10, 10)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    a = np.sort(rng.integers(0, 330, (200, 2)), axis=1).astype(np.uint64)
    b = rng.integers(0, 330, (200, 2)).astype(np.uint64)
    a[4], b[4] = (12, 20), (0, 10)   # empty only after clamping to the read's 10 bases
    a[5], b[5] = (0, QC.U64), (3, QC.U64)
    for bb in (b, None):
        for paired in (False, True):
            got = run_intersect(exe, tmp_path, offsets, 0, int(offsets[-1]), a, bb, paired)
            assert np.array_equal(got, QC.intersect_model(lengths, a, bb, paired)), (bb is None, paired)
    fixed = np.full(200, 150)
    got = run_intersect(exe, tmp_path, None, 150, 200 * 150, a, b, True)
    assert np.array_equal(got, QC.intersect_model(fixed, a, b, True))
