"""CPU-only: the bodies of bl_batch_select and bl_read_spans (biolib_amd/csrc/bl_select_core.hpp: span lengths, placement, the gather
with its wave-bounded bisection, aligned-dword path, seam loop and source tail, the fixed-length rule, the span rule) emulated on the host
under AddressSanitizer / UBSan (tests/emu/emu_select.cpp) over arrays of exactly their lengths, against the numpy model
(select_cases.py).  Index bugs are to be found here, not on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import select_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(ROOT, "tests", "emu", "emu_select.cpp")
    out = os.path.join(ROOT, "tests", "emu", "_build", "emu_select")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([CXX if os.path.exists(CXX) else "clang++", "-std=c++17", "-O1", "-g", "-DBL_CPU_EMU", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
                           src, "-o", out], timeout=600)
    return out


@pytest.fixture(scope="module")
def batch():
    b = SC.batch()
    SC.self_check(b)
    return b


def run_select(exe, tmp_path, bases, offs, spans, read_len=0, keep_empty=False, n_seqs=None):
    """the emulated call -> dict as select_model's"""
    n_seqs = len(spans) if n_seqs is None else n_seqs
    (tmp_path / "bases.bin").write_bytes(np.ascontiguousarray(bases, np.uint8).tobytes())
    (tmp_path / "spans.bin").write_bytes(np.ascontiguousarray(spans, np.uint64).tobytes())
    if offs is not None:
        (tmp_path / "offsets.bin").write_bytes(np.ascontiguousarray(offs, np.uint64).tobytes())
    cmd = [exe, "select", tmp_path / "bases.bin", "-" if offs is None else tmp_path / "offsets.bin", tmp_path / "spans.bin", read_len, len(bases), n_seqs,
           1 if keep_empty else 0, tmp_path / "out"]
    r = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    n_out, total, fixed, register_waves, memory_waves = (int(x) for x in r.stdout.split())
    got = dict(paths=(register_waves, memory_waves), bases=np.fromfile(tmp_path / "out.bases", np.uint8), offsets=np.fromfile(tmp_path / "out.offsets", np.uint64),
               source_index=np.fromfile(tmp_path / "out.index", np.uint64), n_seqs=n_out, n_bases=total, fixed_len=fixed)
    assert len(got["bases"]) == total and len(got["offsets"]) == n_out + 1 and len(got["source_index"]) == n_out
    return got


def same(got, want, names=None, tag=""):
    assert (got["n_seqs"], got["n_bases"], got["fixed_len"]) == (want["n_seqs"], want["n_bases"], want["fixed_len"]), tag
    assert np.array_equal(got["source_index"], want["source_index"]), tag
    assert np.array_equal(got["offsets"], want["offsets"]), tag
    bad = np.nonzero(got["bases"] != want["bases"])[0]
    if len(bad):
        seq = int(np.searchsorted(want["offsets"], bad[0], side="right")) - 1
        src = int(want["source_index"][seq])
        raise AssertionError((tag, "first wrong byte", int(bad[0]), "of", len(bad), "result sequence", seq, names[src] if names else src))


def test_case_batch(exe, tmp_path, batch):
    want = SC.self_check(batch)
    got = run_select(exe, tmp_path, batch["bases"], batch["offs"], batch["spans"])
    same(got, want, batch["names"], "cases")
    assert want["fixed_len"] == 0
    assert got["paths"][0] >= 8, "waves that keep their sequences in registers"


@pytest.mark.parametrize("name", sorted(SC.variants()))
def test_variants(exe, tmp_path, name):
    v = SC.variants()[name]
    want = SC.expected(v)
    got = run_select(exe, tmp_path, v["bases"], v["offs"], v["spans"], v["read_len"], v["keep_empty"])
    same(got, want, None, name)
    if name.startswith("all_dropped"):
        assert got["n_bases"] == 0 and got["n_seqs"] == (len(v["spans"]) if v["keep_empty"] else 0)
    if name in ("result_fixed", "result_whole_reads"):
        assert got["fixed_len"] in (100, 150) and got["n_seqs"] > 1
    if name in ("result_just_not_fixed", "result_one_sequence", "keep_empty"):
        assert got["fixed_len"] == 0
    if name == "many_tiny":
        assert got["paths"] == (0, 1), "more than 63 sequences in the wave: looked up in memory"
    if v["keep_empty"]:
        assert np.array_equal(got["source_index"], np.arange(len(v["spans"]), dtype=np.uint64))


@pytest.mark.parametrize("name", sorted(SC.scale_variants()))
def test_scale_variants(exe, tmp_path, name):
    """search depths 0 .. 4, the switch between the two lookups at 62, 63 and 64 lane offsets, runs of 64 and more empty kept sequences,
    totals around a wave's bytes: the result byte for byte, and the lookup every wave took as the header's prose says it must"""
    v = SC.scale_variants()[name]
    want = SC.expected(v)
    SC.scale_self_check(name, v, want)
    got = run_select(exe, tmp_path, v["bases"], v["offs"], v["spans"], v["read_len"], v["keep_empty"])
    same(got, want, None, name)
    assert got["paths"] == SC.wave_paths(want["offsets"]), (name, "register waves, memory waves")
    if name in ("switch", "empty_runs"):
        assert got["paths"][0] > 0 and got["paths"][1] > 0, "both kinds of wave"
    if name == "switch_first0":
        assert got["paths"][1] == 0
    if name == "switch_first1":
        assert got["paths"] == (1, len(SC.wave_inside(want["offsets"])) - 1), "the last, partial wave alone keeps its sequences in registers"


def test_given_offsets_equal_null_offsets(exe, tmp_path):
    """a fixed-length and a single-sequence source give the same result with their offsets spelled out"""
    for name in ("fixed_source", "single_sequence", "result_fixed"):
        v = SC.variants()[name]
        got = run_select(exe, tmp_path, v["bases"], SC.variant_offsets(v), v["spans"], 0, v["keep_empty"])
        same(got, SC.expected(v), None, name)


def test_every_cut_of_a_short_source(exe, tmp_path):
    """one read of 0 .. 40 bases, span [b, L): the source's tail at every alignment of both ends, the buffer exactly L bytes"""
    rng = np.random.default_rng(3)
    for L in list(range(0, 41)) + [63, 64, 65, 4096, 4097, 4099]:
        bases = rng.integers(1, 255, L).astype(np.uint8)
        for b in sorted({0, 1, 2, 3, 4, 5, 15, 16, 17} & set(range(L + 1))):
            n = 1 if L else 0  # (a batch of no bases holds no sequence)
            spans = np.tile(np.array([[b, SC.U64]], np.uint64), (n, 1))
            got = run_select(exe, tmp_path, bases, None, spans, n_seqs=n)
            want = SC.select_model(bases, np.array([0, L][:n + 1], np.uint64), spans)
            same(got, want, None, (L, b))


def test_wrong_offsets_and_garbage_spans_end_clean(exe, tmp_path, batch):
    """shuffled, out-of-range offsets and random spans: the result is whatever the header's clamping rule makes of them — the model
    applies the same rule — and the run ends clean under the sanitizers (every array is a heap array of exactly its length)"""
    b = batch
    for seed in range(4):
        rng = np.random.default_rng(seed)
        bad = SC.wrong_offsets(b["offs"], rng)
        garbage = SC.garbage_spans(len(b["spans"]), rng)
        for offs, spans in ((bad, b["spans"]), (b["offs"], garbage), (bad, garbage)):
            for keep_empty in (False, True):
                got = run_select(exe, tmp_path, b["bases"], offs, spans, 0, keep_empty)
                same(got, SC.select_model(b["bases"], offs, spans, keep_empty), None, ("wrong", seed, keep_empty))


def run_spans(exe, tmp_path, lengths, records, stat, rule, offs="ragged"):
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    (tmp_path / "records.bin").write_bytes(records.tobytes())
    (tmp_path / "offsets.bin").write_bytes(offsets.tobytes())
    if stat is not None:
        (tmp_path / "stat.bin").write_bytes(np.ascontiguousarray(stat, np.uint32).tobytes())
    cmd = [exe, "spans", tmp_path / "records.bin", "-" if stat is None else tmp_path / "stat.bin", tmp_path / "offsets.bin", 0, int(offsets[-1]), len(lengths),
           tmp_path / "spans.out"] + SC.rule_words(rule)
    r = subprocess.run([str(x) for x in cmd], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    if r.stdout.strip() == "invalid":
        return None
    return np.fromfile(tmp_path / "spans.out", np.uint64).reshape(-1, 2)


@pytest.mark.parametrize("name", sorted(SC.span_cases()[3]))
def test_read_spans(exe, tmp_path, name):
    lengths, records, stat, rules = SC.span_cases()
    r = rules[name]
    for st in (stat, None):
        got = run_spans(exe, tmp_path, lengths, records, st, r)
        want = SC.read_spans_model(lengths, records, r, st)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (name, st is None, [(int(lengths[i]), records[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    assert (got[:, 1].astype(np.int64) <= lengths).all() and (got[:, 0] <= got[:, 1]).all()


def test_read_spans_refuses_bad_rules(exe, tmp_path):
    lengths, records, stat, rules = SC.span_cases()
    good = SC.rule("prefix", 31)
    assert run_spans(exe, tmp_path, lengths, records, stat, good) is not None
    for change in (dict(trim=4), dict(k=0), dict(k=65), dict(solid_min=(1, 0)), dict(solid_min=(3, 2)), dict(solid_max=(0, 0)), dict(solid_max=(5, 4)), dict(reserved=1)):
        assert run_spans(exe, tmp_path, lengths, records, stat, dict(good, **change)) is None, change
