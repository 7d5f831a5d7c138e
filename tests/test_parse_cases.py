"""CPU: the hand-built texts of parse_cases.py.  The plain model of the reference reader, the library's host reader and the reference
reader itself (recorded in tests/golden/ref_verdicts.json, read live where oracle/_ref is built) agree on every text; the table keeps its
shape; and the device-side parser's per-thread code (biolib_amd/csrc/bl_parse_core.hpp), run thread by thread on the host under the
sanitizers (tests/emu/emu_parse.cpp), accepts every regular text, refuses every text the reference calls an error and returns the
reference's sequences for whatever it accepts — the table in its order and again reversed, over a scratch that is never cleared."""
import os
import struct
import subprocess

import pytest

import oracle_lib as O
import parse_cases as PC
import test_ingest as TI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = PC.recorded()


def test_table_is_the_recorded_one():
    assert sorted(PC.CASES) == sorted(RECORDED), "regenerate tests/golden/ref_verdicts.json (make_ref_golden.py) after changing the table"
    for name, text in PC.CASES.items():
        assert PC.text_sha(text) == RECORDED[name]["text"], name
        assert len(text) <= PC.MAX_TEXT, name
    assert set(PC.BGZF_NAMES + PC.FIXED_UNIFORM + PC.FIXED_RAGGED + list(PC.STILL_ACCEPTED)) <= set(PC.CASES) and len(PC.BGZF_NAMES) >= 12


def test_model_and_host_reader_match_the_reference_reader(tmp_path):
    import biolib_amd

    path = tmp_path / "f.txt"
    bad = []
    for name, text in PC.CASES.items():
        path.write_bytes(text)
        exp = RECORDED[name]["ref"]
        if O.have_ref():
            assert PC.compact(TI.reads_verdict(TI._ref_read(path))) == exp, name
        try:
            host = [s for _, s in biolib_amd.Reader(path).records()]
        except biolib_amd.BiolibError:
            host = None
        if PC.verdict(PC.kseq_model(text)) != exp or PC.verdict(host) != exp:
            bad.append(name)
    assert not bad, bad


def test_the_rows_the_parser_used_to_get_wrong():
    """what the reference reader makes of the texts that bl_parse.hip accepted and mis-parsed before it refused them"""
    assert PC.kseq_model(b">h\r\n\r\nACGT\r\n") == [b"\rACGT"] and PC.CASES["lone_cr_first_crlf"] == b">h\r\n\r\nACGT\r\n"
    assert PC.kseq_model(b">h\n\r") == [b"\r"] and PC.CASES["lone_cr_only"] == b">h\n\r"
    assert PC.kseq_model(PC.CASES["lone_cr_fq"]) == [b"\r", b"AC"]
    assert PC.kseq_model(b">h\r\nAC\r\n\r\nGT\r\n") == [b"ACGT"] and PC.CASES["lone_cr_after_bases"] == b">h\r\nAC\r\n\r\nGT\r\n"
    for c in ("at", "plus", "gt"):
        assert RECORDED["fq_seq_opens_with_" + c]["ref"] is None and RECORDED["fq_seq_is_" + c]["ref"] is None


def test_regular_cases():
    regular = [name for name, text in PC.CASES.items() if PC.is_regular(text)]
    assert not [name for name in regular if RECORDED[name]["ref"] is None]
    assert 2 * len(regular) >= len(PC.CASES)  # "refuse everything" must not pass
    assert not [name for name in PC.STILL_ACCEPTED if PC.is_regular(PC.CASES[name]) or RECORDED[name]["ref"] is None]
    for name in PC.FIXED_UNIFORM + PC.FIXED_RAGGED:
        assert name in regular
    for u, group in (("fixed_uniform", ("fixed_ragged_first", "fixed_ragged_last")), ("fixed_uniform_300", ("fixed_ragged_255_256",))):
        seqs = PC.kseq_model(PC.CASES[u])
        assert PC.expected_fixed_len(seqs) == 100
        for r in group:  # the same count and the same total, one pair of lengths apart
            rag = PC.kseq_model(PC.CASES[r])
            assert len(rag) == len(seqs) and b"".join(rag) == b"".join(seqs) and PC.expected_fixed_len(rag) == 0
            assert sorted(set(map(len, rag))) == [99, 100, 101]
    rag = [len(x) for x in PC.kseq_model(PC.CASES["fixed_ragged_255_256"])]
    assert (rag[255], rag[256]) == (99, 101)


def run_emulation(tmp_path, names):
    """[(name, None | (n_seqs, fixed_len, lengths, bases))] from tests/emu/emu_parse.cpp, in the order given"""
    exe = os.path.join(ROOT, "tests", "emu", "_build", "emu_parse")
    assert os.path.exists(exe), "tests/emu/_build/emu_parse is missing: make -C tests/emu (__graft_entry__.build())"
    case_file = tmp_path / "cases.bin"
    with open(case_file, "wb") as f:
        for name in names:
            text = PC.CASES[name]
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<Q", len(text)) + text)
    p = subprocess.run([exe, str(case_file)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.endswith("emu_parse: OK %d cases\n" % len(names)), p.stdout[-2000:] + p.stderr[-4000:]
    assert not p.stderr, p.stderr[-4000:]  # the sanitizers' reports
    out = []
    for name, line in zip(names, p.stdout.splitlines()):
        parts = line.split("\t")
        assert parts[0] == name
        if parts[1].startswith("refused: "):
            assert "bl_reader_" in parts[1] or "quality length" in parts[1], line
            out.append((name, None))
        else:
            out.append((name, (int(parts[1]), int(parts[2]), [int(x) for x in parts[3].split(",")] if parts[3] else [], bytes.fromhex(parts[4]))))
    return out


def check_parse(name, got, exp, problems):
    """got: None (refused) or (n_seqs, lengths, bases) of an accepted text; exp: the reference's verdict"""
    if got is None:
        if PC.is_regular(PC.CASES[name]) or name in PC.STILL_ACCEPTED:
            problems.append((name, "refused"))
        return
    n_seqs, lens, bases = got
    seqs, at = [], 0
    for L in lens:
        seqs.append(bases[at:at + L])
        at += L
    if exp is None:
        problems.append((name, "accepted where the reference reports an error"))
    elif n_seqs != len(lens) or at != len(bases) or PC.verdict(seqs) != exp:
        problems.append((name, "differs from the reference", lens[:8]))


def test_emulation_under_the_sanitizers(tmp_path):
    names = PC.ORDER + PC.ORDER[::-1]
    problems, accepted = [], 0
    for name, got in run_emulation(tmp_path, names):
        check_parse(name, got and (got[0], got[2], got[3]), RECORDED[name]["ref"], problems)
        if got is not None:
            accepted += 1
            if got[1] != PC.expected_fixed_len(PC.kseq_model(PC.CASES[name]) or [b""]):
                problems.append((name, "fixed length", got[1]))
    assert not problems, problems
    assert accepted >= len(names) // 2
    refused = {name for name, got in run_emulation(tmp_path, ["lone_cr_first_crlf", "lone_cr_only", "lone_cr_fq", "fq_seq_opens_with_at"]) if got is None}
    assert len(refused) == 4  # (also alone, as the first text a fresh scratch sees)
