"""CPU-only: the Python specification of the text index and the FASTA / FASTQ writer (format_cases.py: index_model, format_model, the
arithmetic of biolib_amd/csrc/bl_format_core.hpp) against a plain restatement — the text split into lines, strings joined per record —
on the named cases, and the round trip index -> format on the parser's own accepted texts (parse_cases.py)."""
import numpy as np
import pytest

import format_cases as FC
import parse_cases as PC


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_model_equals_the_plain_restatement(name):
    c = FC.cases()[name]
    got, want = FC.format_model(c), FC.format_plain(c)
    assert got[1] == want[1], name
    assert got[0] == want[0], (name, got[0][:200], want[0][:200])


def test_the_cases_reach_their_branches():
    C = FC.cases()
    assert FC.format_model(C["zero_records"]) == (b"", 0)
    assert FC.format_model(C["one_base"])[0] == C["one_base"]["text"]
    assert FC.format_model(C["minimal_fastq"]) == (b"@\n\n+\n\n", 1) and len(FC.format_model(C["minimal_fastq"])[0]) == 6
    assert FC.format_model(C["crlf"])[0] == C["crlf"]["text"].replace(b"\r\n", b"\n")
    assert FC.format_model(C["crlf_fasta"])[0] == C["crlf_fasta"]["text"].replace(b"\r\n", b"\n")
    assert FC.format_model(C["unterminated"])[0] == C["unterminated"]["text"] + b"\n"
    assert FC.format_model(C["trailing_blank_lines"])[0] == C["trailing_blank_lines"]["text"][:-4]
    assert FC.format_model(C["wrapped_fasta_source"])[0] == C["wrapped_fasta_source"]["text"]
    assert FC.format_model(C["lengths"])[0] == C["lengths"]["text"]
    out = FC.format_model(C["numbers_9_to_10"])[0]
    assert out.startswith(b"@n8 KC:i:9\n") and b"@n9 KC:i:10\n" in out and b"@n10 KC:i:18446744073709551615\n" in out
    assert b"@n4294967295 " in FC.format_model(C["numbers_2_pow_32"])[0] and b"@n4294967296 " in FC.format_model(C["numbers_2_pow_32"])[0]
    assert b"@n18446744073709551615 " in FC.format_model(C["numbers_2_pow_64_wraps"])[0] and b"@n0 " in FC.format_model(C["numbers_2_pow_64_wraps"])[0]
    for W in FC.LINE_WIDTHS:
        out = FC.format_model(C["line_width_%d" % W])[0]
        body = [ln for ln in out.split(b"\n")[:-1] if not ln.startswith(b">")]
        assert max(map(len, body)) == W and b"\n\n>" in out and not out.endswith(b"\n\n"), W  # (an empty sequence is one empty line; none behind a full last line)
    keep, skip = FC.format_model(C["spans_keep_empty"]), FC.format_model(C["spans_keep_empty_skip"])
    assert keep[1] == 7 and skip[1] == 5 and skip == FC.format_model(C["spans_compacted"]) and b"\n\n+\n\n" in keep[0]
    assert FC.format_model(C["spans_null_source_index"]) == keep
    assert b"!" * 10 + b"\n" in FC.format_model(C["spans_overrun_gets_fill"])[0] and b"!" * 50 + b"\n" in FC.format_model(C["spans_overrun_gets_fill"])[0]
    lost = FC.format_model(C["source_index_past_the_index"])[0]
    assert b"@lost12\n" in lost and b"@lost4\n" in lost and b"@lost13\n" in lost and b"@lost4294967301\n" in lost
    assert lost.count(b"~" * 40) == 4 and lost.count(b"~" * 7 + b"\n") == 4  # reads of 40, 40, 7 and 100 bases got the fill
    assert FC.format_model(C["fastq_to_fasta"])[0].count(b">") >= 7 and b"+\n" not in FC.format_model(C["fastq_to_fasta"])[0]
    assert FC.format_model(C["fasta_to_fastq"])[0].count(b"5" * 33) == 1
    a = C["alignments"]
    recs, offs, _ = FC.index_model(a["text"])
    out_offs = FC.record_offsets(a)[:-1]
    for what in (recs["name_begin"], recs["name_begin"] + recs["name_len"] + 1, recs["name_begin"] + recs["qual_delta"], out_offs, offs[:-1]):
        assert set(int(x) % 4 for x in what) == {0, 1, 2, 3}
    assert FC.wave_paths(FC.record_offsets(C["many_tiny"]))[1] >= 1 and FC.wave_paths(FC.record_offsets(C["lengths"]))[0] >= 3


def test_index_model_equals_the_plain_parse():
    for name, c in FC.cases().items():
        if not c["text"]:
            continue
        recs, offs, fastq = FC.index_model(c["text"])
        names, seqs, quals = FC.parse_plain(c["text"])
        assert len(recs) == len(names) and (quals is not None) == fastq, name
        assert [int(b) - int(a) for a, b in zip(offs[:-1], offs[1:])] == [len(s) for s in seqs], name
        for r, nm, i in zip(recs, names, range(len(names))):
            at = int(r["name_begin"])
            assert c["text"][at:at + int(r["name_len"])] == nm, name
            if fastq:
                q = at + int(r["qual_delta"])
                assert c["text"][q:q + len(seqs[i])] == quals[i], name


def round_trip_texts():
    """the accepted texts of parse_cases.py that a writer can give back byte for byte: LF-terminated 4-line FASTQ with a bare '+', and
    FASTA wrapped uniformly (every line of a record but its last as wide as the file's widest), both without blank lines.  Decided by
    writing the plain parse back with plain joins, not by the model."""
    out = {}
    for name in PC.ORDER:
        text = PC.CASES[name]
        if not PC.is_regular(text) or b"\r" in text or not text.endswith(b"\n"):
            continue
        names, seqs, quals = FC.parse_plain(text)
        if quals is not None:
            if FC.fastq_text(names, seqs, quals=quals) == text:
                out[name] = 0
        else:
            width = max([len(ln) for ln in text.split(b"\n") if ln[:1] != b">"] + [0])
            if FC.fasta_text(names, seqs, width=width) == text:
                out[name] = width
    return out


def test_round_trip_of_the_parsers_texts():
    texts = round_trip_texts()
    assert sum(1 for n in texts if PC.CASES[n][:1] == b"@") >= 5 and sum(1 for n in texts if PC.CASES[n][:1] == b">") >= 5, sorted(texts)
    for name, width in texts.items():
        text = PC.CASES[name]
        c = FC.case(text, fmt="fastq" if text[:1] == b"@" else "fasta", line_width=width)
        assert np.array_equal(np.frombuffer(b"".join(PC.kseq_model(text)), np.uint8), c["bases"]), name
        assert FC.format_model(c)[0] == text, name
