"""GPU: the device-side FASTA / FASTQ parser (bl_batch_from_text, bl_parse_device_text) on the hand-built texts of parse_cases.py, the
reference reader's recorded verdicts (tests/golden/ref_verdicts.json, key parser_cases) as the judge: a regular text is accepted, a text
the reference calls an error is refused, and whatever is accepted gives the reference's sequences — counts, bases and boundaries.  One
context parses the whole table, large and small texts alternating, and then the table reversed: the parser's scratch only grows and is
never cleared, so no result may depend on the text parsed before."""
import numpy as np
import pytest

import oracle_lib as O
import parse_cases as PC
from test_ingest import _bgzf
from test_parse_cases import check_parse

pytestmark = pytest.mark.gpu
RECORDED = PC.recorded()


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def test_table_forward_and_reversed(ctx):
    import biolib_amd

    problems, accepted = [], 0
    for name in PC.ORDER + PC.ORDER[::-1]:
        text, exp = PC.CASES[name], RECORDED[name]["ref"]
        try:
            b = ctx.from_text(text)
        except biolib_amd.BiolibError as e:
            check_parse(name, None, exp, problems)
            assert "bl_reader_" in str(e) or "quality length" in str(e), (name, str(e))
            continue
        accepted += 1
        bases = bytes(b.download())
        want = PC.kseq_model(text)  # (test_parse_cases.py holds it against the recorded verdict)
        lens = [len(x) for x in want] if want is not None and len(want) == b.n_seqs else [len(bases)] + [0] * (b.n_seqs - 1)
        before = len(problems)
        if b.n_bases != len(bases):
            problems.append((name, "n_bases", b.n_bases, len(bases)))
        check_parse(name, (b.n_seqs, lens, bases), exp, problems)
        if len(problems) == before and len(bases):
            # sequence boundaries: every base is its own unit, windows of 2 never cross a boundary
            v, p, h = O.minimizers(np.frombuffer(bases, np.uint8), _offsets(lens), 1, 2, 0, False, brute=False)
            if not np.array_equal(b.minimizers(1, 2)["positions"], p):
                problems.append((name, "sequence boundaries"))
        b.close()
    assert not problems, problems
    assert accepted >= len(PC.ORDER)  # half of the two passes: the regular texts


def _scan(ctx, name):
    text = PC.CASES[name]
    seqs = PC.kseq_model(text)
    b = ctx.from_text(text)
    got = b.minimizers(21, 5, canonical=True)
    kernels = ctx.last_scan_kernels()
    seq = np.frombuffer(b"".join(seqs), np.uint8)
    v, p, h = O.minimizers(seq, _offsets([len(x) for x in seqs]), 21, 5, 0, True, brute=False)
    assert b.n_seqs == len(seqs) and np.array_equal(b.download(), seq), name
    assert np.array_equal(got["positions"], p) and np.array_equal(got["values"], v) and np.array_equal(got["hashes"], h), name
    b.close()
    return kernels


@pytest.mark.parametrize("name", PC.FIXED_UNIFORM)
def test_reads_of_one_length_take_the_read_tiled_kernels(ctx, name):
    ctx.from_text(PC.CASES["fixed_ragged_first"]).close()  # a ragged text in front: its offsets stay in the recycled buffers
    kernels = _scan(ctx, name)
    assert kernels and kernels[0].startswith("frl"), kernels


@pytest.mark.parametrize("name", PC.FIXED_RAGGED)
def test_equal_mean_ragged_reads_do_not(ctx, name):
    ctx.from_text(PC.CASES["fixed_uniform_300"]).close()  # uniform offsets in front
    kernels = _scan(ctx, name)
    assert kernels and not [k for k in kernels if k.startswith("frl")], kernels


@pytest.mark.parametrize("name", PC.BGZF_NAMES)
def test_compressed_path(ctx, tmp_path, name):
    """BGZF -> inflate and cut on the device -> the parser, in several spans"""
    import biolib_amd

    text, exp = PC.CASES[name], RECORDED[name]["ref"]
    block = max(40, len(text) // 6)
    path = tmp_path / "t.gz"
    path.write_bytes(_bgzf(text, block=block))
    r = biolib_amd.Reader(path)
    assert r.kind == "bgzf"
    got, n_seqs, spans = [], 0, 0
    try:
        for b in r.device_batches(ctx, 2 * block):
            got.append(bytes(b.download()))
            n_seqs += b.n_seqs
            spans += 1
            b.close()
    except biolib_amd.BiolibError:
        assert exp is None, name
        return
    finally:
        r.close()
    assert exp is not None, name
    seqs = PC.kseq_model(text)
    assert PC.verdict(seqs) == exp and b"".join(got) == b"".join(seqs) and n_seqs == len(seqs), (name, n_seqs, spans)
    assert spans >= 2 or len(text) < 128, (name, spans)
