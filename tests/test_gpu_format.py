"""GPU: the text index and the FASTA / FASTQ writer (bl_text_index_build, bl_batch_format, bl_text_write; biolib_amd/csrc/bl_format.hip)
against the Python specification (format_cases.py) byte for byte — guard bytes behind the output, the sizing call, the capacity refusal,
reruns, every refusal — the index's batch against bl_batch_from_text's on the parser's own texts (parse_cases.py), and the chain's exit
end to end: simulated FASTQ in, trimmed and corrected FASTQ out, read back with the host reader."""
import functools

import numpy as np
import pytest

import format_cases as FC
import parse_cases as PC
from test_format_model import round_trip_texts
from test_ingest import _bgzf

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def rule_of(c):
    import biolib_amd

    r = c["rule"]
    return biolib_amd.Batch.format_rule(r["fmt"], r["label"], r["prefix"], r["first_number"], r["line_width"], r["quality_fill"], r["skip_empty"], r["tag_length"])


class OnDevice:
    """a case's batch, index and arrays on the device"""

    def __init__(self, ctx, c):
        self.c, self.rule = c, rule_of(c)
        self.index = None
        if c["text"]:
            own, self.index = ctx.from_text_indexed(c["text"])
            own.close()
        self.batch = ctx.upload(c["bases"], offsets=c["offsets"]) if len(c["offsets"]) > 1 else ctx.upload(b"")  # (no sequence: no offsets to upload)
        self.args = dict(index=self.index, source_index=dev(c["source_index"]), spans=dev(c["spans"]), tags=dev(c["tags"]), offsets=self.batch._device_offsets(None))

    def run(self, capacity=None):
        """(n_bytes, n_records, the whole output buffer with its guard) — the buffer holds 0xA5 where nothing was written"""
        import torch

        n_bytes, n_records = self.batch.format_raw(self.rule, None, 0, **self.args)
        out = torch.full((n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        got = self.batch.format_raw(self.rule, out, n_bytes if capacity is None else capacity, **self.args)
        assert got == (n_bytes, n_records), "the sizing call and the writing call disagree"
        return n_bytes, n_records, out.cpu().numpy()

    def close(self):
        self.batch.close()
        if self.index is not None:
            self.index.close()


@pytest.mark.parametrize("name", sorted(FC.cases()))
def test_cases(ctx, name):
    import biolib_amd
    import torch

    c = FC.cases()[name]
    want, want_records = FC.format_model(c)
    d = OnDevice(ctx, c)
    n_bytes, n_records, out = d.run()
    assert (n_bytes, n_records) == (len(want), want_records), name
    got = out[:n_bytes].tobytes()
    assert got == want, (name, next(i for i in range(len(want)) if got[i] != want[i]))
    assert (out[n_bytes:] == 0xA5).all(), "bytes behind the text were written"
    assert np.array_equal(d.run()[2], out), "a rerun differs"
    if n_bytes:  # one byte short: refused, nothing written
        buf = torch.full((n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(biolib_amd.BiolibError) as e:
            d.batch.format_raw(d.rule, buf, n_bytes - 1, **d.args)
        assert e.value.code == biolib_amd.capi.BL_ERR_CAPACITY and bool((buf == 0xA5).all())
    # the method: the same text as a tensor of exactly its size
    how = dict(fmt=c["rule"]["fmt"], tag_label=c["rule"]["label"], prefix=c["rule"]["prefix"], first_number=c["rule"]["first_number"], line_width=c["rule"]["line_width"],
               quality_fill=c["rule"]["quality_fill"], skip_empty=c["rule"]["skip_empty"], tag_length=c["rule"]["tag_length"])
    t = d.batch.format(index=d.index, source_index=d.args["source_index"], spans=d.args["spans"], tags=d.args["tags"], **how)
    assert t.dtype == torch.uint8 and t.cpu().numpy().tobytes() == want
    d.close()


def test_index_contents(ctx):
    for name in ("name_lengths", "crlf", "unterminated", "trailing_blank_lines", "wrapped_fasta_source", "many_tiny", "alignments"):
        text = FC.cases()[name]["text"]
        b, ix = ctx.from_text_indexed(text)
        records, offs, fastq = FC.index_model(text)
        assert (ix.n_records, ix.is_fastq, ix.n_bytes) == (len(records), fastq, len(text)), name
        assert np.array_equal(ix.records(), records.astype(ix.records().dtype)) and np.array_equal(ix.offsets.cpu().numpy().view(np.uint64), offs), name
        assert ix.text() == text and ix.names() == FC.parse_plain(text)[0], name
        ix.close()
        b.close()


def test_index_batch_equals_from_text_on_the_parsers_texts(ctx):
    """every text of parse_cases.py, large and small alternating: the same refusals with the same messages, and where accepted the same
    bases, count, offsets and fixed-length rule; a parse without index in between leaves the index's text alone (it is not in the
    parser's scratch)"""
    import biolib_amd

    accepted, kept = 0, None
    for name in PC.ORDER:
        text = PC.CASES[name]
        try:
            plain = ctx.from_text(text)
        except biolib_amd.BiolibError as e:
            with pytest.raises(biolib_amd.BiolibError) as e2:
                ctx.from_text_indexed(text)
            assert str(e2.value) == str(e) and e2.value.code == e.code, name
            continue
        accepted += 1
        b, ix = ctx.from_text_indexed(text)
        seqs = PC.kseq_model(text)
        assert (b.n_seqs, b.n_bases) == (plain.n_seqs, plain.n_bases) == (len(seqs), sum(map(len, seqs))), name
        assert b.download().tobytes() == plain.download().tobytes() == b"".join(seqs), name
        offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        assert np.array_equal(ix.offsets.cpu().numpy().view(np.uint64), offs) and np.array_equal(b.offsets, offs), name
        assert b.read_len == PC.expected_fixed_len(seqs), name
        if b.n_bases:  # the fixed-length rule inside the library: the same scan kernels are chosen for both
            want = plain.minimizers(21, 5, canonical=True)
            kernels = ctx.last_scan_kernels()
            got = b.minimizers(21, 5, canonical=True)
            assert ctx.last_scan_kernels() == kernels and got["count"] == want["count"] and np.array_equal(got["positions"], want["positions"]), name
        if kept is not None:  # the index of the text before survived this parse
            assert kept[0].text() == kept[1]
            kept[0].close()
        kept = (ix, text)
        plain.close()
        b.close()
    kept[0].close()
    assert accepted >= len(PC.ORDER) // 2


def test_round_trip_of_the_parsers_texts(ctx):
    for name, width in round_trip_texts().items():
        text = PC.CASES[name]
        b, ix = ctx.from_text_indexed(text)
        out = b.format(fmt="fastq" if text[:1] == b"@" else "fasta", index=ix, line_width=width)
        assert out.cpu().numpy().tobytes() == text, name
        ix.close()
        b.close()


@pytest.mark.parametrize("n", (255, 256, 257, 1023, 1024, 1025, 4097))
def test_record_counts_around_a_wave_and_a_workgroup(ctx, n):
    """16-byte records: 256 of them are a wave's 4 KiB and a workgroup of the length kernel, 1,024 a workgroup of the write"""
    c = FC.case(None, FC.dna(6 * n, n), np.arange(n + 1) * 6, fmt="fasta", first_number=10**6)
    want = FC.format_model(c)[0]
    assert len(want) == 16 * n
    b = ctx.upload(c["bases"], read_len=6)
    assert b.format(fmt="fasta", first_number=10**6).cpu().numpy().tobytes() == want
    b.close()


def refused(call):
    import biolib_amd

    with pytest.raises(biolib_amd.BiolibError) as e:
        call()
    assert e.value.code == biolib_amd.capi.BL_ERR_INVALID, str(e.value)
    return str(e.value)


def test_refusals(ctx):
    import biolib_amd
    import torch
    from biolib_amd import capi

    c = FC.cases()["alignments_trimmed"]
    d = OnDevice(ctx, c)
    n_bytes, _, _ = d.run()
    out = torch.full((n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    L = ctx._lib

    def raw(ctx_h=ctx._h, batch_h=d.batch._h, offsets=d.args["offsets"], index_h=d.index._h, spans=d.args["spans"], rule=d.rule, dest=out):
        nb = biolib_amd.scan.C.c_uint64()
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        capi.check(L.bl_batch_format(ctx_h, batch_h, ptr(offsets), index_h, ptr(d.args["source_index"]), ptr(spans), None,
                                     biolib_amd.scan.C.byref(rule) if rule is not None else None, ptr(dest), n_bytes, biolib_amd.scan.C.byref(nb), None))

    raw()  # (the call as it is passes)
    assert out[:n_bytes].cpu().numpy().tobytes() == FC.format_model(c)[0]
    out.fill_(0xA5)
    refused(lambda: raw(ctx_h=None))
    refused(lambda: raw(batch_h=None))
    refused(lambda: raw(rule=None))
    assert "d_offsets is NULL" in refused(lambda: raw(offsets=None))
    assert "16-byte aligned" in refused(lambda: raw(spans=d.args["spans"].data_ptr() + 8))
    assert "16-byte aligned" in refused(lambda: raw(dest=out.data_ptr() + 4))
    other = biolib_amd.Context(0)
    foreign_batch = other.upload(c["bases"], offsets=c["offsets"])
    foreign_own, foreign_index = other.from_text_indexed(c["text"])
    assert "another context" in refused(lambda: raw(batch_h=foreign_batch._h))
    assert "another context" in refused(lambda: raw(index_h=foreign_index._h))
    other.close()
    make = biolib_amd.Batch.format_rule
    bad = [make(fmt=2), make(fmt="fastq", line_width=60), make(quality_fill=32), make(quality_fill=127), make(prefix=b"sixteen_bytes_16"), make(tag_label=b"sixteen_bytes_16")]
    flags, reserved = make(), make()
    flags.flags, reserved.reserved = 4, 1
    for r in bad + [flags, reserved]:
        assert "bl_format_rule" in refused(lambda: raw(rule=r))
    assert bool((out == 0xA5).all()), "a refused call wrote"
    with pytest.raises(ValueError):
        d.batch.format(spans=d.args["spans"])  # spans without an index
    d.close()


def test_write_reports_io_errors(ctx, tmp_path):
    import biolib_amd

    b = ctx.upload(b"ACGT" * 10, read_len=4)
    with pytest.raises(biolib_amd.BiolibError) as e:
        b.write(tmp_path / "no_such_directory" / "x.fq")
    assert e.value.code == biolib_amd.capi.BL_ERR_IO
    n = b.write(tmp_path / "x.fa", fmt="fasta", prefix="r")
    b.write(tmp_path / "x.fa", append=True, fmt="fasta", prefix="r", first_number=10)
    want = b"".join(b">r%d\nACGT\n" % i for i in range(20))
    assert (tmp_path / "x.fa").read_bytes() == want and n == 90 and len(want) == 190
    b.close()


@functools.lru_cache(maxsize=None)
def simulated_fastq():
    """a 20-kbp genome, 30x reads of 100 bp from both strands with 1 % substitutions, as 4-line FASTQ with distinct names and random
    qualities: (text, names, sequences, qualities)"""
    import correct_cases as CC

    bases, _, offs, _ = CC.simulate(seed=7, genome_len=20000, read_len=100, coverage=30, rate=0.01)
    raw = bases.tobytes()
    seqs = [raw[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
    names = [b"sim.%d/%d" % (i * 7919 % len(seqs), 1 + i % 2) for i in range(len(seqs))]
    quals = [q.tobytes() for q in np.random.default_rng(8).integers(33, 127, (len(seqs), 100)).astype(np.uint8)]
    return FC.fastq_text(names, seqs, quals=quals), names, seqs, quals


def test_end_to_end_trim_correct_write(ctx, tmp_path):
    import biolib_amd
    import torch

    k = 21
    text, names, seqs, quals = simulated_fastq()
    assert len(set(names)) == len(names) == 6000
    b, ix = ctx.from_text_indexed(text)
    scan = b.kmers(k, canonical=True)
    counted = ctx.count_table(torch.from_numpy(np.ascontiguousarray(scan["values"][scan["valid"] != 0]).view(np.int64)).cuda(), key_bits=2 * k)
    rc, _ = b.read_counts(counted, k, 3, canonical=True)
    spans = b.read_spans(rc, k, "prefix")
    kept, source_index = b.select(spans)
    edits, stats = kept.read_edits(counted, k, 3, canonical=True)
    fixed = kept.apply_edits(edits)
    assert 0 < kept.n_seqs < len(seqs) and kept.read_len == 0, "ragged after trimming"
    path = tmp_path / "out.fq"
    n_bytes = fixed.write(path, index=ix, source_index=source_index, spans=spans)
    data = path.read_bytes()
    assert n_bytes == len(data)
    # the host reader is the semantic reference
    r = biolib_amd.Reader(path)
    records = list(r.records())
    r.close()
    src, host_spans = source_index.cpu().numpy(), spans.cpu().numpy()
    corrected, offs = fixed.download().tobytes(), fixed.offsets
    assert len(records) == kept.n_seqs == len(src)
    got_names, got_seqs, got_quals = FC.parse_plain(data)
    for i, (nm, seq) in enumerate(records):
        s = int(src[i])
        lo, hi = int(host_spans[s][0]), int(host_spans[s][1])
        assert nm.encode("latin1") == names[s] == got_names[i], i
        assert seq == corrected[int(offs[i]):int(offs[i + 1])] == got_seqs[i] and len(seq) == hi - lo, i
        assert got_quals[i] == quals[s][lo:hi], i
    # and the device parser takes the file again
    again, ix2 = ctx.from_text_indexed(data)
    assert again.n_seqs == fixed.n_seqs and again.download().tobytes() == corrected and np.array_equal(again.offsets, offs)
    assert ix2.names() == got_names
    for x in (again, ix2, fixed, kept, counted, ix, b):
        x.close()


def test_unitigs_write_fasta(ctx, tmp_path):
    import torch

    from test_gpu_graph import reads_case  # the planted-repeat genome

    k = 21
    b = ctx.upload(reads_case(), read_len=100)
    scan = b.kmers(k, canonical=True)
    counted = ctx.count_table(torch.from_numpy(np.ascontiguousarray(scan["values"][scan["valid"] != 0]).view(np.int64)).cuda(), key_bits=2 * k)
    table = counted.filter(3)
    u = table.unitigs(k)
    assert u.n_unitigs > 1
    for width in (0, 60):
        path = tmp_path / ("unitigs_%d.fa" % width)
        n = u.write_fasta(path, line_width=width)
        data = path.read_bytes()
        assert n == len(data)
        names, seqs, _ = FC.parse_plain(data)
        offs = u.offsets.cpu().numpy().view(np.uint64)
        sums = u.count_sums.cpu().numpy().view(np.uint64)
        assert names == [b"%d LN:i:%d KC:i:%d" % (i, int(offs[i + 1] - offs[i]), int(sums[i])) for i in range(u.n_unitigs)]
        assert b"".join(seqs) == u.batch.download().tobytes()
        assert max(len(ln) for ln in data.split(b"\n") if ln[:1] != b">") == (60 if width else int((offs[1:] - offs[:-1]).max()))
        again, ix = ctx.from_text_indexed(data)
        assert again.n_seqs == u.n_unitigs and again.download().tobytes() == u.batch.download().tobytes() and np.array_equal(again.offsets, offs)
        again.close()
        ix.close()
    for x in (u.batch, table, counted, b):
        x.close()


@pytest.mark.parametrize("kind", ("bgzf", "plain"))
def test_a_file_rewritten_span_by_span(ctx, tmp_path, kind):
    """Reader.device_batches(indexed=True) on a file cut into at least three spans, every span formatted and appended: the file with its
    line ends normalised (CRLF -> LF)"""
    import biolib_amd

    n = 400
    seqs = [FC.dna(20 + i % 150, i) for i in range(n)]
    names = [b"span.%d extra words" % i for i in range(n)]
    text = FC.fastq_text(names, seqs, nl=b"\r\n")
    src = tmp_path / ("in.fq.gz" if kind == "bgzf" else "in.fq")
    src.write_bytes(_bgzf(text, block=6000) if kind == "bgzf" else text)
    dst = tmp_path / "out.fq"
    r = biolib_amd.Reader(src)
    assert r.kind == kind
    spans = total = 0
    for b, ix in r.device_batches(ctx, len(text) // 5, indexed=True):
        if b.n_seqs:
            spans += 1
        total += b.n_seqs
        b.write(dst, append=spans > 1, index=ix)
        ix.close()
        b.close()
    r.close()
    assert spans >= 3 and total == n
    assert dst.read_bytes() == text.replace(b"\r\n", b"\n")
