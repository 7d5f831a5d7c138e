"""GPU tests of bl_scan_read_quality / bl_spans_intersect and their Python binding (Batch.read_quality_raw / read_quality /
intersect_spans / trim_by_quality): every named case of the model (quality_cases.py; the lane bodies were run under the sanitizers in
test_emu_quality.py) word for word with guard words behind every output, both Phred bases, a FASTA index, a fixed-length batch whose
count is no multiple of the reads per wave, the call's behaviour and refusals, and paired trimming end to end through the writers."""
import ctypes as C
import gzip

import numpy as np
import pytest

import quality_cases as QC

pytestmark = pytest.mark.gpu
PAD = 8
GUARD = -0x3A3A3A3A3A3A3A3B  # 0xC5C5...C5 as int64


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads():
    return QC.reads()


@pytest.fixture(scope="module")
def source(ctx, reads):
    """the named reads as an indexed FASTQ batch"""
    batch, index = ctx.from_text_indexed(QC.fastq(reads))
    assert batch.n_seqs == len(reads) and index.is_fastq
    return batch, index


@pytest.fixture(scope="module")
def pairs(ctx):
    text, rs = QC.paired_text(501)
    batch, index = ctx.from_text_indexed(text)
    assert batch.n_seqs == 1002 and batch.read_len == 150 and batch.n_seqs % 4 != 0
    return batch, index, rs, text


def capi_rule(r):
    from biolib_amd import capi

    out = capi.QualityRule()
    for k, x in r.items():
        setattr(out, k, int(x))
    return out


def call(batch, index, r, records=True, spans=True, stats=True):
    """the C call with guarded outputs -> (records, spans, stats) as the model's"""
    import torch

    from biolib_amd import capi

    n = batch.n_seqs
    d_rec = torch.full((n + PAD, 6), GUARD, dtype=torch.int64, device="cuda")
    d_spans = torch.full((n + PAD, 2), GUARD, dtype=torch.int64, device="cuda")
    st = capi.QualityStats()
    torch.cuda.synchronize()  # the raw call runs on the context's stream: torch's fills are complete first
    batch.read_quality_raw(index, r if isinstance(r, C.Structure) else capi_rule(r), d_rec if records else None, d_spans if spans else None, st if stats else None)
    batch.ctx.sync()
    rec, sp = d_rec.cpu().numpy(), d_spans.cpu().numpy()
    assert (rec[n if records else 0:] == GUARD).all() and (sp[n if spans else 0:] == GUARD).all(), "written behind or into an output it was not given"
    return (rec[:n].view(QC.RECORD).reshape(-1) if records else None, sp[:n].view(np.uint64) if spans else None, st.as_dict() if stats else None)


def same(got, want, rs, tag):
    recs, spans, stats = got
    w_recs, w_spans, w_stats = want
    bad = np.nonzero(recs != w_recs)[0]
    assert len(bad) == 0, (tag, [(rs[i][0], len(rs[i][1]), recs[i], w_recs[i]) for i in bad[:4]])
    assert np.array_equal(spans, w_spans), tag
    assert stats == w_stats, tag


@pytest.mark.parametrize("name", sorted(QC.rules()))
def test_named_cases(source, reads, name):
    """ragged reads of 0 .. 5,003 bases around every boundary of the bodies (16, 256, 1,024), windows of 1, 4, 64, 65 and 1,500, failing
    windows across a lane's, a group's and a chunk's end, ties and dips of the running sum, all-low and all-high reads"""
    batch, index = source
    r = QC.rules()[name]
    same(call(batch, index, r), QC.batch_model(reads, r), reads, name)


def test_phred_base_64(ctx, reads):
    rs = [x for x in reads if max(x[2], default=0) + 31 <= 126]
    assert len(rs) > len(reads) - 3
    batch, index = ctx.from_text_indexed(QC.fastq(rs, shift=31))
    shifted = [(n, b, bytes(q + 31 for q in qual)) for n, b, qual in rs]
    for name in ("all_steps", "fastp"):
        r = dict(QC.rules()[name], phred_base=64)
        same(call(batch, index, r), QC.batch_model(shifted, r), rs, name)
        # the same text read as Phred+33: every value 31 higher, capped at 93
        r33 = dict(r, phred_base=33)
        same(call(batch, index, r33), QC.batch_model(shifted, r33), rs, name + "/33")
    index.close()
    batch.close()


def test_fasta_index(ctx, reads):
    batch, index = ctx.from_text_indexed(QC.fasta(reads))
    assert not index.is_fastq and batch.n_seqs == len(reads)
    for name in ("filters", "fill_low", "window4"):
        r = QC.rules()[name]
        same(call(batch, index, r), QC.batch_model(reads, r, fasta_index=True), reads, name)
    index.close()
    batch.close()


@pytest.mark.parametrize("name", ["fastp", "all_steps", "maxsum_both"])
def test_fixed_length_reads(pairs, name):
    batch, index, rs, _ = pairs
    r = QC.rules()[name]
    same(call(batch, index, r), QC.batch_model(rs, r), rs, name)


def test_reruns_and_partial_outputs(source, reads):
    batch, index = source
    r = QC.rules()["all_steps"]
    first = call(batch, index, r)
    again = call(batch, index, r)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    only_records = call(batch, index, r, spans=False, stats=False)
    only_spans = call(batch, index, r, records=False, stats=False)
    assert only_records[0].tobytes() == first[0].tobytes() and only_spans[1].tobytes() == first[1].tobytes()
    nothing = call(batch, index, r, records=False, spans=False)
    assert nothing[2] == first[2]
    # max_ee as the one condition, without records: the error sums are taken for the spans alone
    r = QC.rule(max_ee=1 << 30)
    want = QC.batch_model(reads, r)
    assert np.array_equal(call(batch, index, r, records=False, stats=False)[1], want[1])


def test_python_binding(source, reads):
    batch, index = source
    rq = batch.read_quality(index, window=(4, 20), low_q=15, max_low=(2, 5), min_len=50, stats=True)
    want = QC.batch_model(reads, QC.rules()["fastp"])
    assert np.array_equal(rq.host(), want[0]) and np.array_equal(rq.spans.cpu().numpy().view(np.uint64), want[1]) and rq.stats == want[2]
    rq = batch.read_quality(index, front_q=10, back_q=10, maxsum_q=18, window=(4, 22), low_q=20, max_low=0.5, mean_q=20, max_ambiguous=0, min_len=16,
                            max_len=3000, max_ee=3.0)
    want = QC.batch_model(reads, QC.rules()["all_steps"])
    assert np.array_equal(rq.host(), want[0]) and rq.stats is None


def test_refusals(ctx, source):
    import torch

    import biolib_amd
    from biolib_amd import capi

    batch, index = source
    L = ctx._lib
    n = batch.n_seqs
    rec = torch.zeros((n + 1, 6), dtype=torch.int64, device="cuda")
    spans = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")
    good = capi_rule(QC.rule())
    vp = C.c_void_p

    def refused(what, b=batch._h, ix=index._h, rule=good, d_rec=rec.data_ptr(), d_spans=spans.data_ptr(), c=ctx._h):
        rc = L.bl_scan_read_quality(c, b, ix, C.byref(rule) if rule is not None else None, vp(d_rec), vp(d_spans), None)
        assert rc == capi.BL_ERR_INVALID, what
        msg = L.bl_last_error().decode()
        assert what in msg, (what, msg)

    refused("NULL", c=None)
    refused("NULL", b=None)
    refused("NULL", ix=None)
    refused("NULL", rule=None)
    for change, what in ((dict(phred_base=35), "phred_base"), (dict(quality_fill=32), "quality_fill"), (dict(quality_fill=127), "quality_fill"),
                         (dict(front_q=95), "threshold"), (dict(back_q=95), "threshold"), (dict(maxsum_front_q=95), "threshold"),
                         (dict(maxsum_back_q=95), "threshold"), (dict(window_q=95), "threshold"), (dict(low_q=95), "threshold"), (dict(mean_q=95), "threshold"),
                         (dict(window_len=65536), "window_len"), (dict(low_max_den=0), "low_max_den"), (dict(low_max_num=3, low_max_den=2), "low_max_num"),
                         (dict(reserved=1), "reserved")):
        refused(what, rule=capi_rule(QC.rule(**change)))
    refused("16-byte aligned", d_rec=rec.data_ptr() + 8)
    refused("16-byte aligned", d_spans=spans.data_ptr() + 8)
    other = biolib_amd.Context(0)
    try:
        b2, ix2 = other.from_text_indexed(b"@a\nACGT\n+\nIIII\n")
        refused("the index belongs to another context", ix=ix2._h)
        refused("the batch belongs to another context", b=b2._h)
        ix2.close()
        b2.close()
    finally:
        other.close()
    b3, ix3 = ctx.from_text_indexed(b"@a\nACGT\n+\nIIII\n")
    refused("not the one the index was built with", b=b3._h)
    refused("not the one the index was built with", ix=ix3._h)
    ix3.close()
    b3.close()
    assert not rec.any() and not spans.any(), "a refused call wrote"
    # bl_spans_intersect
    a = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")
    offs = batch._device_offsets(None)

    def refused2(what, c=ctx._h, b=batch._h, o=offs.data_ptr(), d_a=a.data_ptr(), d_b=None, flags=0, out=a.data_ptr()):
        rc = L.bl_spans_intersect(c, b, vp(o), vp(d_a), vp(d_b), flags, vp(out))
        assert rc == capi.BL_ERR_INVALID, what
        assert what in L.bl_last_error().decode(), (what, L.bl_last_error().decode())

    refused2("NULL", c=None)
    refused2("NULL", b=None)
    refused2("NULL", d_a=None)
    refused2("NULL", out=None)
    refused2("16-byte aligned", d_a=a.data_ptr() + 8)
    refused2("16-byte aligned", d_b=a.data_ptr() + 8)
    refused2("16-byte aligned", out=a.data_ptr() + 8)
    refused2("unknown flag", flags=2)
    refused2("offsets", o=None)
    odd, ixo = ctx.from_text_indexed(QC.fastq(QC.reads()[:3]))
    o3 = odd._device_offsets(None)
    rc = L.bl_spans_intersect(ctx._h, odd._h, vp(o3.data_ptr()), vp(a.data_ptr()), None, capi.SPANS_PAIRED, vp(a.data_ptr()))
    assert rc == capi.BL_ERR_INVALID and "even" in L.bl_last_error().decode()
    ixo.close()
    odd.close()


def test_spans_intersect(ctx, source, reads):
    import torch

    batch, index = source
    n = batch.n_seqs
    assert n % 2 == 0
    lengths = np.array([len(b) for _, b, _ in reads])
    rng = np.random.default_rng(17)
    a = np.sort(rng.integers(0, 400, (n, 2)), axis=1).astype(np.uint64)
    b = rng.integers(0, 400, (n, 2)).astype(np.uint64)
    i10 = int(np.nonzero(lengths >= 10)[0][0])
    a[i10], b[i10] = (lengths[i10] + 2, lengths[i10] + 9), (0, lengths[i10])   # empty only after clamping
    a[-1], b[-1] = (0, QC.U64), (1, QC.U64)
    to_dev = lambda x: torch.from_numpy(x.view(np.int64)).cuda()
    for bb in (b, None):
        for paired in (False, True):
            want = QC.intersect_model(lengths, a, bb, paired)
            got = batch.intersect_spans(to_dev(a), None if bb is None else to_dev(bb), paired)
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want), (bb is None, paired)
            # in place, with guard words behind the array
            for alias in ("a", "b") if bb is not None else ("a",):
                d_a = torch.full((n + PAD, 2), GUARD, dtype=torch.int64, device="cuda")
                d_b = torch.full((n + PAD, 2), GUARD, dtype=torch.int64, device="cuda")
                d_a[:n] = to_dev(a)
                if bb is not None:
                    d_b[:n] = to_dev(bb)
                torch.cuda.synchronize()
                out = d_a if alias == "a" else d_b
                batch.intersect_spans_raw(d_a, d_b if bb is not None else None, 1 if paired else 0, out, batch._device_offsets(None))
                ctx.sync()
                res = out.cpu().numpy()
                assert np.array_equal(res[:n].view(np.uint64), want) and (res[n:] == GUARD).all(), (bb is None, paired, alias)
    assert (QC.intersect_model(lengths, a, b)[i10] == 0).all()


def parse_records(text):
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def test_paired_trimming_end_to_end(pairs, tmp_path):
    """interleaved mates with degraded tails and Ns: trim_by_quality(paired=True), then the plain and the BGZF writer; names, bases and
    qualities of every record are the model's slices and mates are still interleaved"""
    batch, index, rs, _ = pairs
    how = dict(window=(4, 20), low_q=15, max_low=(2, 5), min_len=50, max_ambiguous=1)
    r = QC.rule(window_len=4, window_q=20, low_q=15, low_max_num=2, low_max_den=5, min_len=50, max_ambiguous=1)
    _, w_spans, _ = QC.batch_model(rs, r)
    w_spans = QC.intersect_model([150] * len(rs), w_spans, None, paired=True)
    dropped = int((w_spans[:, 1] == 0).sum())
    assert 0 < dropped < len(rs) and dropped % 2 == 0 and (w_spans[:, 0] != 0).sum() == 0 and ((w_spans[:, 1] != 0) & (w_spans[:, 1] != 150)).any()
    out, source_index, spans, rq = batch.trim_by_quality(index, paired=True, **how)
    assert np.array_equal(spans.cpu().numpy().view(np.uint64), w_spans)
    assert out.n_seqs == len(rs) and np.array_equal(source_index.cpu().numpy(), np.arange(len(rs)))
    out.write(str(tmp_path / "out.fq"), index=index, source_index=source_index, spans=spans)
    out.write(str(tmp_path / "out.fq.gz"), compress=True, index=index, source_index=source_index, spans=spans)
    plain = (tmp_path / "out.fq").read_bytes()
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == plain
    got = parse_records(plain)
    assert len(got) == len(rs)
    for i, ((name, bases, qual), (g_name, g_bases, g_qual)) in enumerate(zip(rs, got)):
        b, e = int(w_spans[i, 0]), int(w_spans[i, 1])
        assert (g_name, g_bases, g_qual) == (name, bases[b:e], qual[b:e]), i
        assert g_name.endswith(b"/%d" % (i % 2 + 1)) and (len(g_bases) == 0) == (len(got[i ^ 1][1]) == 0), "mates in step"
    # without keep_empty both mates go: the result is still interleaved
    out2, src2, _, _ = batch.trim_by_quality(index, paired=True, keep_empty=False, **how)
    s2 = src2.cpu().numpy()
    assert out2.n_seqs == len(rs) - dropped and (s2[0::2] % 2 == 0).all() and (s2[1::2] == s2[0::2] + 1).all()
