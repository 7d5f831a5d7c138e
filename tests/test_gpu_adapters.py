"""GPU tests of bl_scan_read_adapters and its Python binding (Batch.read_adapters_raw / read_adapters / trim_adapters): every named case of
the model (adapter_cases.py; the lane bodies were run under the sanitizers in test_emu_adapters.py) word for word with guard words behind
every output, batches without a packed copy, a fixed-length batch of 1,002 reads and a ragged one, reruns, partial outputs, every
refusal with its message, and paired trimming after read_quality end to end through the writers."""
import ctypes as C
import gzip

import numpy as np
import pytest

import adapter_cases as AC
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
def results():
    """the model's answer to every named case, computed once and left unchanged"""
    return {name: AC.batch_model(reads, r, spans) for name, (reads, r, spans) in AC.cases().items()}


def upload(ctx, reads):
    lay = AC.layout(reads)
    return ctx.upload(lay["bases"], offsets=lay["offsets"])


def capi_rule(r):
    from biolib_amd import capi

    return r if isinstance(r, C.Structure) else capi.AdapterRule.from_buffer_copy(AC.rule_struct(r).tobytes())


def call(batch, r, spans_in=None, records=True, spans=True, stats=True):
    """the C call with guarded outputs -> (records, spans, stats) as the model's"""
    import torch

    from biolib_amd import capi

    n = batch.n_seqs
    d_rec = torch.full((n + PAD, 4), GUARD, dtype=torch.int64, device="cuda")
    d_spans = torch.full((n + PAD, 2), GUARD, dtype=torch.int64, device="cuda")
    d_in = None if spans_in is None else torch.from_numpy(np.ascontiguousarray(spans_in, np.uint64).view(np.int64)).cuda()
    st = capi.AdapterStats()
    torch.cuda.synchronize()  # the raw call runs on the context's stream: torch's fills are complete first
    batch.read_adapters_raw(capi_rule(r), d_rec if records else None, d_spans if spans else None, st if stats else None, d_in, batch._device_offsets(None))
    batch.ctx.sync()
    rec, sp = d_rec.cpu().numpy(), d_spans.cpu().numpy()
    assert (rec[n if records else 0:] == GUARD).all() and (sp[n if spans else 0:] == GUARD).all(), "written behind or into an output it was not given"
    return (rec[:n].view(AC.RECORD).reshape(-1) if records else None, sp[:n].view(np.uint64) if spans else None, st.as_dict() if stats else None)


def same(got, want, reads, tag):
    recs, spans, stats = got
    w_recs, w_spans, w_stats = want
    bad = np.nonzero(recs != w_recs)[0]
    assert len(bad) == 0, (tag, [(int(i), len(reads[i]), recs[i], w_recs[i]) for i in bad[:4]])
    assert np.array_equal(spans, w_spans), tag
    assert stats == w_stats, tag


@pytest.mark.parametrize("name", sorted(AC.cases()))
def test_named_cases(ctx, results, name):
    """ragged reads of 0 .. 5,000 bases around every boundary of the kernel (16, 32, 64, 512, 1,024), adapters of 1 .. 64 bases whole, cut by
    the read's end at the least overlap and one below, with mismatches at and above the allowance, invalid bases in and beside a match,
    eight adapters with both tie rules, mates of every geometry, poly tails with a mismatch at every place, input spans of every kind"""
    reads, r, spans_in = AC.cases()[name]
    batch = upload(ctx, reads)
    same(call(batch, r, spans_in), results[name], reads, name)
    batch.close()


@pytest.mark.parametrize("how", ["option", "borrowed"])
def test_without_a_packed_copy(ctx, results, how):
    """bl_ctx_set_option("packed_codes", 0) and borrowed device memory both give a batch without a packed copy: every chunk from ASCII"""
    import torch

    try:
        if how == "option":
            ctx.set_option("packed_codes", 0)
        for name in ("lengths", "pair_all_steps", "poly_any", "spans_in", "adapter33"):
            reads, r, spans_in = AC.cases()[name]
            lay = AC.layout(reads)
            if how == "option":
                batch = upload(ctx, reads)
            else:
                t = torch.from_numpy(np.frombuffer(lay["bases"], np.uint8).copy()).cuda()
                batch = ctx.from_tensor(t, offsets=lay["offsets"])
            same(call(batch, r, spans_in), results[name], reads, (how, name))
            batch.close()
    finally:
        ctx.set_option("packed_codes", 1)


def test_all_byte_values(ctx):
    rng = np.random.default_rng(29)
    reads, r, _ = AC.cases()["pair_all_steps"]
    rs = []
    for x in reads:
        y = np.frombuffer(x, np.uint8).copy()
        where = rng.random(len(y)) < 0.06
        y[where] = rng.integers(0, 256, int(where.sum()))
        rs.append(y.tobytes())
    rs += [bytes(range(256)), bytes(range(255, -1, -1))]
    batch = upload(ctx, rs)
    same(call(batch, r), AC.batch_model(rs, r), rs, "bytes")
    batch.close()


def thousand_reads():
    """501 pairs of 150-bp mates: read-through of every insert size in a third of them, poly-G tails, Ns"""
    rng = np.random.default_rng(41)
    reads = []
    for k in range(501):
        I = int(rng.integers(20, 150)) if k % 3 == 0 else int(rng.integers(150, 400))
        r1, r2 = AC.mates(I, 150, 150, 9000 + 3 * k, errors=int(rng.integers(0, 3)) if I > 40 else 0)
        r1, r2 = bytearray(r1), bytearray(r2)
        if k % 7 == 0:
            t = int(rng.integers(5, 40))
            r2[150 - t:] = b"G" * t
        if k % 11 == 0:
            r1[int(rng.integers(0, 150))] = ord("N")
        reads += [bytes(r1), bytes(r2)]
    return reads


FULL = dict(flags=AC.PAIRED, adapters=[AC.TRUSEQ, AC.ADAPTERS["nextera"]], poly_before=AC.poly_mask(b"G"), poly_after=AC.poly_mask(b"G"), min_len=25)


def test_fixed_length_and_ragged_batches(ctx):
    """1,002 reads of 150 bp as a fixed-length batch (no offsets; the count is no multiple of the waves of a workgroup), and the same
    reads with two shorter ones in front as a ragged batch: every read starts elsewhere in its 16-base chunk"""
    reads = thousand_reads()
    r = AC.rule(**FULL)
    want = AC.batch_model(reads, r)
    assert want[2]["n_pair"] > 100 and want[2]["n_adapter"] > 50 and want[2]["n_poly_before"] + want[2]["n_poly_after"] > 20 and want[2]["n_too_short"] > 0
    batch = ctx.upload(b"".join(reads), read_len=150)
    assert batch.n_seqs == 1002 and batch.read_len == 150
    same(call(batch, r), want, reads, "fixed")
    single = dict(r, flags=0)
    same(call(batch, single), AC.batch_model(reads, single), reads, "fixed, single")
    batch.close()
    ragged = [AC.dna(7, 1), AC.dna(38, 2)] + reads
    batch = upload(ctx, ragged)
    same(call(batch, r), AC.batch_model(ragged, r), ragged, "ragged")
    batch.close()


def test_reruns_and_partial_outputs(ctx, results):
    reads, r, spans_in = AC.cases()["pair_all_steps"]
    batch = upload(ctx, reads)
    first = call(batch, r)
    again = call(batch, r)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    only_records = call(batch, r, spans=False, stats=False)
    only_spans = call(batch, r, records=False, stats=False)
    assert only_records[0].tobytes() == first[0].tobytes() and only_spans[1].tobytes() == first[1].tobytes()
    nothing = call(batch, r, records=False, spans=False)
    assert nothing[2] == first[2] == results["pair_all_steps"][2]
    batch.close()


def test_python_binding(ctx, results):
    import torch

    import biolib_amd

    assert biolib_amd.ADAPTERS == {k: v.decode() for k, v in AC.ADAPTERS.items()}
    reads, r, _ = AC.cases()["pair_all_steps"]
    batch = upload(ctx, reads)
    ra = batch.read_adapters([biolib_amd.ADAPTERS["truseq"], biolib_amd.ADAPTERS["nextera"]], paired=True, poly_before="G", poly_after="G", min_len=31,
                             stats=True)
    want = results["pair_all_steps"]
    assert np.array_equal(ra.host(), want[0]) and np.array_equal(ra.spans.cpu().numpy().view(np.uint64), want[1]) and ra.stats == want[2]
    batch.close()
    reads, r, spans_in = AC.cases()["spans_in"]
    batch = upload(ctx, reads)
    clamped = np.minimum(spans_in, np.uint64(1 << 62)).view(np.int64)   # (as int64 tensors; the clamp to the read is the library's)
    ra = batch.read_adapters("AGATCGGAAGAGC", spans=torch.from_numpy(clamped).cuda(), max_error=(1, 10), poly_before="g", poly_after=b"G", min_len=20)
    want = AC.batch_model(reads, r, clamped.view(np.uint64))
    assert np.array_equal(ra.host(), want[0]) and np.array_equal(ra.spans.cpu().numpy().view(np.uint64), want[1]) and ra.stats is None
    with pytest.raises(ValueError):
        batch.read_adapters(poly_before="N")
    batch.close()


def test_refusals(ctx):
    import torch

    import biolib_amd
    from biolib_amd import capi

    reads = [AC.dna(30, 1), AC.dna(31, 2), AC.dna(32, 3)]
    batch = upload(ctx, reads)
    L = ctx._lib
    n = batch.n_seqs
    rec = torch.zeros((n + 1, 4), dtype=torch.int64, device="cuda")
    spans = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")
    offs = batch._device_offsets(None)
    good = AC.rule(adapters=[AC.TRUSEQ])
    vp = C.c_void_p

    def refused(what, b=batch._h, o=offs.data_ptr(), d_in=None, rule=good, d_rec=rec.data_ptr(), d_spans=spans.data_ptr(), c=ctx._h, **fields):
        if rule is not None:
            s = AC.rule_struct(rule)
            for k, x in fields.items():
                s[k] = x
            rule = capi.AdapterRule.from_buffer_copy(s.tobytes())
        rc = L.bl_scan_read_adapters(c, b, vp(o), vp(d_in), C.byref(rule) if rule is not None else None, vp(d_rec), vp(d_spans), None)
        assert rc == capi.BL_ERR_INVALID, what
        msg = L.bl_last_error().decode()
        assert what in msg, (what, msg)

    assert L.bl_scan_read_adapters(ctx._h, batch._h, vp(offs.data_ptr()), None, C.byref(capi_rule(good)), None, None, None) == capi.BL_OK
    refused("NULL", c=None)
    refused("NULL", b=None)
    refused("NULL", rule=None)
    refused("offsets", o=None)
    refused("unknown flag", flags=2)
    refused("even", flags=1)
    refused("n_adapters", n_adapters=9)
    refused("1 .. 64", adapter_len=[0] * 8)
    refused("1 .. 64", adapter_len=[65] + [0] * 7)
    refused("ACGTUacgtu", rule=AC.rule(adapters=[b"ACGN"]))
    refused("ACGTUacgtu", rule=AC.rule(adapters=[AC.TRUSEQ, b"AC-T"]))
    refused("min_overlap", min_overlap=0)
    refused("error_den", error_den=0)
    refused("error_num", error_num=11)
    refused("pair_error_den", pair_error_den=0)
    refused("pair_error_num", pair_error_num=6)
    refused("poly mask", poly_before=16)
    refused("poly mask", poly_after=17)
    refused("poly_min_len", poly_after=1, poly_min_len=0)
    refused("reserved", reserved=1)
    refused("16-byte aligned", d_rec=rec.data_ptr() + 8)
    refused("16-byte aligned", d_spans=spans.data_ptr() + 8)
    refused("16-byte aligned", d_in=spans.data_ptr() + 8)
    even = upload(ctx, reads + [b"ACGT"])
    refused("pair_min_overlap", b=even._h, o=even._device_offsets(None).data_ptr(), rule=AC.rule(flags=1), pair_min_overlap=0)
    even.close()
    other = biolib_amd.Context(0)
    try:
        b2 = other.upload(b"ACGT")
        refused("the batch belongs to another context", b=b2._h, o=None)
        b2.close()
    finally:
        other.close()
    ctx.sync()
    assert not rec.any() and not spans.any(), "a refused call wrote"
    batch.close()


def test_trim_adapters_after_read_quality_end_to_end(ctx, tmp_path):
    """interleaved mates with read-through, poly-G tails, degraded qualities and Ns: read_quality, then trim_adapters(paired=True) on its
    spans, then the plain and the BGZF writer; names, bases and qualities of every record are the models' slices, mates interleaved"""
    reads = thousand_reads()[:400]
    rng = np.random.default_rng(43)
    rs = []
    for i, x in enumerate(reads):
        good = int(rng.integers(60, 151)) if rng.random() < 0.5 else 150
        v = np.concatenate([rng.integers(30, 41, good), rng.integers(2, 18, 150 - good)])
        rs.append((b"pair%d/%d" % (i // 2, i % 2 + 1), x, QC.q33(v)))
    batch, index = ctx.from_text_indexed(QC.fastq(rs))
    assert batch.n_seqs == 400 and batch.read_len == 150
    q_rule = QC.rule(window_len=4, window_q=20, min_len=30)
    _, q_spans, _ = QC.batch_model(rs, q_rule)
    a_rule = AC.rule(**dict(FULL, min_len=60))
    w_recs, a_spans, _ = AC.batch_model(reads, a_rule, q_spans)
    w_spans = QC.intersect_model([150] * len(rs), a_spans, None, paired=True)
    dropped = int((w_spans[:, 1] == 0).sum())
    assert 0 < dropped < len(rs) and dropped % 2 == 0 and (w_recs["cut"] & 2).any() and (w_recs["cut"] & 4).any() and (w_recs["cut"] & 9).any()
    assert (q_spans[:, 1] < 150).any() and (a_spans[:, 1] < q_spans[:, 1]).any()

    rq = batch.read_quality(index, window=(4, 20), min_len=30)
    out, source_index, spans, ra = batch.trim_adapters([AC.TRUSEQ, AC.ADAPTERS["nextera"]], paired=True, spans=rq.spans, poly_before="G", poly_after="G",
                                                       min_len=60)
    assert np.array_equal(ra.host(), w_recs) and np.array_equal(spans.cpu().numpy().view(np.uint64), w_spans)
    assert out.n_seqs == len(rs) and np.array_equal(source_index.cpu().numpy(), np.arange(len(rs)))
    out.write(str(tmp_path / "out.fq"), index=index, source_index=source_index, spans=spans)
    out.write(str(tmp_path / "out.fq.gz"), compress=True, index=index, source_index=source_index, spans=spans)
    plain = (tmp_path / "out.fq").read_bytes()
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == plain
    got = QC.parse_fastq(plain)
    assert len(got) == len(rs)
    for i, ((name, bases, qual), (g_name, g_bases, g_qual)) in enumerate(zip(rs, got)):
        b, e = int(w_spans[i, 0]), int(w_spans[i, 1])
        assert (g_name, g_bases, g_qual) == (name, bases[b:e], qual[b:e]), i
        assert (len(g_bases) == 0) == (len(got[i ^ 1][1]) == 0), "mates in step"
    # without keep_empty both mates go: the result is still interleaved
    out2, src2, _, _ = batch.trim_adapters([AC.TRUSEQ, AC.ADAPTERS["nextera"]], paired=True, spans=rq.spans, keep_empty=False, poly_before="G", poly_after="G",
                                           min_len=60)
    s2 = src2.cpu().numpy()
    assert out2.n_seqs == len(rs) - dropped and (s2[0::2] % 2 == 0).all() and (s2[1::2] == s2[0::2] + 1).all()
    index.close()
    batch.close()
