"""GPU tests of bl_scan_read_duplicates and its Python binding (Batch.read_duplicates_raw / read_duplicates / dedup): every named case of
the model (dedup_cases.py; the lane bodies were run under the sanitizers in test_emu_dedup.py) word for word with guard words behind
every output, batches without a packed copy, every hash width and two seeds with identical results, reruns, partial outputs, every
refusal with its message, and paired duplicate removal after read_quality and read_adapters end to end through the writers."""
import ctypes as C
import gzip

import numpy as np
import pytest

import adapter_cases as AC
import dedup_cases as DC
import quality_cases as QC

pytestmark = pytest.mark.gpu
PAD = 8
GUARD = -0x3A3A3A3A3A3A3A3B  # 0xC5C5...C5 as int64
WORK = ("n_mixed_groups", "rounds")


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def results():
    """the model's answer to every named case, computed once and left unchanged"""
    return {name: DC.batch_model(c.reads, c.rule, c.spans_in, c.scores) for name, c in DC.cases().items()}


def upload(ctx, reads, read_len=0):
    if read_len:
        return ctx.upload(b"".join(reads), read_len=read_len)
    lay = DC.layout(reads)
    return ctx.upload(lay["bases"], offsets=lay["offsets"])


def capi_rule(r):
    from biolib_amd import capi

    return r if isinstance(r, C.Structure) else capi.DedupRule.from_buffer_copy(DC.rule_struct(r).tobytes())


def call(batch, r, spans_in=None, scores=None, records=True, spans=True, stats=True):
    """the C call with guarded outputs -> (records, spans, stats, work) as the model's"""
    import torch

    from biolib_amd import capi

    n = batch.n_seqs
    n_units = n // 2 if r["flags"] & 1 else n
    d_rec = torch.full((n_units + PAD, 2), GUARD, dtype=torch.int64, device="cuda")
    d_spans = torch.full((n + PAD, 2), GUARD, dtype=torch.int64, device="cuda")
    d_in = None if spans_in is None else torch.from_numpy(np.ascontiguousarray(spans_in, np.uint64).view(np.int64)).cuda()
    d_scores = None if scores is None else torch.from_numpy(np.array([int(x) for x in scores], np.uint64).view(np.int64)).cuda()
    st = capi.DedupStats()
    torch.cuda.synchronize()  # the raw call runs on the context's stream: torch's fills are complete first
    batch.read_duplicates_raw(capi_rule(r), d_rec if records else None, d_spans if spans else None, st if stats else None, d_in, d_scores,
                              batch._device_offsets(None))
    batch.ctx.sync()
    rec, sp = d_rec.cpu().numpy(), d_spans.cpu().numpy()
    assert (rec[n_units if records else 0:] == GUARD).all() and (sp[n if spans else 0:] == GUARD).all(), "written behind or into an output it was not given"
    d = st.as_dict() if stats else None
    work = {k: d.pop(k) for k in WORK} if stats else None
    return (rec[:n_units].view(DC.RECORD).reshape(-1) if records else None, sp[:n].view(np.uint64) if spans else None, d, work)


def call_case(ctx, c, **changes):
    batch = upload(ctx, c.reads, c.read_len)
    got = call(batch, dict(c.rule, **changes), c.spans_in, c.scores)
    batch.close()
    return got


def same(got, want, tag):
    recs, spans, stats = got[:3]
    w_recs, w_spans, w_stats = want
    bad = np.nonzero(recs != w_recs)[0]
    assert len(bad) == 0, (tag, [(int(i), recs[i], w_recs[i]) for i in bad[:4]])
    assert np.array_equal(spans, w_spans), tag
    assert stats == w_stats, (tag, stats, w_stats)


@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_named_cases(ctx, results, name):
    """reads of 0 .. 5,000 bases around every boundary of the kernels (16, 32, 512), a read at every residue of the batch, keys that
    differ in one place, the five letters, reverse complements and swapped mates, prefixes, input spans of every kind, scores, every
    bin of the histogram, 1,002 reads fixed-length and ragged"""
    got = call_case(ctx, DC.cases()[name])
    same(got, results[name], name)
    assert got[3] == dict(n_mixed_groups=0, rounds=1)


@pytest.mark.parametrize("how", ["option", "borrowed"])
def test_without_a_packed_copy(ctx, results, how):
    """bl_ctx_set_option("packed_codes", 0) and borrowed device memory both give a batch without a packed copy: every word from ASCII"""
    import torch

    try:
        if how == "option":
            ctx.set_option("packed_codes", 0)
        for name in ("lengths_canonical", "pairs_canonical", "letters", "spans_in", "one_difference"):
            c = DC.cases()[name]
            lay = DC.layout(c.reads)
            if how == "option":
                batch = upload(ctx, c.reads)
            else:
                t = torch.from_numpy(np.frombuffer(lay["bases"], np.uint8).copy()).cuda()
                batch = ctx.from_tensor(t, offsets=lay["offsets"])
            same(call(batch, c.rule, c.spans_in, c.scores), results[name], (how, name))
            batch.close()
    finally:
        ctx.set_option("packed_codes", 1)


def test_all_byte_values(ctx):
    c = DC.cases()["lengths_canonical"]
    table = {}
    for x in c.reads:
        if x not in table:
            rng = np.random.default_rng(len(table))
            y = np.frombuffer(x, np.uint8).copy()
            where = rng.random(len(y)) < 0.06
            y[where] = rng.integers(0, 256, int(where.sum()))
            table[x] = y.tobytes()
    reads = [table[x] for x in c.reads] + [bytes(range(256)), bytes(range(255, -1, -1))] * 2
    assert len({b for x in reads for b in x}) == 256
    batch = upload(ctx, reads)
    same(call(batch, c.rule), DC.batch_model(reads, c.rule), "bytes")
    batch.close()


@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_hash_bits_and_seeds_change_the_work_only(ctx, results, name):
    """96, 8 and 1 bits of the hash (1 only up to 300 units) and two seeds: identical records, spans and statistics"""
    c = DC.cases()[name]
    want = results[name]
    n_classes, n_units = want[2]["n_classes"], want[2]["n_units"]
    for bits, seed in ((96, 0), (8, 0), (1, 0), (0, 0x123456789abcdef), (0, DC.U64)):
        if bits == 1 and n_units > 300:
            continue
        got = call_case(ctx, c, hash_bits=bits, seed=seed)
        same(got, want, (name, bits, seed))
        if bits in (0, 96):
            assert got[3] == dict(n_mixed_groups=0, rounds=1)
        if bits == 8 and n_classes >= 300:
            assert got[3]["n_mixed_groups"] > 0 and got[3]["rounds"] > 1
        if bits == 1 and n_classes >= 3:
            assert got[3]["n_mixed_groups"] > 0 and got[3]["rounds"] >= (n_classes + 1) // 2


def test_reruns_and_partial_outputs(ctx, results):
    for name in ("volume_pairs_canonical", "canonical_on", "spans_in_pairs"):
        c = DC.cases()[name]
        batch = upload(ctx, c.reads, c.read_len)
        first = call(batch, c.rule, c.spans_in, c.scores)
        again = call(batch, c.rule, c.spans_in, c.scores)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2] and first[3] == again[3]
        only_records = call(batch, c.rule, c.spans_in, c.scores, spans=False, stats=False)
        only_spans = call(batch, c.rule, c.spans_in, c.scores, records=False, stats=False)
        assert only_records[0].tobytes() == first[0].tobytes() and only_spans[1].tobytes() == first[1].tobytes()
        nothing = call(batch, c.rule, c.spans_in, c.scores, records=False, spans=False)
        assert nothing[2] == first[2] == results[name][2]
        mixed = call(batch, dict(c.rule, hash_bits=2), c.spans_in, c.scores, stats=False)   # (several rounds, the class order sorted, no counters)
        assert mixed[0].tobytes() == first[0].tobytes() and mixed[1].tobytes() == first[1].tobytes()
        batch.close()


def test_python_binding(ctx, results):
    import torch

    c = DC.cases()["canonical_on"]
    batch = upload(ctx, c.reads)
    scores = torch.from_numpy(np.array(c.scores, np.int64)).cuda()
    rd = batch.read_duplicates(canonical=True, scores=scores, stats=True)
    want = results["canonical_on"]
    assert rd.n_units == len(c.reads) and np.array_equal(rd.host(), want[0]) and np.array_equal(rd.spans.cpu().numpy().view(np.uint64), want[1])
    assert {k: v for k, v in rd.stats.items() if k not in WORK} == want[2]
    assert np.array_equal(rd.kept_mask.cpu().numpy(), (want[0]["flags"] & DC.DUPLICATE) == 0)
    strided = torch.stack([scores, scores, scores], 1)[:, 1]   # (a column of a matrix, as read_quality's sum is)
    again = batch.read_duplicates(canonical=True, scores=strided, hash_bits=3, seed=5)
    assert np.array_equal(again.host(), want[0]) and again.stats is None
    with pytest.raises(ValueError):
        batch.read_duplicates(scores=scores[:-1])
    batch.close()
    c = DC.cases()["prefix_pairs"]
    batch = upload(ctx, c.reads)
    rd = batch.read_duplicates(paired=True, canonical=True, prefix_len=50)
    assert rd.n_units == len(c.reads) // 2 and np.array_equal(rd.host(), results["prefix_pairs"][0])
    out, source_index, spans, rd2 = batch.dedup(paired=True, canonical=True, prefix_len=50)
    keep = np.repeat((results["prefix_pairs"][0]["flags"] & (DC.DUPLICATE | DC.EMPTY)) == 0, 2)
    assert np.array_equal(source_index.cpu().numpy(), np.nonzero(keep)[0]) and out.n_seqs == int(keep.sum())
    batch.close()


def test_refusals(ctx):
    import torch

    import biolib_amd
    from biolib_amd import capi

    reads = [DC.dna(30, 1), DC.dna(31, 2), DC.dna(32, 3)]
    batch = upload(ctx, reads)
    L = ctx._lib
    n = batch.n_seqs
    rec = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")
    spans = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")
    offs = batch._device_offsets(None)
    vp = C.c_void_p

    def refused(what, b=batch._h, o=offs.data_ptr(), d_in=None, rule=True, d_rec=rec.data_ptr(), d_spans=spans.data_ptr(), c=ctx._h, **fields):
        r = capi_rule(DC.rule(**fields)) if rule else None
        rc = L.bl_scan_read_duplicates(c, b, vp(o), vp(d_in), None, C.byref(r) if r is not None else None, vp(d_rec), vp(d_spans), None)
        assert rc == capi.BL_ERR_INVALID, what
        msg = L.bl_last_error().decode()
        assert what in msg, (what, msg)

    assert L.bl_scan_read_duplicates(ctx._h, batch._h, vp(offs.data_ptr()), None, None, C.byref(capi_rule(DC.rule())), None, None, None) == capi.BL_OK
    refused("NULL", c=None)
    refused("NULL", b=None)
    refused("NULL", rule=False)
    refused("offsets", o=None)
    refused("unknown flag", flags=4)
    refused("even", flags=DC.PAIRED)
    refused("hash_bits", hash_bits=97)
    refused("reserved", reserved=1)
    refused("16-byte aligned", d_rec=rec.data_ptr() + 8)
    refused("16-byte aligned", d_spans=spans.data_ptr() + 8)
    refused("16-byte aligned", d_in=spans.data_ptr() + 8)
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


def test_dedup_after_read_quality_and_read_adapters_end_to_end(ctx, tmp_path):
    """interleaved mates, a third of the pairs copies of earlier ones with other qualities (some with the mates swapped): read_quality,
    read_adapters on its spans, dedup(paired=True) on those with the quality sums as scores, then the plain and the BGZF writer; the
    written reads are the model's kept reads, names and qualities theirs"""
    rng = np.random.default_rng(47)
    pairs = []
    for k in range(150):
        if k >= 40 and k % 3 == 0:
            r1, r2 = pairs[int(rng.integers(0, 40))]
            pairs.append((r2, r1) if k % 2 else (r1, r2))
        else:
            pairs.append(AC.mates(int(rng.integers(160, 400)), 150, 150, 12000 + 3 * k, errors=0))
    rs = []
    for k, pair in enumerate(pairs):
        for m, x in enumerate(pair):
            v = rng.integers(30, 41, 150) if k < 40 else rng.integers(31, 42, 150)
            rs.append((b"pair%d/%d" % (k, m + 1), bytes(x), QC.q33(v)))
    reads = [x for _, x, _ in rs]
    batch, index = ctx.from_text_indexed(QC.fastq(rs))
    assert batch.n_seqs == 300 and batch.read_len == 150
    q_rule = QC.rule(back_q=31, min_len=30)
    q_recs, q_spans, _ = QC.batch_model(rs, q_rule)
    a_rule = AC.rule(flags=AC.PAIRED, adapters=[AC.TRUSEQ], min_len=60)
    _, a_spans, _ = AC.batch_model(reads, a_rule, q_spans)
    d_rule = DC.rule(flags=DC.PAIRED | DC.CANONICAL, prefix_len=100)
    scores = [int(x) for x in q_recs["sum"]]
    w_recs, d_spans, w_stats = DC.batch_model(reads, d_rule, a_spans, scores)
    w_spans = QC.intersect_model([150] * len(rs), d_spans, None, paired=True)
    kept = np.nonzero(w_spans[:, 1] > w_spans[:, 0])[0]
    assert w_stats["n_duplicates"] >= 30 and (w_recs["kept"] != w_recs["first"]).any() and (w_recs["flags"] & DC.REVERSED).any()
    assert (q_spans[:, 1] < 150).any() and 0 < len(kept) < len(rs)

    rq = batch.read_quality(index, back_q=31, min_len=30)
    ra = batch.read_adapters([AC.TRUSEQ], paired=True, spans=rq.spans, min_len=60)
    out, source_index, spans, rd = batch.dedup(paired=True, spans=ra.spans, scores=rq.records[:, 2], canonical=True, prefix_len=100, stats=True)
    assert np.array_equal(rd.host(), w_recs) and np.array_equal(spans.cpu().numpy().view(np.uint64), w_spans)
    assert {k: v for k, v in rd.stats.items() if k not in WORK} == w_stats
    assert out.n_seqs == len(kept) and np.array_equal(source_index.cpu().numpy(), kept)
    out.write(str(tmp_path / "out.fq"), index=index, source_index=source_index, spans=spans)
    out.write(str(tmp_path / "out.fq.gz"), compress=True, index=index, source_index=source_index, spans=spans)
    plain = (tmp_path / "out.fq").read_bytes()
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == plain
    got = QC.parse_fastq(plain)
    assert len(got) == len(kept)
    for i, (g_name, g_bases, g_qual) in zip(kept, got):
        name, bases, qual = rs[i]
        b, e = int(w_spans[i, 0]), int(w_spans[i, 1])
        assert (g_name, g_bases, g_qual) == (name, bases[b:e], qual[b:e]), i
    s = source_index.cpu().numpy()
    assert (s[0::2] % 2 == 0).all() and (s[1::2] == s[0::2] + 1).all(), "mates in step"
    index.close()
    batch.close()
