"""GPU tests of bl_batch_select / bl_read_spans and their Python binding (Batch.select_raw / select / read_spans / trim_by_counts): every
case of the model (select_cases.py: each index path was run under the sanitizers in test_emu_select.py) byte for byte, the result used as
a batch by scans this feature does not touch, refusals, a source without slack, and abundance trimming end to end."""
import numpy as np
import pytest

import select_cases as SC

pytestmark = pytest.mark.gpu
PAD = 8          # guard entries behind both outputs
GUARD = -0x3A3A3A3A3A3A3A3B  # 0xC5C5...C5 as int64


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    b = SC.batch()
    return b, SC.self_check(b)


def source_of(ctx, v):
    if v["offs"] is not None:
        return ctx.upload(v["bases"], v["offs"])
    return ctx.upload(v["bases"], read_len=v["read_len"]) if v["read_len"] else ctx.upload(v["bases"])


def dev_u64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def select_raw(ctx, src, spans, keep_empty, offsets, outputs=True):
    """the C call with guarded outputs -> (model-shaped dict, Batch)"""
    import torch

    from biolib_amd.scan import Batch

    n_seqs = src.n_seqs
    d_spans = dev_u64(np.asarray(spans, np.uint64).reshape(-1, 2)) if n_seqs else torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    out_offsets = torch.full((n_seqs + 1 + PAD,), GUARD, dtype=torch.int64, device="cuda")
    source_index = torch.full((n_seqs + PAD,), GUARD, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # the raw call runs on the context's stream: torch's fills are complete first
    h, n_out, n_bases = src.select_raw(d_spans, 1 if keep_empty else 0, None if offsets is None else dev_u64(offsets), out_offsets if outputs else None,
                                       source_index if outputs else None)
    offs, index = out_offsets.cpu().numpy(), source_index.cpu().numpy()
    if outputs:
        assert (offs[n_out + 1:] == GUARD).all() and (index[n_out:] == GUARD).all(), "written behind an output"
    else:
        assert (offs == GUARD).all() and (index == GUARD).all()
    out = Batch(ctx, h)
    assert out.n_bases == n_bases and out.n_seqs == n_out
    got = dict(bases=out.download(), offsets=offs[:n_out + 1].view(np.uint64), source_index=index[:n_out].view(np.uint64), n_seqs=n_out, n_bases=n_bases)
    return got, out


def same(got, want, tag, names=None, arrays=True):
    assert (got["n_seqs"], got["n_bases"]) == (want["n_seqs"], want["n_bases"]), tag
    if arrays:
        assert np.array_equal(got["source_index"], want["source_index"]), tag
        assert np.array_equal(got["offsets"], want["offsets"]), tag
    bad = np.nonzero(got["bases"] != want["bases"])[0]
    if len(bad):
        seq = int(np.searchsorted(want["offsets"], bad[0], side="right")) - 1
        src = int(want["source_index"][seq])
        raise AssertionError((tag, "first wrong byte", int(bad[0]), "of", len(bad), "result sequence", seq, names[src] if names else src))


def digests(ctx, b, table):
    """what three scans make of a batch: the k-mer digest, the minimizer records, the table counts"""
    km = b.kmers(21, seed=3, canonical=True, arrays=False)
    mm = b.minimizers(15, 9, seed=5, canonical=True)
    counts, kc = b.kmer_counts(table, 21, canonical=True)
    return km, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in mm.items()}, kc, counts.cpu().numpy().tolist()


def table_of(ctx, b, k):
    import torch

    from biolib_amd.scan import _flags

    n = b.n_bases
    vals = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    b.kmers128_raw(k, 0, _flags(True, False, True), 0, 0, vals, None, ok)
    keys = vals[ok == 1].contiguous()
    uniq, mult = ctx.sort_count128(keys, key_bits=2 * k)
    return ctx.count_table(uniq if k > 32 else uniq[:, 0].contiguous(), mult, key_bits=2 * k)


def test_case_batch_byte_for_byte(ctx, cases):
    b, want = cases
    src = ctx.upload(b["bases"], b["offs"])
    before = src.download()
    got, out = select_raw(ctx, src, b["spans"], False, b["offs"])
    same(got, want, "cases", b["names"])
    again, out2 = select_raw(ctx, src, b["spans"], False, b["offs"])
    same(again, want, "cases again", b["names"])
    bare, out3 = select_raw(ctx, src, b["spans"], False, b["offs"], outputs=False)  # every nullable output NULL
    same(bare, want, "no outputs", b["names"], arrays=False)
    assert np.array_equal(src.download(), before) and np.array_equal(before, b["bases"]), "the source batch is unchanged"
    for x in (out, out2, out3, src):
        x.close()


@pytest.mark.parametrize("name", sorted(SC.variants()))
def test_variants_byte_for_byte(ctx, name):
    v = SC.variants()[name]
    want = SC.expected(v)
    src = source_of(ctx, v)
    assert src.n_seqs == len(v["spans"])
    got, out = select_raw(ctx, src, v["spans"], v["keep_empty"], v["offs"])
    same(got, want, name)
    if name.startswith("all_dropped"):
        assert out.n_bases == 0 and out.n_seqs == (len(v["spans"]) if v["keep_empty"] else 0) and len(out.download()) == 0
    out.close()
    # the binding: offsets kept on both sides, read_len where the result is fixed-length
    new, index = src.select(dev_u64(v["spans"]).view(-1, 2), keep_empty=v["keep_empty"])
    assert np.array_equal(new.offsets, want["offsets"]) and new.read_len == want["fixed_len"]
    assert np.array_equal(new._d_offsets.cpu().numpy().view(np.uint64), want["offsets"])
    assert np.array_equal(index.cpu().numpy().view(np.uint64), want["source_index"])
    assert np.array_equal(new.download(), want["bases"])
    new.close()
    src.close()


@pytest.mark.parametrize("name", sorted(SC.scale_variants()))
def test_scale_variants_byte_for_byte(ctx, name):
    """the wave's 64-ary search at depths 0 .. 4, the switch between its two lookups at 62, 63 and 64 lane offsets, runs of 64 and more
    empty kept sequences, totals around a wave's bytes (select_cases.scale_variants; the emulation ran each under the sanitizers)"""
    v = SC.scale_variants()[name]
    want = SC.expected(v)
    inside = SC.scale_self_check(name, v, want)
    print(name, dict(n_out=want["n_seqs"], n_bases=want["n_bases"], depth=SC.search_depth(want["n_seqs"]), paths=SC.wave_paths(want["offsets"]),
                     inside=sorted(set(inside.tolist()))[-3:]))
    src = source_of(ctx, v)
    assert src.n_seqs == len(v["spans"])
    got, out = select_raw(ctx, src, v["spans"], v["keep_empty"], v["offs"])
    same(got, want, name)
    out.close()
    again, out = select_raw(ctx, src, v["spans"], v["keep_empty"], v["offs"])
    assert np.array_equal(again["bases"], got["bases"]), "two runs give the same bytes"
    out.close()
    # the binding: offsets kept on both sides, read_len where the result is fixed-length
    new, index = src.select(dev_u64(v["spans"]).view(-1, 2), keep_empty=v["keep_empty"])
    assert np.array_equal(new.offsets, want["offsets"]) and new.read_len == want["fixed_len"]
    assert np.array_equal(index.cpu().numpy().view(np.uint64), want["source_index"])
    assert np.array_equal(new.download(), want["bases"])
    new.close()
    src.close()


def test_a_deep_search_on_a_source_without_slack(ctx):
    """depth_4097 (three steps of the search) from a tensor of exactly n_bases bytes"""
    import torch

    v = SC.scale_variants()["depth_4097"]
    want = SC.expected(v)
    t = torch.from_numpy(v["bases"].copy()).cuda()
    assert t.numel() == len(v["bases"]) and t.data_ptr() % 16 == 0 and SC.search_depth(want["n_seqs"]) == 3
    src = ctx.from_tensor(t, read_len=v["read_len"])
    assert src.n_seqs == len(v["spans"])
    got, out = select_raw(ctx, src, v["spans"], v["keep_empty"], None)
    same(got, want, "depth_4097 from_device")
    assert torch.equal(t.cpu(), torch.from_numpy(v["bases"])), "the source tensor is unchanged"
    out.close()
    src.close()


@pytest.mark.parametrize("name", ("cases", "keep_empty", "result_fixed", "result_just_not_fixed", "fixed_source"))
def test_the_result_is_a_batch_for_every_scan(ctx, cases, name):
    """kmers, minimizers and kmer_counts on the selected batch equal those on an upload of the model's bases and offsets"""
    b, _ = cases
    v = dict(bases=b["bases"], offs=b["offs"], read_len=0, spans=b["spans"], keep_empty=False) if name == "cases" else SC.variants()[name]
    want = SC.expected(v)
    src = source_of(ctx, v)
    new, _ = src.select(dev_u64(v["spans"]).view(-1, 2), keep_empty=v["keep_empty"])
    ref = ctx.upload(want["bases"], want["offsets"])
    assert (new.n_seqs, new.n_bases) == (ref.n_seqs, ref.n_bases)
    table = table_of(ctx, ref, 21)
    assert digests(ctx, new, table) == digests(ctx, ref, table)
    if want["fixed_len"]:
        assert new.read_len == want["fixed_len"] and ref.n_seqs == want["n_seqs"]
    # read_counts and read_quantiles take the new batch as it is: its offsets travel with it
    rc_new, rc_ref = new.read_counts(table, 21, canonical=True)[0].host(), ref.read_counts(table, 21, canonical=True)[0].host()
    assert np.array_equal(rc_new, rc_ref)
    q_new, q_ref = new.read_quantiles(table, 21, canonical=True), ref.read_quantiles(table, 21, canonical=True)
    assert np.array_equal(q_new[0].cpu().numpy(), q_ref[0].cpu().numpy()) and np.array_equal(q_new[1].cpu().numpy(), q_ref[1].cpu().numpy())
    for x in (table, new, ref, src):
        x.close()


def test_a_source_without_slack(ctx, cases):
    """bl_batch_from_device around a tensor of exactly n_bases bytes: the same answer, also where a span ends at the tensor's last byte"""
    import torch

    b, want = cases
    t = torch.from_numpy(b["bases"].copy()).cuda()
    assert t.numel() == len(b["bases"]) and t.data_ptr() % 16 == 0
    src = ctx.from_tensor(t, offsets=b["offs"])
    got, out = select_raw(ctx, src, b["spans"], False, b["offs"])
    same(got, want, "from_device", b["names"])
    assert torch.equal(t.cpu(), torch.from_numpy(b["bases"])), "the source tensor is unchanged"
    out.close()
    src.close()
    for n in (1, 15, 16, 17, 4099):  # one sequence, whole: the tail bytes come from byte loads
        t = torch.from_numpy(b["bases"][:n].copy()).cuda()
        src = ctx.from_tensor(t)
        got, out = select_raw(ctx, src, [[0, SC.U64]], False, None)
        assert np.array_equal(got["bases"], b["bases"][:n]), n
        out.close()
        src.close()


def test_wrong_offsets_follow_the_clamping_rule(ctx, cases):
    """the safety rule is also the answer: offsets clamped to [0, n_bases], a decreasing pair is an empty read"""
    b, _ = cases
    src = ctx.upload(b["bases"], b["offs"])
    rng = np.random.default_rng(1)
    bad, garbage = SC.wrong_offsets(b["offs"], rng), SC.garbage_spans(len(b["spans"]), rng)
    got, out = select_raw(ctx, src, garbage, True, bad)
    same(got, SC.select_model(b["bases"], bad, garbage, True), "wrong offsets, garbage spans")
    assert np.array_equal(src.download(), b["bases"])
    out.close()
    src.close()


def test_refusals_launch_nothing(ctx, cases):
    import ctypes as C

    import torch

    import biolib_amd

    b, _ = cases
    src = ctx.upload(b["bases"], b["offs"])
    n_seqs = src.n_seqs
    spans, offs = dev_u64(b["spans"]), dev_u64(b["offs"])
    out_offsets = torch.full((n_seqs + 1,), GUARD, dtype=torch.int64, device="cuda")
    source_index = torch.full((n_seqs,), GUARD, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lib = ctx._lib

    def invalid(call):
        with pytest.raises(biolib_amd.BiolibError) as e:
            call()
        assert e.value.code == biolib_amd.capi.BL_ERR_INVALID, e.value
        assert len(str(e.value).split(":", 1)[1].strip()) > 0, "a message"
        return str(e.value)

    def call(c_ctx, c_batch, c_offs, c_spans, flags, c_out):
        ns, nb = C.c_uint64(7), C.c_uint64(7)
        biolib_amd.capi.check(lib.bl_batch_select(c_ctx, c_batch, c_offs, c_spans, flags, c_out, C.c_void_p(out_offsets.data_ptr()),
                                                  C.c_void_p(source_index.data_ptr()), C.byref(ns), C.byref(nb)))

    h = C.c_void_p()
    p_offs, p_spans = C.c_void_p(offs.data_ptr()), C.c_void_p(spans.data_ptr())
    invalid(lambda: call(None, src._h, p_offs, p_spans, 0, C.byref(h)))
    invalid(lambda: call(ctx._h, None, p_offs, p_spans, 0, C.byref(h)))
    invalid(lambda: call(ctx._h, src._h, p_offs, p_spans, 0, None))
    assert "spans" in invalid(lambda: call(ctx._h, src._h, p_offs, None, 0, C.byref(h)))
    assert "aligned" in invalid(lambda: call(ctx._h, src._h, p_offs, C.c_void_p(spans.data_ptr() + 8), 0, C.byref(h)))
    assert "flag" in invalid(lambda: call(ctx._h, src._h, p_offs, p_spans, 2, C.byref(h)))
    assert "offsets" in invalid(lambda: call(ctx._h, src._h, None, p_spans, 0, C.byref(h)))  # NULL offsets on a ragged batch
    other = biolib_amd.Context(0)
    assert "context" in invalid(lambda: call(other._h, src._h, p_offs, p_spans, 0, C.byref(h)))
    other.close()
    assert not h.value, "no batch was made"
    # bl_read_spans
    rc = biolib_amd.scan.ReadCounts(ctx, n_seqs)
    out = torch.full((n_seqs, 2), GUARD, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def rule(**change):
        r = biolib_amd.capi.SpanRule(trim=1, k=31, min_len=31, min_kmers=0, solid_min_num=0, solid_min_den=1, solid_max_num=1, solid_max_den=1, stat_lo=0,
                                     stat_hi=2**32 - 1, reserved=0)
        for key, val in change.items():
            setattr(r, key, val)
        return r

    for change in (dict(trim=4), dict(k=0), dict(k=65), dict(solid_min_den=0), dict(solid_min_num=2), dict(solid_max_den=0), dict(solid_max_num=3), dict(reserved=1)):
        invalid(lambda: src.read_spans_raw(rc.records, rule(**change), out, None, offs))
    invalid(lambda: src.read_spans_raw(None, rule(), out, None, offs))
    invalid(lambda: src.read_spans_raw(rc.records, rule(), None, None, offs))
    assert "offsets" in invalid(lambda: src.read_spans_raw(rc.records, rule(), out, None, None))
    ctx.sync()
    torch.cuda.synchronize()
    assert (out_offsets.cpu().numpy() == GUARD).all() and (source_index.cpu().numpy() == GUARD).all() and (out.cpu().numpy() == GUARD).all(), "nothing was written"
    src.close()


@pytest.mark.parametrize("name", sorted(SC.span_cases()[3]))
def test_read_spans_against_the_model(ctx, name):
    import torch

    lengths, records, stat, rules = SC.span_cases()
    r = rules[name]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    src = ctx.upload(np.full(int(offs[-1]), ord("A"), np.uint8), offs)
    rc = __import__("biolib_amd").scan.ReadCounts(ctx, len(lengths))
    rc.records.copy_(torch.from_numpy(records.view(np.int64).reshape(-1, 6)).cuda())
    d_stat = torch.from_numpy(stat.view(np.int32)).cuda()
    trim = {v: k for k, v in SC.TRIM.items()}[r["trim"]]
    for st, host_stat in ((d_stat, stat), (None, None)):
        spans = src.read_spans(rc, r["k"], trim, r["min_len"], r["min_kmers"], r["solid_min"], r["solid_max"], st, r["stat"])
        got = spans.cpu().numpy().view(np.uint64)
        want = SC.read_spans_model(lengths, records, r, host_stat)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (name, st is None, [(int(lengths[i]), records[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    src.close()


def planted_reads():
    """a few hundred reads of 80 .. 200 bases from one genome, each three times, and a planted error in two thirds of the first copies:
    one base changed makes up to k weak k-mers, counted once, while the k-mers it replaced still count 2 in the other copies"""
    rng = np.random.default_rng(99)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 20_000)
    reads = []
    for i in range(300):
        L = int(rng.integers(80, 201))
        s = int(rng.integers(0, len(genome) - L))
        reads.append(genome[s:s + L].copy())
    reads = reads + [r.copy() for r in reads] + [r.copy() for r in reads]
    for i, r in enumerate(reads[:300]):
        if i % 3:
            at = int(rng.integers(0, len(r)))
            r[at] = ord("ACGT"[("ACGT".index(chr(r[at])) + 1 + int(rng.integers(0, 3))) % 4])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return np.concatenate(reads), offs


@pytest.mark.parametrize("trim", ("prefix", "suffix", "longer", "none"))
def test_trim_by_counts_end_to_end(ctx, trim):
    k, min_count = 21, 2
    seq, offs = planted_reads()
    src = ctx.upload(seq, offs)
    table = table_of(ctx, src, k)
    records = src.read_counts(table, k, min_count, canonical=True)[0].host()
    lengths = np.diff(offs.astype(np.int64))
    weak = records["weak_begin"] != np.uint64(SC.U64)
    assert 150 < weak.sum() < 250, "two thirds of the first 300 reads carry a weak k-mer"
    for keep_empty in (False, True):
        r = SC.rule(trim, k, min_len=k + 10, solid_min=(1, 2))
        want_spans = SC.read_spans_model(lengths, records, r)
        want = SC.select_model(seq, offs, want_spans, keep_empty)
        new, index, rc = src.trim_by_counts(table, k, min_count, trim=trim, min_len=k + 10, solid_min=(1, 2), canonical=True, keep_empty=keep_empty)
        assert np.array_equal(rc.host(), records)
        assert np.array_equal(new.offsets, want["offsets"]) and np.array_equal(index.cpu().numpy().view(np.uint64), want["source_index"])
        assert np.array_equal(new.download(), want["bases"])
        assert 0 < want["n_bases"] < len(seq) or trim == "none"
        after = new.read_counts(table, k, min_count, canonical=True)[0].host()
        if trim == "prefix":  # khmer's cut leaves no weak k-mer behind: the first one lost its last base, the others lay behind it
            assert (after["weak_begin"] == np.uint64(SC.U64)).all() and (after["n_solid"] == after["n_kmers"]).all()
        if trim == "none":
            assert (after["weak_begin"] != np.uint64(SC.U64)).sum() > 100
        new.close()
    table.close()
    src.close()
