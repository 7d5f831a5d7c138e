"""GPU tests of bl_select_read_counts and its Python binding (Batch.select_read_counts_raw / read_quantiles / read_medians): every case of
the model (read_quantiles_cases.py: each index path was run under the sanitizers in test_emu_read_quantiles.py) on device arrays, and
end to end against the model applied to Batch.kmer_counts and against Batch.read_counts — code this feature does not touch.  Exact
equality everywhere."""
import numpy as np
import pytest

import read_quantiles_cases as QC

pytestmark = pytest.mark.gpu
PAD = 8  # guard entries behind both outputs


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    """the model's batch: any bases will do, the call reads none of them"""
    b = QC.batch()
    QC.self_check(b)
    batch = ctx.upload(np.full(len(b["counts"]), ord("A"), np.uint8), b["offs"])
    assert batch.n_seqs == len(b["offs"]) - 1
    yield b, batch
    batch.close()


def dev(a, dtype, shift=0):
    """the array on the device, `shift` elements behind a 16-byte boundary"""
    import torch

    t = torch.empty(len(a) + shift + 1, dtype=dtype, device="cuda")
    view = t[shift:shift + len(a)]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if dtype == torch.int32 else np.uint8)))
    assert (view.data_ptr() - t.data_ptr()) == shift * t.element_size() and t.data_ptr() % 16 == 0
    return view


def guards(n):
    import torch

    return torch.full((n + PAD,), QC.GUARD - (1 << 32), dtype=torch.int32, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint32)


def select(batch, b, first, n, quantiles, shift=0, offsets="given", n_kmers=True):
    """the call over counts[first:end] -> (quantiles [n_seqs, n_q], n_kmers [n_seqs]) with the guards behind them checked"""
    import torch

    n_seqs, n_q = len(b["offs"]) - 1, len(quantiles)
    end = len(b["counts"]) if n == 0 else first + n
    counts, valid = dev(b["counts"][first:end], torch.int32, shift), dev(b["valid"][first:end], torch.uint8, shift)
    offs = torch.from_numpy(b["offs"].view(np.int64)).cuda() if offsets == "given" else None
    out_q, out_m = guards(n_seqs * n_q), guards(n_seqs)
    torch.cuda.synchronize()  # the raw call runs on the context's stream: torch's fills are complete first
    batch.select_read_counts_raw(counts, valid, quantiles, out_q, out_m if n_kmers else None, first, n, offs)
    q, m = host(out_q), host(out_m)
    assert (q[n_seqs * n_q:] == QC.GUARD).all() and (m[n_seqs:] == QC.GUARD).all(), "written behind an output"
    if not n_kmers:
        assert (m == QC.GUARD).all()
    return q[:n_seqs * n_q].reshape(n_seqs, n_q), m[:n_seqs]


def same(b, got, want, tag):
    for what, g, w in (("quantiles", got[0], want[0]), ("n_kmers", got[1], want[1])):
        bad = np.nonzero((g != w).reshape(len(w), -1).any(axis=1))[0]
        assert len(bad) == 0, (tag, what, [(b["names"][i], g[i].tolist(), w[i].tolist()) for i in bad[:6]])


@pytest.mark.parametrize("qname", sorted(QC.QUANTILES))
def test_every_sequence_and_quantile(cases, qname):
    b, batch = cases
    q = QC.QUANTILES[qname]
    want = QC.expected(b["counts"], b["valid"], b["offs"], 0, len(b["counts"]), q)
    got = select(batch, b, 0, 0, q)
    same(b, got, want, qname)
    again = select(batch, b, 0, 0, q)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), "two runs give the same bits"
    without = select(batch, b, 0, 0, q, n_kmers=False)  # d_n_kmers = NULL
    assert np.array_equal(without[0], want[0])


def test_ranges_alignments_and_guards(cases):
    b, batch = cases
    q = QC.QUANTILES["ends"]
    n_bases = len(b["counts"])
    for name, first, n in QC.ranges(b):
        end = n_bases if n == 0 else first + n
        want = QC.expected(b["counts"], b["valid"], b["offs"], first, end, q)
        for shift in (0, 1, 2, 3):  # d_counts 0, 4, 8 and 12 bytes behind a 16-byte boundary, d_valid 0 .. 3 bytes
            same(b, select(batch, b, first, n, q, shift), want, (name, shift))
        if name == "no_whole_sequence":
            assert (want[0] == QC.GUARD).all() and (want[1] == QC.GUARD).all()


def synthetic_reads():
    """a few hundred 150-bp reads and a handful of 5 - 20 kbp reads drawn from one short genome (multiplicities above 1), some N"""
    rng = np.random.default_rng(77)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 30_000)
    lengths = [150] * 200 + [5_000, 150, 20_000, 7_777] + [150] * 100 + [12_345, 19_001, 150]
    pieces = []
    for length in lengths:
        s = int(rng.integers(0, len(genome) - length))
        pieces.append(genome[s:s + length].copy())
    seq = np.concatenate(pieces)
    seq[rng.integers(0, len(seq), 40)] = ord("N")
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    assert len(seq) < 1_000_000
    return seq, offs


def table_of(ctx, b, k, n):
    import torch

    from biolib_amd.scan import _flags

    vals = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    b.kmers128_raw(k, 0, _flags(True, False, True), 0, 0, vals, None, ok)
    keys = vals[ok == 1].contiguous()
    uniq, mult = ctx.sort_count128(keys, key_bits=2 * k)
    return ctx.count_table(uniq if k > 32 else uniq[:, 0].contiguous(), mult, key_bits=2 * k)


@pytest.mark.parametrize("k", (31, 51))
def test_end_to_end_against_kmer_counts_and_read_counts(ctx, k):
    import torch

    seq, offs = synthetic_reads()
    b = ctx.upload(seq, offs)
    t = table_of(ctx, b, k, len(seq))
    quantiles = QC.QUANTILES["ends"]
    counts, valid, r = b.kmer_counts(t, k, canonical=True, valid=True)
    want = QC.expected(host(counts), valid.cpu().numpy(), offs, 0, len(seq), quantiles)
    q, m, folded = b.read_quantiles(t, k, quantiles, canonical=True)
    assert np.array_equal(host(q), want[0]) and np.array_equal(host(m), want[1])
    assert folded == r, "one chunk: the scan's digest"
    assert want[0][:, 2].max() > 1, "the table holds multiplicities"
    # against bl_scan_read_counts
    rc = b.read_counts(t, k, canonical=True)[0].host()
    has = rc["n_kmers"] > 0
    assert has.sum() > 290 and np.array_equal(host(m), rc["n_kmers"])
    assert np.array_equal(host(q)[has, 0], rc["min_count"][has]) and np.array_equal(host(q)[has, 1], rc["max_count"][has])
    # chunking: several chunks, and chunks smaller than the longest read (which then gets one of its own)
    for chunk in (30_000, 1_000):
        q2, m2, folded2 = b.read_quantiles(t, k, quantiles, canonical=True, chunk_positions=chunk)
        assert torch.equal(q2, q) and torch.equal(m2, m) and folded2 == r, chunk
    assert len(b._sequence_chunks(offs, 30_000)) > 3 and max(e - s for s, e in b._sequence_chunks(offs, 1_000)) == 20_000
    med = b.read_medians(t, k, canonical=True)
    assert torch.equal(med, q[:, 2])
    # offsets= as a host array and as a device tensor
    q3 = b.read_quantiles(t, k, quantiles, canonical=True, offsets=offs, chunk_positions=50_000)[0]
    q4 = b.read_quantiles(t, k, quantiles, canonical=True, offsets=torch.from_numpy(offs.view(np.int64)).cuda(), chunk_positions=50_000)[0]
    assert torch.equal(q3, q) and torch.equal(q4, q)
    t.close()
    b.close()


def test_fixed_read_length_batch_without_offsets(ctx):
    k, read_len = 31, 150
    n = read_len * 700 + 77  # the last read is shorter
    b = ctx.synth(11, n, read_len)
    t = table_of(ctx, b, k, n)
    quantiles = QC.QUANTILES["inner"]
    counts, valid, r = b.kmer_counts(t, k, canonical=True, valid=True)
    offs = QC.fixed_offsets(n, read_len)
    want = QC.expected(host(counts), valid.cpu().numpy(), offs, 0, n, quantiles)
    for chunk in (None, 10 * read_len + 7):
        q, m, folded = b.read_quantiles(t, k, quantiles, canonical=True, chunk_positions=chunk)
        assert np.array_equal(host(q), want[0]) and np.array_equal(host(m), want[1]) and folded == r, chunk
    # the raw call, NULL offsets, a range that cuts a read at either end
    first, end = read_len * 3 + 5, read_len * 90 + 149
    cut = QC.expected(host(counts), valid.cpu().numpy(), offs, first, end, quantiles)
    got = select(b, dict(counts=host(counts), valid=valid.cpu().numpy(), offs=offs), first, end - first, quantiles, offsets=None)
    assert np.array_equal(got[0], cut[0]) and np.array_equal(got[1], cut[1])
    assert (got[1][:4] == QC.GUARD).all() and got[1][4] != QC.GUARD and got[1][89] != QC.GUARD and (got[1][90:] == QC.GUARD).all()
    t.close()
    b.close()


def test_single_sequence_batch_with_null_offsets(ctx):
    rng = np.random.default_rng(3)
    n = 2 * QC.CHUNK + 333
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    seq[1000:1010] = ord("N")
    b = ctx.upload(seq)
    assert b.n_seqs == 1
    t = table_of(ctx, b, 31, n)
    quantiles = QC.QUANTILES["ends"]
    counts, valid, r = b.kmer_counts(t, 31, valid=True)
    offs = np.array([0, n], np.uint64)
    want = QC.expected(host(counts), valid.cpu().numpy(), offs, 0, n, quantiles)
    q, m, folded = b.read_quantiles(t, 31, quantiles, chunk_positions=1000)  # one sequence, longer than the chunk
    assert np.array_equal(host(q), want[0]) and np.array_equal(host(m), want[1]) and folded == r
    arrays = dict(counts=host(counts), valid=valid.cpu().numpy(), offs=offs)
    for first, cnt in ((1, 0), (0, n - 1)):  # cut at either end: not touched
        got = select(b, arrays, first, cnt, quantiles, offsets=None)
        assert (got[0] == QC.GUARD).all() and (got[1] == QC.GUARD).all()
    t.close()
    b.close()


def test_refusals_and_empty_range(ctx, cases):
    import ctypes as C

    import torch

    import biolib_amd

    b, batch = cases
    n_seqs, n_bases = len(b["offs"]) - 1, len(b["counts"])
    counts, valid = dev(b["counts"], torch.int32), dev(b["valid"], torch.uint8)
    offs = torch.from_numpy(b["offs"].view(np.int64)).cuda()
    out_q, out_m = guards(n_seqs * 4), guards(n_seqs)
    lib, one = ctx._lib, ((1, 2),)
    torch.cuda.synchronize()

    def invalid(call):
        with pytest.raises(biolib_amd.BiolibError) as e:
            call()
        assert e.value.code == biolib_amd.capi.BL_ERR_INVALID, e.value
        assert len(str(e.value).split(":", 1)[1].strip()) > 0, "a message"
        return str(e.value)

    raw = batch.select_read_counts_raw
    invalid(lambda: raw(None, valid, one, out_q, out_m, 0, 0, offs))
    invalid(lambda: raw(counts, None, one, out_q, out_m, 0, 0, offs))
    invalid(lambda: raw(counts, valid, one, None, out_m, 0, 0, offs))
    assert "offsets" in invalid(lambda: raw(counts, valid, one, out_q, out_m, 0, 0, None))  # NULL offsets on a ragged batch
    assert "n_q" in invalid(lambda: raw(counts, valid, (), out_q, out_m, 0, 0, offs))
    assert "n_q" in invalid(lambda: raw(counts, valid, ((1, 2),) * 5, out_q, out_m, 0, 0, offs))
    assert "q_den" in invalid(lambda: raw(counts, valid, ((0, 0),), out_q, out_m, 0, 0, offs))
    assert "q_num" in invalid(lambda: raw(counts, valid, ((1, 2), (3, 2)), out_q, out_m, 0, 0, offs))
    invalid(lambda: raw(counts, valid, one, out_q, out_m, n_bases + 1, 0, offs))  # a range outside the batch
    # the C arguments the wrapper cannot leave out: ctx, batch, q_num, q_den
    num, den = (C.c_uint32 * 1)(1), (C.c_uint32 * 1)(2)
    args = [C.c_void_p(x.data_ptr()) for x in (counts, valid, offs)]
    outs = [C.c_void_p(x.data_ptr()) for x in (out_q, out_m)]
    for c_ctx, c_batch, c_num, c_den in ((None, batch._h, num, den), (ctx._h, None, num, den), (ctx._h, batch._h, None, den), (ctx._h, batch._h, num, None)):
        invalid(lambda: biolib_amd.capi.check(lib.bl_select_read_counts(c_ctx, c_batch, 0, 0, *args, c_num, c_den, 1, *outs)))
    other = biolib_amd.Context(0)
    assert "context" in invalid(lambda: biolib_amd.capi.check(lib.bl_select_read_counts(other._h, batch._h, 0, 0, *args, num, den, 1, *outs)))
    other.close()
    # an empty range succeeds and writes nothing; nor did any refused call
    raw(counts, valid, one, out_q, out_m, n_bases, 0, offs)
    raw(counts, valid, one, out_q, out_m, n_bases, 5, offs)
    assert (host(out_q) == QC.GUARD).all() and (host(out_m) == QC.GUARD).all()
    # a range of more than 2^31 positions (refused before anything is read); such a sequence cannot be chunked either
    big = ctx.synth(1, (1 << 31) + 5)
    assert big.n_seqs == 1
    assert "2^31" in invalid(lambda: big.select_read_counts_raw(counts, valid, one, out_q, out_m, 0, 0, None))
    assert (host(out_q) == QC.GUARD).all() and (host(out_m) == QC.GUARD).all()
    t = ctx.count_table(torch.tensor([1, 2], dtype=torch.int64, device="cuda"), None, key_bits=62)
    with pytest.raises(ValueError, match="2\\^31"):
        big.read_quantiles(t, 31)
    t.close()
    big.close()


# ---- past both grid caps (scale_cases.py): a wave's second sequence, a workgroup's second, third and fourth long sequence

@pytest.fixture(scope="module")
def tiled(ctx):
    """the model's batch laid end to end 140 times: 8,400 sequences (the wave kernel has 8,192 waves), 3,220 of them long (the workgroup
    kernel has 1,024 workgroups, which take the list in the order the wave kernel's atomic handed it out)"""
    import scale_cases as S

    qc = S.quantile_case()
    print(S.self_check_quantiles(qc))
    batch = ctx.upload(np.full(len(qc["counts"]), ord("A"), np.uint8), qc["offs"])
    assert batch.n_seqs == len(qc["offs"]) - 1
    yield qc, batch
    batch.close()


@pytest.mark.parametrize("qname", sorted(QC.QUANTILES))
def test_tiled_batch_past_both_grid_caps(tiled, qname):
    import scale_cases as S

    qc, batch = tiled
    q = QC.QUANTILES[qname]
    want = S.expected_quantiles(qc, 0, len(qc["counts"]), q)
    assert want[2].all()
    got = select(batch, qc, 0, 0, q)
    same(qc, got, want[:2], qname)
    again = select(batch, qc, 0, 0, q)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), "two runs give the same bits"


def test_tiled_batch_range_from_a_boundary_into_a_long_sequence(tiled):
    import scale_cases as S

    qc, batch = tiled
    q = QC.QUANTILES["ends"]
    first, n = S.cut_range(qc)
    want = S.expected_quantiles(qc, first, first + n, q)
    assert first > 0 and first in qc["offs"].tolist() and S.CAPS["WG_GRID_MAX"] < int(want[2].sum()) < len(want[2])
    got = select(batch, qc, first, n, q)
    same(qc, got, want[:2], "cut")
    again = select(batch, qc, first, n, q)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), "two runs give the same bits"


@pytest.mark.parametrize("kind", ("shuffled1", "shuffled2", "shuffled3", "alternating", "sawtooth"))
def test_wrong_offsets_on_the_device(cases, kind):
    """The contract fixes no set of visited sequences where the offsets are wrong, so the property is asserted: a row is all guard, or
    the model's answer for its raw span, which then lies inside the range; nothing else is written and no source array changes."""
    import torch

    import scale_cases as S

    b, batch = cases
    n = len(b["counts"])
    if kind.startswith("shuffled"):
        bad = QC.wrong_offsets(b["offs"], np.random.default_rng(int(kind[-1])))
    else:
        bad = S.alternating_offsets(b) if kind == "alternating" else S.sawtooth_offsets(b)
    q = QC.QUANTILES["ends"]
    n_seqs = len(bad) - 1
    counts, valid = dev(b["counts"], torch.int32), dev(b["valid"], torch.uint8)
    offs = torch.from_numpy(bad.view(np.int64)).cuda()
    out_q, out_m = guards(n_seqs * len(q)), guards(n_seqs)
    torch.cuda.synchronize()
    batch.select_read_counts_raw(counts, valid, q, out_q, out_m, 0, 0, offs)
    got_q, got_m = host(out_q), host(out_m)
    assert (got_q[n_seqs * len(q):] == QC.GUARD).all() and (got_m[n_seqs:] == QC.GUARD).all(), "written behind an output"
    written, long_written = S.check_rows_under_wrong_offsets(b, bad, 0, n, q, got_q[:n_seqs * len(q)].reshape(n_seqs, len(q)), got_m[:n_seqs])
    print(kind, dict(rows_written=written, long_rows_written=long_written, long_cap=S.long_cap(n, n_seqs)))
    assert long_written <= S.long_cap(n, n_seqs), "more long sequences answered than the list holds"
    assert np.array_equal(host(counts), b["counts"]) and np.array_equal(valid.cpu().numpy(), b["valid"]), "a source array changed"
    assert np.array_equal(offs.cpu().numpy().view(np.uint64), bad)
