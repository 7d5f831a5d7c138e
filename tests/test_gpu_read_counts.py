"""GPU tests of bl_scan_read_counts and its Python binding (Batch.read_counts / read_counts_raw / ReadCounts): against the Python model
with the batches of the host emulation (read_counts_cases.py: every index path was run under the sanitizers there), against
bl_scan_kmer_counts on the same arguments — whose result the call must return word for word — and against a torch segment reduction
of that scan's per-position output."""
import numpy as np
import pytest

import kmers128_model as M
import lookup_cases as LC
import read_counts_cases as RC

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
U32 = (1 << 32) - 1
DIGEST = ("count", "xor_value", "aux", "xor_hash", "xor_pos")


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def build(ctx, table, key_words, key_bits):
    import torch

    keys = list(table)
    return ctx.count_table(torch.from_numpy(LC.words(keys, key_words).view(np.int64)).cuda(),
                           torch.from_numpy(np.array([table[k] for k in keys], np.uint32).view(np.int32)).cuda(), key_bits=key_bits)


def invalid(call):
    import biolib_amd

    with pytest.raises(biolib_amd.BiolibError) as e:
        call()
    assert e.value.code == biolib_amd.capi.BL_ERR_INVALID, e.value
    return str(e.value)


def canaries(n_seqs):
    import torch

    return torch.full((n_seqs, 48), RC.CANARY_BYTE, dtype=torch.uint8, device="cuda")


def host_records(buf):
    return buf.cpu().numpy().view(RC.RECORD).reshape(-1)


def dev_offsets(offs):
    import torch

    return torch.from_numpy(offs.view(np.int64)).cuda()


def upload(ctx, c):
    if c["name"] == "ragged":
        return ctx.upload(c["seq"], c["offs"])
    return ctx.upload(c["seq"], read_len=c["read_len"]) if c["read_len"] else ctx.upload(c["seq"])


def check_against_model(ctx, c, key_words, min_count, with_offsets):
    """both ranges of lookup_cases.RANGES under INIT into buffers of canaries: the touched records are the model's, byte for byte, every
    other record is untouched; the result is bl_scan_kmer_counts's and the model's"""
    from biolib_amd.scan import _flags

    b = upload(ctx, c)
    t = build(ctx, c["table"], key_words, 2 * c["k"])
    n_seqs = len(c["offs"]) - 1
    assert b.n_seqs == n_seqs
    offs = dev_offsets(c["offs"]) if with_offsets else None
    flags = _flags(c["canonical"], c["drop_last"], True)
    for first, n in LC.RANGES:
        end = len(c["seq"]) if n == 0 else first + n
        buf = canaries(n_seqs)
        r = b.read_counts_raw(t, c["k"], flags, min_count, buf, first, n, offs).as_dict()
        d = LC.expected_scan(c["m"], c["table"], first, end)[2]
        assert {x: r[x] for x in d} == d and r["status"] == 0
        r2 = b.kmer_counts_raw(t, c["k"], flags, first, n).as_dict()
        assert r == r2
        want = RC.expected_records(c["m"], c["table"], c["offs"], first, end, min_count)
        got = host_records(buf)
        assert RC.same(got, want), (c["name"], c["k"], c["canonical"], c["drop_last"], key_words, min_count, first, np.nonzero(got != want)[0][:8])
        lo, hi = RC.touched(c["offs"], first, end)
        if c["name"] == "ragged":  # a canary record in front of and behind the touched span
            assert lo >= 1 and hi <= n_seqs - 2 and (got[[lo - 1, hi + 1]].view(np.uint8) == RC.CANARY_BYTE).all()
    t.close()
    b.close()


@pytest.mark.parametrize("k", (1, 31, 32, 33, 64))
def test_records_vs_model(ctx, k):
    for i, (canonical, drop_last) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        c = RC.case("ragged", k, canonical, drop_last)
        for kw in ((1, 2) if k <= 32 else (2,)):
            check_against_model(ctx, c, kw, RC.MIN_COUNTS[(i + kw) % 3], True)


@pytest.mark.parametrize("name", ("single",) + tuple(f"fixed{length}" for length in RC.FIXED))
def test_single_sequence_and_fixed_length_batches(ctx, name):
    c = RC.case(name, 31, True, False)
    check_against_model(ctx, c, 2, 2, with_offsets=False)  # sequence = position / read_len, or 0
    check_against_model(ctx, c, 1, 1, with_offsets=True)   # the same batch with its offsets: bisection


def torch_records(counts, valid, seq_ids, bases, n_seqs, min_count):
    """the segment reduction of bl_scan_kmer_counts's output a caller writes in torch; seq_ids / bases: sequence and sequence start of every
    position.  A stored count is at least 1 in the tables used with it, so found = count > 0."""
    import torch

    v = valid == 1
    c = (counts.to(torch.int64) & U32)[v]
    ids = seq_ids[v]
    rel = (torch.arange(len(valid), device=valid.device) - bases)[v]
    out = np.zeros(n_seqs, RC.RECORD)
    zeros = lambda: torch.zeros(n_seqs, dtype=torch.int64, device=valid.device)
    big = 1 << 62
    out["n_kmers"] = zeros().index_add_(0, ids, torch.ones_like(c)).cpu().numpy()
    out["n_found"] = zeros().index_add_(0, ids, (c > 0).to(torch.int64)).cpu().numpy()
    out["n_solid"] = zeros().index_add_(0, ids, (c >= min_count).to(torch.int64)).cpu().numpy()
    out["sum_counts"] = zeros().index_add_(0, ids, c).cpu().numpy()
    mn = torch.full((n_seqs,), big, dtype=torch.int64, device=valid.device).scatter_reduce_(0, ids, c, "amin").cpu().numpy()
    out["min_count"] = np.where(mn == big, U32, mn)
    out["max_count"] = zeros().scatter_reduce_(0, ids, c, "amax").cpu().numpy()
    weak = c < min_count
    wb = torch.full((n_seqs,), big, dtype=torch.int64, device=valid.device).scatter_reduce_(0, ids[weak], rel[weak], "amin").cpu().numpy()
    out["weak_begin"] = np.where(wb == big, np.uint64(M64), wb.astype(np.uint64))
    out["weak_end"] = zeros().scatter_reduce_(0, ids[weak], rel[weak] + 1, "amax").cpu().numpy()
    return out


@pytest.mark.parametrize("k,read_len,min_count", [(31, 150, 2), (51, 10_000, 1)])
def test_equals_kmer_counts_then_torch_reduction(ctx, k, read_len, min_count):
    import torch

    from biolib_amd.scan import _flags

    n = 150 * 7000 + 77  # about 1 Mbp; the last read is shorter
    b, ref = ctx.synth(11, n, read_len), ctx.synth(12, n, read_len)
    n_seqs = b.n_seqs
    assert n_seqs == -(-n // read_len)
    # the table: this batch's canonical k-mers of the first half and another batch's, counted by the library itself
    vals = torch.empty((2 * n, 2), dtype=torch.int64, device="cuda")
    ok = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    b.kmers128_raw(k, 0, _flags(True, False, True), 0, n // 2, vals, None, ok)
    ref.kmers128_raw(k, 0, _flags(True, False, True), 0, 0, vals[n // 2:], None, ok[n // 2:])
    keys = vals[: n // 2 + n][ok[: n // 2 + n] == 1].contiguous()
    uniq, mult = ctx.sort_count128(keys, key_bits=2 * k)
    t = ctx.count_table(uniq if k > 32 else uniq[:, 0].contiguous(), mult, key_bits=2 * k)
    pos = torch.arange(n, device="cuda")
    seq_ids = pos // read_len
    for canonical in (True, False):
        counts, valid, r = b.kmer_counts(t, k, canonical=canonical, valid=True)
        rc, r2 = b.read_counts(t, k, min_count=min_count, canonical=canonical)
        assert r2 == r and r["count"] > n // 2
        want = torch_records(counts, valid, seq_ids, seq_ids * read_len, n_seqs, min_count)
        got = rc.host()
        assert RC.same(got, want), np.nonzero(got != want)[0][:8]
        assert int(rc.n_found.sum()) == r["found"] and int(rc.sum_counts.sum()) == r["sum_counts"] and int(rc.n_kmers.sum()) == r["count"]
        if canonical:
            assert r["found"] > n // 3
        # with the offsets (bisection over n_seqs sequences) the records are the same
        rc_off, r3 = b.read_counts(t, k, min_count=min_count, canonical=canonical, offsets=RC.fixed_offsets(n, read_len))
        assert r3 == r and torch.equal(rc_off.records, rc.records)
    t.close()
    b.close()
    ref.close()


def test_accumulate_init_and_reproducibility(ctx):
    import torch

    k = 33
    c = RC.case("ragged", k, True, False)
    b = upload(ctx, c)
    t = build(ctx, c["table"], 2, 2 * k)
    n_bases, offs = len(c["seq"]), c["offs"]
    whole, r = b.read_counts(t, k, min_count=2, canonical=True)
    want = RC.expected_records(c["m"], c["table"], offs, 0, n_bases, 2)
    filled = want.copy()
    filled[[0, -1]] = RC.IDENTITY  # the empty first and last sequence are outside the touched span: ReadCounts starts as identities
    assert RC.same(whole.host(), filled)
    again, r_again = b.read_counts(t, k, min_count=2, canonical=True)
    assert torch.equal(again.records, whole.records) and r_again == r, "two runs give the same bits"
    # ranges cut inside the read over three tiles, at a read's first base (4000, 8300) and inside a short read add up
    cuts = [0, 1500, 4000, 5234, 8300, 8303, n_bases]
    acc = None
    total = dict.fromkeys(("count", "found", "sum_counts"), 0)
    for first, end in reversed(list(zip(cuts[:-1], cuts[1:]))):
        acc, part = b.read_counts(t, k, min_count=2, canonical=True, first=first, n=end - first, into=acc)
        for word in total:
            total[word] += part[word]
    assert torch.equal(acc.records, whole.records), np.nonzero(acc.host() != whole.host())[0][:8]
    assert total == {word: r[word] for word in total}
    # INIT after ACCUMULATE resets: the touched records are this range's alone, the others keep what they had
    first, n = 37, 8200
    from biolib_amd.scan import _flags

    b.read_counts_raw(t, k, _flags(True, False, True), 2, acc.records, first, n, dev_offsets(offs))
    lo, hi = RC.touched(offs, first, first + n)
    want = RC.expected_records(c["m"], c["table"], offs, first, first + n, 2)
    got, before = acc.host(), whole.host()
    assert RC.same(got[lo:hi + 1], want[lo:hi + 1]) and RC.same(got[:lo], before[:lo]) and RC.same(got[hi + 1:], before[hi + 1:])
    assert not RC.same(got[lo:hi + 1], before[lo:hi + 1])
    t.close()
    b.close()


def test_refusals_and_empty_range(ctx):
    import torch

    import biolib_amd
    from biolib_amd.scan import _flags

    c = RC.case("ragged", 31, False, False)
    b = upload(ctx, c)
    n_seqs = b.n_seqs
    offs = dev_offsets(c["offs"])
    flags = _flags(False, False, True)
    t1 = ctx.count_table(torch.tensor([1, 2], dtype=torch.int64, device="cuda"), None, key_bits=62)
    t2 = ctx.count_table(torch.tensor([[1, 0], [2, 0]], dtype=torch.int64, device="cuda"), None, key_bits=102)
    buf = canaries(n_seqs)
    assert "min_count" in invalid(lambda: b.read_counts_raw(t2, 31, flags, 0, buf, 0, 0, offs))
    assert "offsets" in invalid(lambda: b.read_counts_raw(t2, 31, flags, 1, buf, 0, 0, None))        # NULL offsets on a ragged batch
    parsed = ctx.from_text(b">a\nACGTACGTACGTACGT\n>b\nACGTACG\n>c\nAC\n")                            # no offsets on record: offsets= is required
    assert parsed.n_seqs == 3 and "offsets" in invalid(lambda: parsed.read_counts(t2, 3))
    rc, r = parsed.read_counts(t2, 3, offsets=np.array([0, 16, 23, 25], np.uint64))
    assert [int(x) for x in rc.n_kmers.cpu()] == [14, 5, 0] and r["count"] == 19
    parsed.close()
    assert "key_bits" in invalid(lambda: b.read_counts_raw(t1, 32, flags, 1, buf, 0, 0, offs))      # 2k = 64 > 62
    assert "key_bits" in invalid(lambda: b.read_counts_raw(t2, 52, flags, 1, buf, 0, 0, offs))      # 2k = 104 > 102
    t64 = ctx.count_table(torch.tensor([1, 2], dtype=torch.int64, device="cuda"), None, key_bits=64)
    invalid(lambda: b.read_counts_raw(t64, 33, flags, 1, buf, 0, 0, offs))                          # a one-word table takes k <= 32
    invalid(lambda: b.read_counts_raw(t2, 0, flags, 1, buf, 0, 0, offs))
    invalid(lambda: b.read_counts_raw(t2, 65, flags, 1, buf, 0, 0, offs))
    invalid(lambda: b.read_counts_raw(t2, 31, flags, 1, buf, 0, 0, offs, mode=2))
    invalid(lambda: b.read_counts_raw(t2, 31, flags, 1, None, 0, 0, offs))                           # d_records NULL
    odd = canaries(n_seqs + 1).view(-1)[8:8 + 48 * n_seqs]
    assert odd.data_ptr() % 16 == 8
    assert "aligned" in invalid(lambda: b.read_counts_raw(t2, 31, flags, 1, odd, 0, 0, offs))
    other = biolib_amd.Context(0)
    foreign = other.count_table(torch.tensor([[1, 0], [2, 0]], dtype=torch.int64, device="cuda"), None, key_bits=102)
    assert "context" in invalid(lambda: b.read_counts_raw(foreign, 31, flags, 1, buf, 0, 0, offs))
    foreign.close()
    other.close()
    invalid(lambda: b.read_counts_raw(t2, 31, flags, 1, buf, len(c["seq"]) + 1, 0, offs))
    # an empty range succeeds and writes nothing; nor did any refused call
    for mode in (0, 1):
        r = b.read_counts_raw(t2, 31, flags, 1, buf, len(c["seq"]), 0, offs, mode=mode)
        assert r.count == 0 and r.xor_hash == 0 and r.xor_pos == 0
    assert (buf == RC.CANARY_BYTE).all()
    for t in (t1, t2, t64):
        t.close()
    b.close()


@pytest.mark.parametrize("k,m", [(31, 15), (51, 21)])
def test_count_then_table_then_read_counts(ctx, k, m):
    from biolib_amd import shard

    rng = np.random.default_rng(k)
    n_reads, L = 60, 150
    base = rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000)
    starts = rng.integers(0, len(base) - L, n_reads)
    seq = np.concatenate([base[s:s + L] for s in starts])  # overlapping reads of one short genome: multiplicities above 1
    seq[[100, 4000]] = ord("N")
    offs = np.arange(0, len(seq) + 1, L, dtype=np.uint64)
    b = ctx.upload(seq, offs)
    keys, mult = shard.count_kmers_via_super_kmers(ctx, b, k, m, canonical=True)
    t = ctx.count_table(keys, mult, key_bits=2 * k)
    model = M.scan(seq.tobytes(), offs, k, 0, True, False)
    valid = model["valid"] == 1
    pairs = np.stack([model["lo"][valid], model["hi"][valid]], axis=1)
    uniq, inverse, cnt = np.unique(pairs, axis=0, return_inverse=True, return_counts=True)
    counts = np.zeros(len(seq), np.uint64)
    counts[valid] = cnt[inverse.reshape(-1)]
    rc, r = b.read_counts(t, k, min_count=2, canonical=True)
    got = rc.host()
    per_read = valid.reshape(n_reads, L)
    assert np.array_equal(got["n_kmers"], per_read.sum(axis=1)) and (got["n_kmers"] < L - k + 1).sum() == 2, "two reads hold an N"
    assert np.array_equal(got["n_found"], got["n_kmers"]), "every k-mer of the batch is in the table made from it"
    assert np.array_equal(got["sum_counts"], counts.reshape(n_reads, L).sum(axis=1)) and cnt.max() > 1
    assert np.array_equal(got["max_count"], counts.reshape(n_reads, L).max(axis=1))
    assert np.array_equal(got["n_solid"], ((counts >= 2) & valid).reshape(n_reads, L).sum(axis=1))
    assert r["found"] == r["count"] == int(valid.sum()) and r["sum_counts"] == int(counts.sum())
    t.close()
    b.close()
