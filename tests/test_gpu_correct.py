"""GPU tests of bl_scan_read_edits / bl_batch_apply_edits and their Python binding (Batch.read_edits_raw / read_edits / apply_edits /
correct_by_counts / edit_reads): every named case of the model (correct_cases.py: each index path was run under the sanitizers in
test_emu_correct.py) record for record, range seams, capacity, the kernels' launch limits, apply, refusals, and the chain end to end."""
import ctypes as C

import numpy as np
import pytest

import correct_cases as CC

pytestmark = pytest.mark.gpu
PAD = 8                      # guard records behind the edits
GUARD = -0x3A3A3A3A3A3A3A3B  # 0xC5C5...C5 as int64


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def upload(ctx, L):
    if L["read_len"]:
        return ctx.upload(L["bases"], read_len=L["read_len"])
    return ctx.upload(L["bases"], L["offs"]) if len(L["offs"]) > 2 else ctx.upload(L["bases"])


def table_on(ctx, table, k):
    import torch

    keys, counts = CC.table_arrays(table, k)
    return ctx.count_table(torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(counts.view(np.int32)).cuda(), key_bits=2 * k)


def scan(batch, table, k, canonical, min_count, min_support=1, first=0, n=0, capacity=None, need=None):
    """the C call with guarded edits -> (rc, EDIT array of the records stored, stats dict)"""
    import torch

    from biolib_amd import capi

    cap = capacity if capacity is not None else (need if need is not None else batch.n_bases // 2 + 1)
    edits = torch.full((cap + PAD, 2), GUARD, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # the raw call runs on the context's stream: torch's fill is complete first
    rc, stats = batch.read_edits_raw(table, k, 1 if canonical else 0, min_count, min_support, edits, cap, first, n)
    host = edits.cpu().numpy()
    stored = min(int(stats.n_edits), cap)
    assert (host[stored:] == GUARD).all(), "written at or beyond the capacity, or behind the last edit"
    assert rc == (capi.BL_ERR_CAPACITY if stats.n_edits > cap else capi.BL_OK)
    return rc, host[:stored].copy().view(CC.EDIT).reshape(-1), stats.as_dict()


def same_edits(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (tag, int(bad[0]), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("canonical", (False, True), ids=("forward", "canonical"))
@pytest.mark.parametrize("k", CC.KS)
def test_named_cases_in_three_layouts(ctx, k, canonical):
    c = CC.cases(k, canonical)
    table = table_on(ctx, c["table"], k)
    for kind in CC.LAYOUTS:
        L = CC.layout(c, kind)
        b = upload(ctx, L)
        for min_support in sorted({1, min(2, k), k}):
            want, stats, _ = CC.model(L["bases"], L["offs"], k, c["table"], c["min_count"], min_support, canonical)
            _, got, got_stats = scan(b, table, k, canonical, c["min_count"], min_support)
            assert got_stats == stats, (kind, min_support, got_stats, stats)
            same_edits(got, want, (kind, min_support))
        b.close()
    if k == 64:  # a run of 64 k-mers: 192 lookups of one wave
        assert want["support"].max() == 64 == CC.constants()["MAX_RUN"]
    table.close()


def short_batch(k, canonical, limit=620):
    c = CC.cases(k, canonical)
    reads, total = [], 0
    for name, r in zip(c["names"], c["reads"]):
        if k >= 10 and name.startswith("every_base") and int(name.rsplit("_p", 1)[1]) % 4:
            continue
        if total + len(r) <= limit:
            reads.append(r)
            total += len(r)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return c, CC.as_bytes("".join(reads)), offs


@pytest.mark.parametrize("k,canonical", ((5, False), (15, True)))
def test_every_cut_into_two_ranges_and_ranges_of_one_position(ctx, k, canonical):
    c, bases, offs = short_batch(k, canonical)
    n = len(bases)
    assert 500 <= n <= 620
    table = table_on(ctx, c["table"], k)
    b = ctx.upload(bases, offs)
    want, stats, _ = CC.model(bases, offs, k, c["table"], c["min_count"], 1, canonical)
    assert len(want) >= 5 and stats["n_misfit"] > 0
    _, whole, whole_stats = scan(b, table, k, canonical, c["min_count"], need=len(want))
    same_edits(whole, want, "whole")
    assert whole_stats == stats
    for cut in range(1, n):
        _, e1, s1 = scan(b, table, k, canonical, c["min_count"], first=0, n=cut, need=len(want))
        _, e2, s2 = scan(b, table, k, canonical, c["min_count"], first=cut, n=0, need=len(want))
        same_edits(np.concatenate([e1, e2]), want, cut)
        assert {name: s1[name] + s2[name] for name in stats} == stats, cut
    parts, total = [], dict.fromkeys(stats, 0)
    for first in range(n):
        _, e, s = scan(b, table, k, canonical, c["min_count"], first=first, n=1, need=len(want))
        parts.append(e)
        total = {name: total[name] + s[name] for name in stats}
    same_edits(np.concatenate(parts), want, "ranges of one position")
    assert total == stats
    b.close()
    table.close()


def one_error_reads(k, m, canonical, seed=5):
    """m reads of 2k + 5 bases, each with exactly one repairable error: -> (bases, offs, table dict, pos and true byte of every error)"""
    rng = np.random.default_rng(seed)
    R = 2 * k + 5
    codes = rng.integers(0, 4, (m, R)).astype(np.uint8)
    letters = np.frombuffer(b"ACGT", np.uint8)
    truth = letters[codes].reshape(-1)
    offs = np.arange(0, (m + 1) * R, R, dtype=np.uint64)
    table = {key: 3 for key in set(t[2] for q in range(m) for t in CC.read_kmers(codes[q], k, canonical))}
    at = rng.integers(0, R, m)
    wrong = codes.copy()
    wrong[np.arange(m), at] = (wrong[np.arange(m), at] + rng.integers(1, 4, m)) % 4
    return letters[wrong].reshape(-1), offs, table, np.arange(m) * R + at, truth


def test_every_read_with_one_repairable_error_and_the_launch_limits(ctx):
    """candidate counts one below, at and one above a workgroup of the test pass (one candidate per wave: TEST_WAVES) and of the
    compaction (CTPB), and ranges of CTPB - 1, CTPB and CTPB + 1 positions for the run pass, which takes one position per thread"""
    k = 21
    K = CC.constants()
    m = 2 * K["CTPB"] + 1
    bases, offs, table, at, truth = one_error_reads(k, m, True)
    R = int(offs[1])
    want, stats, _ = CC.model(bases, offs, k, table, 3, 1, True)
    assert stats["n_edits"] == stats["n_runs"] == m and np.array_equal(want["pos"], at.astype(np.uint64)) and np.array_equal(want["to"], truth[at])
    t = table_on(ctx, table, k)
    b = ctx.upload(bases, read_len=R)
    _, got, got_stats = scan(b, t, k, True, 3)
    same_edits(got, want, "all reads")
    assert got_stats == stats
    for n_cand in sorted({K["TEST_WAVES"] - 1, K["TEST_WAVES"], K["TEST_WAVES"] + 1, 63, 64, 65, K["CTPB"] - 1, K["CTPB"], K["CTPB"] + 1, 2 * K["CTPB"]}):
        _, got, s = scan(b, t, k, True, 3, first=0, n=n_cand * R)  # the runs of the first n_cand reads: a run never begins in a read's last k - 1 positions
        same_edits(got, want[:n_cand], n_cand)
        assert s["n_edits"] == s["n_runs"] == n_cand
    for first in (0, 7, R + 3):
        for n in (K["CTPB"] - 1, K["CTPB"], K["CTPB"] + 1, 2 * K["CTPB"], 2 * K["CTPB"] + 1):
            w, ws, _ = CC.model(bases, offs, k, table, 3, 1, True, first, n)
            _, got, s = scan(b, t, k, True, 3, first=first, n=n)
            same_edits(got, w, (first, n))
            assert s == ws
    # the chain: every error repaired, the truth restored
    fixed, edits, all_stats = b.correct_by_counts(t, k, 3, canonical=True, passes=3)
    assert len(all_stats) == 2 and all_stats[0]["n_edits"] == m and all_stats[1]["n_runs"] == 0
    assert np.array_equal(fixed.download(), truth) and fixed.n_seqs == m and fixed.read_len == R
    read, rel = b.edit_reads(edits[0])
    assert np.array_equal(read.cpu().numpy(), np.arange(m)) and np.array_equal(rel.cpu().numpy(), at % R)
    fixed.close()
    b.close()
    t.close()


def test_capacity(ctx):
    from biolib_amd import capi

    k = 31
    c = CC.cases(k, False)
    L = CC.layout(c, "offsets")
    table = table_on(ctx, c["table"], k)
    b = upload(ctx, L)
    want, stats, _ = CC.model(L["bases"], L["offs"], k, c["table"], c["min_count"])
    need = len(want)
    for cap in (need, need - 1, 1, 0):
        rc, got, s = scan(b, table, k, False, c["min_count"], capacity=cap)
        assert rc == (capi.BL_OK if cap >= need else capi.BL_ERR_CAPACITY) and s == stats
        same_edits(got, want[:cap], cap)
    rc, s = b.read_edits_raw(table, k, 0, c["min_count"], 1, None, 0)  # the counting call
    assert rc == capi.BL_ERR_CAPACITY and s.as_dict() == stats
    edits, s = b.read_edits(table, k, c["min_count"], capacity=3)  # the binding runs once more with the reported count
    assert s == stats
    same_edits(b.edits_host(edits), want, "read_edits")
    read, rel = b.edit_reads(edits)
    assert np.array_equal(L["offs"][read.cpu().numpy()].astype(np.int64) + rel.cpu().numpy(), want["pos"].astype(np.int64))
    assert all(0 <= r < len(c["reads"][q]) for q, r in zip(read.tolist(), rel.tolist()))
    b.close()
    table.close()


def test_empty_range_batch_and_table(ctx):
    import torch

    c = CC.cases(5, False)
    L = CC.layout(c, "offsets")
    table = table_on(ctx, c["table"], 5)
    b = upload(ctx, L)
    zero = dict.fromkeys(CC.STAT_NAMES, 0)
    assert scan(b, table, 5, False, 3, first=len(L["bases"]), n=0)[2] == zero
    empty = ctx.upload(b"")
    assert scan(empty, table, 5, False, 3, capacity=1)[2] == zero
    copy = empty.apply_edits(torch.zeros((0, 2), dtype=torch.int64, device="cuda"))
    assert copy.n_bases == 0
    none = ctx.count_table(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), key_bits=10)
    _, got, s = scan(b, none, 5, False, 1)
    assert len(got) == 0 and s["n_runs"] == s["n_misfit"] > 0 and s == CC.model(L["bases"], L["offs"], 5, {}, 1)[1]
    for x in (copy, empty, b, none, table):
        x.close()


@pytest.mark.parametrize("kind", CC.LAYOUTS)
def test_apply_edits(ctx, kind):
    import torch

    k = 15
    c = CC.cases(k, True)
    L = CC.layout(c, kind)
    n = len(L["bases"])
    table = table_on(ctx, c["table"], k)
    b = upload(ctx, L).set_origin(1000)
    want, _, _ = CC.model(L["bases"], L["offs"], k, c["table"], c["min_count"], 1, True)
    edits, _ = b.read_edits(table, k, c["min_count"], canonical=True)
    fixed = b.apply_edits(edits)
    assert np.array_equal(fixed.download(), CC.apply_model(L["bases"], want))
    assert (fixed.n_bases, fixed.n_seqs, fixed.read_len) == (b.n_bases, b.n_seqs, b.read_len) and fixed._lib.bl_batch_origin(fixed._h) == 1000
    assert np.array_equal(b.download(), L["bases"]), "the source batch is unchanged"
    # the geometry: the corrected batch's k-mers are valid where the model says, read by read
    counts, valid, _ = fixed.kmer_counts(table, k, canonical=True, valid=True)
    st, cnt = CC.position_states(CC.apply_model(L["bases"], want), L["offs"], k, c["table"], c["min_count"], True)
    assert np.array_equal(valid.cpu().numpy() != 0, st != CC.INVALID) and np.array_equal(counts.cpu().numpy(), cnt)
    # pos >= n_bases is ignored, among equal neighbours the first wins, from is not checked
    odd = np.zeros(6, CC.EDIT)
    odd["pos"] = (3, 3, 3, n, 2**63, n - 1)
    odd["to"] = (ord("x"), ord("y"), ord("z"), ord("!"), ord("!"), ord("q"))
    odd["from"] = 7
    d_odd = torch.from_numpy(odd.view(np.int64).reshape(-1, 2)).cuda()
    out = b.apply_edits(d_odd)
    expect = L["bases"].copy()
    expect[3], expect[n - 1] = ord("x"), ord("q")
    assert np.array_equal(out.download(), expect) and np.array_equal(expect, CC.apply_model(L["bases"], odd))
    plain = b.apply_edits(d_odd[:0])
    assert np.array_equal(plain.download(), L["bases"]) and plain.n_seqs == b.n_seqs
    for x in (plain, out, fixed, b, table):
        x.close()


def test_end_to_end_on_simulated_reads(ctx):
    """0.2 Mbp of simulated reads: read_counts of the corrected batch gives, per read, the old n_kmers and n_solid increased by exactly
    the summed support of that read's edits; a second pass makes edits only where the model says so"""
    import torch

    k = 21
    bases, truth, offs, planted = CC.simulate(seed=1, genome_len=20000, read_len=100, coverage=10, rate=0.01)
    assert len(bases) == 200000
    table_py = CC.counted_table(bases, offs, k, True)
    table = table_on(ctx, table_py, k)
    b = ctx.upload(bases, read_len=100)
    before, _ = b.read_counts(table, k, 2, canonical=True)
    fixed, edits, stats = b.correct_by_counts(table, k, 2, canonical=True, passes=2)
    first = b.edits_host(edits[0])
    want, want_stats, _ = CC.model(bases, offs, k, table_py, 2, 1, True)
    same_edits(first, want, "first pass")
    assert stats[0] == want_stats and 2 * len(first) >= len(planted)
    once = b.apply_edits(edits[0])
    after, _ = once.read_counts(table, k, 2, canonical=True)
    r0, r1 = before.host(), after.host()
    gain = np.zeros(len(offs) - 1, np.int64)
    np.add.at(gain, (first["pos"] // 100).astype(np.int64), first["support"].astype(np.int64))
    assert np.array_equal(r1["n_kmers"], r0["n_kmers"]) and np.array_equal(r1["n_solid"].astype(np.int64), r0["n_solid"].astype(np.int64) + gain)
    second_want, second_stats, _ = CC.model(CC.apply_model(bases, want), offs, k, table_py, 2, 1, True)
    assert stats[1] == second_stats
    if len(edits) > 1:
        same_edits(b.edits_host(edits[1]), second_want, "second pass")
    assert np.array_equal(fixed.download(), CC.apply_model(CC.apply_model(bases, want), second_want))
    for x in (once, fixed, b, table):
        x.close()


def test_refusals_write_nothing(ctx):
    import biolib_amd
    import torch

    from biolib_amd import capi

    k = 15
    c = CC.cases(k, False)
    L = CC.layout(c, "offsets")
    table = table_on(ctx, c["table"], k)
    narrow = table_on(ctx, CC.cases(5, False)["table"], 5)  # key_bits = 10
    b = upload(ctx, L)
    other = biolib_amd.Context(0)
    foreign_batch = other.upload(L["bases"], L["offs"])
    foreign_table = table_on(other, c["table"], k)
    lib = b._lib
    edits = torch.full((64 + PAD, 2), GUARD, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vp = C.c_void_p

    def call(c_ctx=ctx._h, c_batch=b._h, first=0, n=0, kk=k, flags=0, c_table=table._h, min_count=3, min_support=1, ptr=edits.data_ptr(), cap=64):
        stats = capi.EditStats()
        stats.n_runs = 77
        rc = lib.bl_scan_read_edits(c_ctx, c_batch, first, n, kk, flags, c_table, min_count, min_support, vp(ptr), cap, C.byref(stats))
        assert rc == capi.BL_ERR_INVALID and lib.bl_last_error(), "refused with a message"
        assert stats.n_runs == 77, "nothing written"

    call(c_ctx=None)
    call(c_batch=None)
    call(c_table=None)
    call(c_batch=foreign_batch._h)
    call(c_table=foreign_table._h)
    call(ptr=edits.data_ptr() + 8)
    call(ptr=None)  # NULL with a capacity
    call(kk=0)
    call(kk=65)
    call(c_table=narrow._h)  # 2k > key_bits
    call(kk=33, c_table=table._h)  # a one-word table takes k <= 32
    call(min_count=0)
    call(min_support=0)
    call(min_support=k + 1)
    call(flags=capi.FLAG_DROP_LAST)
    call(flags=1 << 7)
    call(first=len(L["bases"]) + 1)
    torch.cuda.synchronize()
    assert (edits.cpu().numpy() == GUARD).all()
    rc, _ = b.read_edits_raw(table, k, capi.FLAG_SYNC, 3, 1, edits, 64)  # BL_FLAG_SYNC is accepted
    assert rc in (capi.BL_OK, capi.BL_ERR_CAPACITY)

    h = vp(5)
    for args in ((None, b._h, vp(edits.data_ptr()), 1, C.byref(h)), (ctx._h, None, vp(edits.data_ptr()), 1, C.byref(h)), (ctx._h, b._h, vp(edits.data_ptr()), 1, None),
                 (ctx._h, foreign_batch._h, vp(edits.data_ptr()), 1, C.byref(h)), (ctx._h, b._h, None, 1, C.byref(h)), (ctx._h, b._h, vp(edits.data_ptr() + 8), 1, C.byref(h))):
        assert lib.bl_batch_apply_edits(*args) == capi.BL_ERR_INVALID and lib.bl_last_error()
    for x in (foreign_batch, foreign_table):
        x.close()
    other.close()
    for x in (b, narrow, table):
        x.close()
