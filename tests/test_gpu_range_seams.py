"""The range sweep of tests/range_cases.py on the device: every scan entry point as consecutive ranges cut at every kind of place (every residue
of `first` mod 16, around tile and wave borders, sequence starts, N's, the repeat island, planted tie windows, the batch's end; two- and
three-way).  Per range: the count, every array element for element and every digest word against the rule of range_cases.py, with the
arrays given EXACTLY the expected count as capacity; per cut set: the concatenation against the whole scan.  The same sweep through the CPU
emulation is test_range_seams.py; what only this module meets: bl_capi.hip's planning of a range (scan_windows, prepare_kmers128,
scan_two_pass128), the tile prefix scan, the capacity path of end_scan, start bits built by the first unaligned range of a batch of reads,
two halves of one scan in different layouts, asynchronous ranges on two lanes, a batch origin, and the device build of the phases.

One item is one (shape, input): a few hundred scans of at most four tiles."""
import ctypes as C

import numpy as np
import pytest

import kernel_cases as K
import oracle_lib as O
import range_cases as RC

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A5A5A5A5A
MIXED_NAMES = {}


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def upload(ctx, inp):
    return ctx.upload(inp.seq, read_len=inp.read_len) if inp.read_len else ctx.upload(inp.seq, offsets=inp.offs)


class Out:
    """output arrays of one input, reused over its ranges: a sentinel behind what a call may write"""

    def __init__(self, n):
        import torch

        self.cap = n + 1 + RC.GUARD
        self.w = torch.full((4 * self.cap,), SENT, dtype=torch.int64, device="cuda")  # values / records: up to four words per record
        self.p = torch.full((self.cap,), SENT, dtype=torch.int64, device="cuda")
        self.h = torch.full((self.cap,), SENT, dtype=torch.int64, device="cuda")
        self.mp = torch.zeros(self.cap, dtype=torch.uint8, device="cuda")
        self.sz = torch.zeros(self.cap, dtype=torch.uint8, device="cuda")


def _u64(t, n, words=1):
    a = t[:n * words].cpu().numpy().view(np.uint64).copy()
    return a.reshape(-1, words) if words > 1 else a


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def scan64(ctx, batch, r, out, first, n, capacity, seed, sync=True, result=None):
    """one call of the row's entry point through the C ABI with `capacity` slots: (rc, Result)"""
    import biolib_amd as B
    from biolib_amd import capi

    L = capi.lib()
    flags = (B.FLAG_CANONICAL if r.canonical else 0) | (B.FLAG_SYNC if sync else 0)
    res = result if result is not None else capi.Result()
    k = r.unit + r.w - 1
    if r.entry == "minimizers":
        rc = L.bl_scan_minimizers(ctx._h, batch._h, first, n, r.unit, r.w, seed, flags, _ptr(out.w), _ptr(out.p), _ptr(out.h), capacity, C.byref(res))
    elif r.entry == "hash_sample":
        rc = L.bl_scan_hash_sample(ctx._h, batch._h, first, n, r.unit, seed, K.THRESHOLD, flags, _ptr(out.w), _ptr(out.p), _ptr(out.h), capacity, C.byref(res))
    elif r.entry == "super_kmers":
        rc = L.bl_scan_super_kmers(ctx._h, batch._h, first, n, k, r.unit, seed, flags, _ptr(out.w), _ptr(out.p), _ptr(out.mp), _ptr(out.sz), _ptr(out.h), capacity, C.byref(res))
    else:
        rc = L.bl_scan_syncmers(ctx._h, batch._h, first, n, k, r.unit, r.offsets[0], r.offsets[1], seed, flags, _ptr(out.p), capacity, C.byref(res))
    return rc, res


def got64(r, out, res):
    c = int(res.count)
    got = res.as_dict()
    if r.entry in ("minimizers", "hash_sample"):
        got.update(values=_u64(out.w, c), positions=_u64(out.p, c), hashes=_u64(out.h, c))
    elif r.entry == "super_kmers":
        got.update(minimizers=_u64(out.w, c), first_pos=_u64(out.p, c), mm_pos=out.mp[:c].cpu().numpy().copy(), sizes=out.sz[:c].cpu().numpy().copy(), hashes=_u64(out.h, c))
    else:
        got.update(positions=_u64(out.p, c))
    return got


def merged_groups(parts):
    """super-k-mer pieces of consecutive ranges put together again: a piece that opens a range continues the piece that closed the range
    before iff it starts at the next k-mer and has the same minimizer occurrence"""
    cat = {f: np.concatenate([p[f] for p in parts]).astype(np.int64 if f in ("mm_pos", "sizes", "first_pos") else np.uint64) for f in K.SK_FIELDS}
    keep = np.ones(len(cat["sizes"]), bool)
    at = 0
    for p in parts[:-1]:
        at += int(p["count"])
        if 0 < at < len(keep) and keep[at]:
            j = at - 1
            while not keep[j]:
                j -= 1
            if (cat["first_pos"][at] == cat["first_pos"][j] + cat["sizes"][j] and cat["first_pos"][at] + cat["mm_pos"][at] == cat["first_pos"][j] + cat["mm_pos"][j]
                    and cat["hashes"][at] == cat["hashes"][j]):
                cat["sizes"][j] += cat["sizes"][at]
                keep[at] = False
    return {f: cat[f][keep] for f in K.SK_FIELDS}


def check_concatenation(r, W, whole, parts, what):
    if r.entry == "super_kmers":
        assert sum(int(p["sizes"].astype(np.int64).sum()) for p in parts) == W.kmers, (what, "the sizes of all ranges sum to the valid k-mers of the batch")
        m = merged_groups(parts)
        for f in K.SK_FIELDS:
            assert np.array_equal(m[f].astype(whole[f].dtype), whole[f]), (what, f)
    else:
        K.assert_same(r.entry, RC.concat(parts, r.entry), whole, what)


def sweep64(ctx, r, inp, sets, origin=0, after_range=None):
    """every range of every cut set against its rule, at exactly the capacity the rule says; the concatenation against the whole scan; on the
    first three-way cut set, every range again one slot short"""
    from biolib_amd import capi

    n = len(inp.seq)
    W = RC.Whole(r, inp)
    whole = W.of_range(0, n, origin) if origin else W.whole()
    batch, out = upload(ctx, inp), Out(n)
    short_done = False
    try:
        ctx.set_exact_windows(r.exact)
        if origin:
            batch.set_origin(origin)
        rc, res = scan64(ctx, batch, r, out, 0, 0, whole["count"], inp.seed)
        assert rc == capi.BL_OK, (K.row_id(r), inp.label, rc)
        K.assert_same(r.entry, got64(r, out, res), whole, (K.row_id(r), inp.label, "whole"))
        assert whole["count"] > (20 if r.entry != "hash_sample" else 5)
        for cuts in sets:
            parts, want = [], []
            for first, end in RC.ranges_of(cuts, n):
                x = W.of_range(first, end, origin)
                rc, res = scan64(ctx, batch, r, out, *RC.call_args(first, end, n), x["count"], inp.seed)
                what = (K.row_id(r), inp.label, cuts, first, end)
                assert rc == capi.BL_OK, (what, "capacity = the expected count", x["count"], "rc", rc, "count", int(res.count))
                got = got64(r, out, res)
                K.assert_same(r.entry, got, x, what)
                if after_range:
                    after_range(cuts, first, end)
                parts.append(got)
                want.append(x)
            check_concatenation(r, W, whole, parts, (K.row_id(r), inp.label, cuts, "concatenation"))
            if len(cuts) == 2 and not short_done:
                short_done = True
                for (first, end), x in zip(RC.ranges_of(cuts, n), want):
                    if x["count"] == 0:
                        continue
                    out.p[x["count"] - 1:x["count"] + 1] = SENT
                    rc, res = scan64(ctx, batch, r, out, *RC.call_args(first, end, n), x["count"] - 1, inp.seed)
                    assert rc == capi.BL_ERR_CAPACITY and int(res.count) == x["count"], (K.row_id(r), cuts, first, "one slot short", rc, int(res.count), x["count"])
                    assert out.p[x["count"] - 1:x["count"] + 1].cpu().numpy().view(np.uint64).tolist() == [SENT, SENT], (K.row_id(r), cuts, first, "written at the capacity")
        assert short_done
    finally:
        ctx.set_exact_windows(False)
        batch.close()


# ----------------------------------------------------------------------------- the 64-bit window scans, position-tiled

POS_ITEMS = [(r, label) for r in RC.POS_ROWS for label in RC.pos_labels(r)]


@pytest.mark.parametrize("r,label", POS_ITEMS, ids=[f"{K.row_id(r)}-{label}" for r, label in POS_ITEMS])
def test_position_tiled_ranges(ctx, r, label):
    inp = [i for i in RC.pos_inputs(r) if i.label == label][0]

    def names(cuts, first, end):
        got = ctx.last_scan_kernels()  # the range takes the kernels the census names for the shape (a second run of pass 1 only where it is needed)
        assert got and got[0] == r.names[0] and got[-1] == r.names[-1] and set(got) <= set(r.names), (K.row_id(r), cuts, first, got)

    sweep64(ctx, r, inp, RC.cut_sets(inp, r.unit, r.w), after_range=names)


# ----------------------------------------------------------------------------- batches of reads: the two layouts in one scan

@pytest.mark.parametrize("r", RC.FRL_ROWS, ids=K.row_id)
def test_read_tiled_ranges(ctx, r):
    """an aligned range records the read-tiled kernels (frl...), any other the position-tiled ones (count...); cut sets that mix the two"""
    inp = RC.frl_input(r)
    L, n = inp.read_len, len(inp.seq)
    layouts = {}

    def names(cuts, first, end):
        got = ctx.last_scan_kernels()
        assert got and got[0].startswith("frl" if RC.read_tiled(first, end, L) else "count"), (K.row_id(r), cuts, first, end, got)
        layouts.setdefault(cuts, []).append(got)

    sweep64(ctx, r, inp, RC.frl_cut_sets(inp, r), after_range=names)
    mixed = {cs: ns for cs, ns in layouts.items() if len({x[0][:3] for x in ns}) == 2}
    assert len(mixed) >= 2, layouts
    cs = sorted(mixed)[0]
    MIXED_NAMES[K.row_id(r)] = (cs, mixed[cs])
    print(f"\n{K.row_id(r)}: cut set {cs} of {n} bases recorded", mixed[cs])


def test_first_scan_of_a_fresh_batch_of_reads_is_an_unaligned_range(ctx):
    """the start bits of a batch of fixed-length reads are built by the first call that needs them: an unaligned range, then an aligned one,
    then the whole batch"""
    from biolib_amd import capi

    r = RC.FRL_ROWS[0]
    inp = RC.frl_input(r)
    L, n = inp.read_len, len(inp.seq)
    W = RC.Whole(r, inp)
    batch, out = upload(ctx, inp), Out(n)
    try:
        for first, end, head in ((L + 5, 7 * L + 1, "count"), (2 * L, 9 * L, "frl"), (0, n, "frl")):
            x = W.of_range(first, end)
            rc, res = scan64(ctx, batch, r, out, *RC.call_args(first, end, n), x["count"], inp.seed)
            assert rc == capi.BL_OK and ctx.last_scan_kernels()[0].startswith(head), (first, end, rc, ctx.last_scan_kernels())
            K.assert_same(r.entry, got64(r, out, res), x, (first, end))
    finally:
        batch.close()


# ----------------------------------------------------------------------------- two lanes, an origin

def test_ranges_on_two_lanes():
    """the three ranges of every three-way cut issued without BL_FLAG_SYNC on a context with its own streams and two lanes, read after sync"""
    import biolib_amd as B
    from biolib_amd import capi

    r = RC.POS_ROWS[0]
    inp = [i for i in RC.pos_inputs(r) if i.label == "ragged"][0]
    n = len(inp.seq)
    W = RC.Whole(r, inp)
    c = B.Context(0, torch_stream=False, lanes=2)
    try:
        batch = upload(c, inp)
        outs = [Out(n) for _ in range(3)]
        c._inputs_ready()
        for cuts in RC.three_way(inp, r.unit, r.w):
            spans = RC.ranges_of(cuts, n)
            want = [W.of_range(a, b) for a, b in spans]
            res = [capi.Result() for _ in spans]
            for (a, b), o, x, rs in zip(spans, outs, want, res):
                rc, _ = scan64(c, batch, r, o, *RC.call_args(a, b, n), x["count"], inp.seed, sync=False, result=rs)
                assert rc == capi.BL_OK
            c.sync()
            parts = [got64(r, o, rs) for o, rs in zip(outs, res)]
            for (a, b), g, x, rs in zip(spans, parts, want, res):
                assert rs.status == 0
                K.assert_same(r.entry, g, x, ("two lanes", cuts, a, b))
            for (a, b), o, g in zip(spans, outs, parts):  # ... and the synchronous call
                rc, rs = scan64(c, batch, r, o, *RC.call_args(a, b, n), int(g["count"]), inp.seed)
                assert rc == capi.BL_OK
                K.assert_same(r.entry, got64(r, o, rs), g, ("two lanes against the synchronous call", cuts, a, b))
        batch.close()
    finally:
        c.close()


@pytest.mark.parametrize("r", [RC.POS_ROWS[0], RC.POS_ROWS[2], RC.POS_ROWS[3]], ids=K.row_id)
def test_ranges_of_a_batch_with_an_origin(ctx, r):
    """positions shift by the origin, `first` stays relative to the batch, the digests follow"""
    inp = RC.pos_inputs(r)[0]
    sweep64(ctx, r, inp, RC.cut_sets(inp, r.unit, r.w), origin=10**12 + 7)


# ----------------------------------------------------------------------------- dense k-mers

@pytest.mark.parametrize("k,drop_last", RC.KMER_SHAPES)
def test_dense_kmer_ranges(ctx, k, drop_last):
    for inp in RC.dense_inputs(k):
        n = len(inp.seq)
        W = RC.WholeKmers(inp, k, True, K.SEED, drop_last)
        batch = upload(ctx, inp)
        try:
            for cuts in RC.cut_sets(inp, k, 1):
                parts = []
                for first, end in RC.ranges_of(cuts, n):
                    f, cnt = RC.call_args(first, end, n)
                    x = W.of_range(first, end)
                    got = batch.kmers(k, seed=K.SEED, canonical=True, drop_last=drop_last, first=f, n=cnt)
                    RC.assert_same_kmers(got, x, (k, drop_last, inp.label, cuts, first, end))
                    dig = batch.kmers(k, seed=K.SEED, canonical=True, drop_last=drop_last, first=f, n=cnt, arrays=False)  # the digest-only form of the kernel
                    assert all(int(dig[d]) == int(x[d]) for d in ("count", "xor_value", "xor_hash", "sum_hash")), (k, drop_last, inp.label, cuts, first, "digest only")
                    parts.append(got)
                assert np.array_equal(np.concatenate([p["values"] for p in parts]), W.values) and np.array_equal(np.concatenate([p["hashes"] for p in parts]), W.hashes)
                assert np.array_equal(np.concatenate([p["valid"] for p in parts]), W.valid) and sum(p["count"] for p in parts) == int(W.valid.sum())
        finally:
            batch.close()


# ----------------------------------------------------------------------------- the 128-bit entries

def scan128(ctx, batch, shape, W, out, first, n, capacity, canonical=True):
    """(rc, got) of one call of a 128-bit entry through the C ABI"""
    import biolib_amd as B
    from biolib_amd import capi

    L = capi.lib()
    entry, a = shape
    flags = (B.FLAG_CANONICAL if canonical else 0) | B.FLAG_SYNC
    res = capi.Result()
    h = (ctx._h, batch._h, first, n)
    if entry == "hash_sample128":
        rc = L.bl_scan_hash_sample128(*h, a[0], RC.SEED128, RC.THRESHOLD128, flags, _ptr(out.w), _ptr(out.p), _ptr(out.h), capacity, C.byref(res))
    elif entry == "minimizers128":
        rc = L.bl_scan_minimizers128(*h, a[0], a[1], RC.SEED128, flags, _ptr(out.w), _ptr(out.p), _ptr(out.h), capacity, C.byref(res))
    elif entry == "syncmers128":
        rc = L.bl_scan_syncmers128(*h, a[0], a[1], W.soff, W.eoff, RC.SEED128, flags, _ptr(out.p), capacity, C.byref(res))
    else:
        rc = L.bl_scan_super_kmer_records128(*h, a[0], a[1], RC.SEED128, flags, _ptr(out.w), _ptr(out.h), capacity, C.byref(res))
    c = min(int(res.count), capacity)
    got = res.as_dict()
    if entry in ("hash_sample128", "minimizers128"):
        got.update(values=_u64(out.w, c, 2), positions=_u64(out.p, c), hashes=_u64(out.h, c))
    elif entry == "syncmers128":
        got.update(positions=_u64(out.p, c))
    else:
        got.update(records=_u64(out.w, c, 4), hashes=_u64(out.h, c))
    return rc, got


ITEMS128 = [(s, label) for s in RC.SHAPES128 for label in ("contig", "ragged", "ragged_n", "breaks")]


@pytest.mark.parametrize("shape,label", ITEMS128, ids=[f"{RC.id128(s)}-{label}" for s, label in ITEMS128])
def test_ranges_128(ctx, shape, label):
    from biolib_amd import capi

    entry, a = shape
    inp = [i for i in RC.inputs128(shape) if i.label == label][0]
    n = len(inp.seq)
    W = RC.Whole128(shape, inp)
    unit, w = (a[0], 1) if len(a) == 1 else ((a[0], a[1]) if entry == "minimizers128" else (a[1], a[0] - a[1] + 1))
    batch, out = upload(ctx, inp), Out(n)
    short_done = False
    try:
        whole = W.of_range(0, n)
        assert whole["count"] > 5
        for cuts in RC.cut_sets(inp, unit, w):
            parts, want = [], []
            for first, end in RC.ranges_of(cuts, n):
                x = W.of_range(first, end)
                what = (RC.id128(shape), label, cuts, first, end)
                if entry == "kmers128":
                    f, cnt = RC.call_args(first, end, n)
                    got = batch.kmers128(a[0], seed=RC.SEED128, canonical=True, first=f, n=cnt)
                    got["values"] = got["values"].reshape(-1, 2)
                    rc = capi.BL_OK
                else:
                    rc, got = scan128(ctx, batch, shape, W, out, *RC.call_args(first, end, n), x["count"])
                assert rc == capi.BL_OK, (what, "capacity = the expected count", x["count"], rc, got["count"])
                RC.assert_same128(entry, got, x, what)
                parts.append(got)
                want.append(x)
            if entry == "records128":  # (clipped pieces: the k-mers of all ranges are the batch's, none twice: the sizes in bits 5..0 of word 3)
                sizes = lambda recs: int(((recs[:, 3] & np.uint64(63)) + np.uint64(1)).sum()) if len(recs) else 0
                assert sum(sizes(p["records"]) for p in parts) == sizes(whole["records"]), (RC.id128(shape), label, cuts)
            else:
                for f in RC.FIELDS128[entry]:
                    assert np.array_equal(np.concatenate([np.asarray(p[f]) for p in parts]), np.asarray(whole[f])), (RC.id128(shape), label, cuts, f, "concatenation")
            if len(cuts) == 2 and not short_done and entry != "kmers128":
                short_done = True
                for (first, end), x in zip(RC.ranges_of(cuts, n), want):
                    if x["count"]:
                        rc, got = scan128(ctx, batch, shape, W, out, *RC.call_args(first, end, n), x["count"] - 1)
                        assert rc == capi.BL_ERR_CAPACITY and got["count"] == x["count"], (RC.id128(shape), cuts, first, "one slot short", rc, got["count"], x["count"])
    finally:
        batch.close()


# ----------------------------------------------------------------------------- packed records, and the counters over ranges

@pytest.mark.parametrize("label", RC.pos_labels(RC.POS_ROWS[2]))
def test_packed_record_ranges(ctx, label):
    """bl_scan_super_kmer_records (k = 31, m = 15): the 16-byte records of every range are superkmer_model.pack of the groups clipped to the
    range, with exactly that many slots; the sizes in the records of a cut set sum to the batch's k-mers"""
    import biolib_amd as B
    from biolib_amd import capi

    r = RC.POS_ROWS[2]
    inp = [i for i in RC.pos_inputs(r) if i.label == label][0]
    n, k = len(inp.seq), r.unit + r.w - 1
    W = RC.Whole(r, inp)
    batch, out = upload(ctx, inp), Out(n)
    try:
        for cuts in RC.cut_sets(inp, r.unit, r.w):
            kmers = 0
            for first, end in RC.ranges_of(cuts, n):
                xr, xh = W.records_of_range(first, end)
                res = capi.Result()
                f, cnt = RC.call_args(first, end, n)
                rc = capi.lib().bl_scan_super_kmer_records(ctx._h, batch._h, f, cnt, k, r.unit, inp.seed, B.FLAG_CANONICAL | B.FLAG_SYNC, _ptr(out.w), _ptr(out.h), len(xh), C.byref(res))
                what = (label, cuts, first, end)
                assert rc == capi.BL_OK and int(res.count) == len(xh), (what, rc, int(res.count), len(xh))
                got = _u64(out.w, len(xh), 2)
                assert np.array_equal(got, xr) and np.array_equal(_u64(out.h, len(xh)), xh), what
                kmers += int(((got[:, 1] & np.uint64(31)) + np.uint64(1)).sum()) if len(got) else 0
            assert kmers == W.kmers, (label, cuts)
    finally:
        batch.close()


def test_counter_over_ranges_16_byte_records(ctx):
    """super_kmer_records(k = 31, m = 15) of a three-way cut, concatenated, through count_super_kmers: the oracle's k-mers of the whole batch, none
    counted twice or lost at a seam"""
    import torch

    r = K._row(("?",), "super_kmers", 15, 17, 1)
    inp = [i for i in RC.pos_inputs(RC.POS_ROWS[2]) if i.label == "ragged"][0]
    n, k = len(inp.seq), 31
    W = RC.Whole(r, inp)
    vals, valid = O.units(inp.seq, inp.offs, k, True)
    want_k, want_c = np.unique(vals[valid.astype(bool)], return_counts=True)
    batch = upload(ctx, inp)
    try:
        for cuts in RC.three_way(inp, r.unit, r.w)[::7]:
            recs, hashes = [], []
            for first, end in RC.ranges_of(cuts, n):
                rr, hh = batch.super_kmer_records(k, 15, seed=inp.seed, canonical=True, first=first, n=end - first)
                xr, xh = W.records_of_range(first, end)
                assert np.array_equal(rr.cpu().numpy().view(np.uint64).reshape(-1, 2), xr) and np.array_equal(hh.cpu().numpy().view(np.uint64), xh), (cuts, first, end)
                recs.append(rr)
                hashes.append(hh)
            keys, cnts = ctx.count_super_kmers(torch.cat(recs), k, 15, seed=inp.seed, canonical=True)
            keys, cnts = keys.cpu().numpy().view(np.uint64), cnts.cpu().numpy()
            order = np.argsort(keys)
            assert np.array_equal(keys[order], want_k) and np.array_equal(cnts[order].astype(np.int64), want_c), cuts
    finally:
        batch.close()


def test_counter_over_ranges_32_byte_records(ctx):
    import torch

    import records128_cases as R

    shape = ("records128", (51, 21))
    inp = [i for i in RC.inputs128(shape) if i.label == "ragged"][0]
    n, k, m = len(inp.seq), 51, 21
    W = RC.Whole128(shape, inp)
    km = RC.Whole128(("kmers128", (k,)), inp).m
    ok = km["valid"].astype(bool)
    want_k, want_c = R.unique_counts128(np.stack([km["hi"][ok], km["lo"][ok]], axis=1))
    batch = upload(ctx, inp)
    try:
        for cuts in RC.three_way(inp, m, k - m + 1)[::7]:
            recs = []
            for first, end in RC.ranges_of(cuts, n):
                rr, hh = batch.super_kmer_records128(k, m, seed=RC.SEED128, canonical=True, first=first, n=end - first)
                x = W.of_range(first, end)
                assert np.array_equal(rr.cpu().numpy().view(np.uint64).reshape(-1, 4), x["records"]) and np.array_equal(hh.cpu().numpy().view(np.uint64), x["hashes"]), (cuts, first)
                recs.append(rr)
            keys, cnts = ctx.count_super_kmers128(torch.cat(recs), k, m, seed=RC.SEED128, canonical=True)
            lo_hi = keys.cpu().numpy().view(np.uint64).reshape(-1, 2)
            got_k, got_c = R.unique_counts128(lo_hi[:, ::-1])
            assert len(got_k) == len(lo_hi), "a k-mer reported twice"
            order = np.lexsort((lo_hi[:, 0], lo_hi[:, 1]))
            assert np.array_equal(got_k, want_k) and np.array_equal(cnts.cpu().numpy()[order].astype(np.int64), want_c.astype(np.int64)), cuts
    finally:
        batch.close()
