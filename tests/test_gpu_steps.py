"""GPU tests of the reads' steps through the compacted graph, the link support and the GAF text (bl_scan_read_steps / bl_link_support /
bl_steps_format_gaf, Batch.read_steps, ReadSteps.link_support / format_gaf / write_gaf) against the Python model of steps_cases.py, word
for word and byte for byte.  The cases are those of the host emulation (test_emu_steps.py), where every index path ran under the
sanitizers.  Every output buffer is longer than the call may write and the rest must keep its fill."""
import ctypes as C

import numpy as np
import pytest

import graph_cases as GC
import links_cases as LK
import lookup_cases as LC
import steps_cases as SC

pytestmark = pytest.mark.gpu
GUARD = 24
FILL32, FILL64, FILL8 = 0x5A5A5A5A, -7, 0xA5
KS = (5, 31, 33, 63)


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.set_option("table_prefix_bits", -1)
    c.close()


def build(ctx, table, key_words, key_bits, option=-1):
    import torch

    keys = sorted(table)
    ctx.set_option("table_prefix_bits", option)
    d_keys = torch.from_numpy(LC.words(keys, key_words).view(np.int64)).cuda()
    d_counts = torch.from_numpy(np.array([table[x] for x in keys], np.uint32).view(np.int32)).cuda()
    t = ctx.count_table(d_keys, d_counts, key_bits=key_bits)
    ctx.set_option("table_prefix_bits", -1)
    return t


def labels(ctx, t, k, once):
    """bl_table_unitigs and bl_unitig_links through the raw bindings"""
    import torch

    n, dev = t.n_distinct, ctx.torch_device
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    nodes = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
    _, n_unitigs, _ = t.unitigs_raw(k, False, offsets, None, nodes, None)
    flags = LK.ONCE if once else 0
    n_links = t.unitig_links_raw(k, nodes, offsets, n_unitigs, flags)
    link_offsets = torch.empty(2 * n_unitigs + 1, dtype=torch.int64, device=dev)
    links = torch.empty((max(n_links, 1), 2), dtype=torch.int32, device=dev)
    t.unitig_links_raw(k, nodes, offsets, n_unitigs, flags, link_offsets, links, n_links)
    return dict(nodes=nodes if n else None, offsets=offsets[:n_unitigs + 1] if n else None, n_unitigs=n_unitigs, link_offsets=link_offsets, links=links, n_links=n_links)


def upload(ctx, batch):
    import torch

    if batch.fixed:
        return ctx.upload(batch.bases, read_len=batch.fixed), None
    b = ctx.upload(batch.bases, offsets=batch.offsets)
    return b, torch.from_numpy(batch.offsets.view(np.int64)).cuda()


def steps_raw(ctx, b, d_offsets, t, k, lab, first=0, n=0):
    """a sizing call, then the records into a guarded buffer -> (host records, stats, the device records)"""
    import torch

    from biolib_amd import capi

    rc, st0 = b.read_steps_raw(t, k, 0, lab["nodes"], lab["offsets"], lab["n_unitigs"], None, 0, first, n, d_offsets)
    assert rc == capi.BL_OK
    n_steps = int(st0.n_steps)
    steps = torch.full((n_steps + GUARD, 4), FILL64, dtype=torch.int64, device=ctx.torch_device)
    rc, st = b.read_steps_raw(t, k, capi.FLAG_CANONICAL if first & 1 else 0, lab["nodes"], lab["offsets"], lab["n_unitigs"], steps, n_steps, first, n, d_offsets)
    assert rc == capi.BL_OK and st.as_dict() == st0.as_dict(), "the sizing call counts what the full call writes"
    host = steps.cpu().numpy()
    assert (host[n_steps:] == FILL64).all(), "guard words behind the records"
    return host[:n_steps].copy().view(SC.STEP).reshape(-1), st.as_dict(), steps[:n_steps]


def support_raw(ctx, d_steps, lab):
    import torch

    from biolib_amd import capi

    n_links, n_steps = lab["n_links"], int(d_steps.shape[0])
    sup = torch.full((n_links + GUARD,), FILL32, dtype=torch.int32, device=ctx.torch_device)
    st = capi.SupportStats()
    capi.check(ctx._lib.bl_link_support(ctx._h, C.c_void_p(d_steps.data_ptr()) if n_steps else None, n_steps, C.c_void_p(lab["link_offsets"].data_ptr()),
                                        C.c_void_p(lab["links"].data_ptr()) if n_links else None, n_links, lab["n_unitigs"],
                                        C.c_void_p(sup.data_ptr()) if n_links else None, C.byref(st)))
    host = sup.cpu().numpy().view(np.uint32)
    assert (host[n_links:] == FILL32).all(), "guard words behind the supports"
    return host[:n_links], st.as_dict()


def gaf_call(ctx, b, d_offsets, d_steps, lab, k, rule, out, capacity):
    from biolib_amd import capi

    r = capi.GafRule()
    r.flags, r.k, r.read_prefix, r.read_first_number, r.segment_prefix, r.segment_first_number = 0, k, rule[0].encode("latin1"), rule[1], rule[2].encode("latin1"), rule[3]
    nb, n_steps = C.c_uint64(12345), int(d_steps.shape[0])
    rc = ctx._lib.bl_steps_format_gaf(ctx._h, b._h, C.c_void_p(d_offsets.data_ptr()) if d_offsets is not None else None,
                                      C.c_void_p(d_steps.data_ptr()) if n_steps else None, n_steps,
                                      C.c_void_p(lab["offsets"].data_ptr()) if lab["offsets"] is not None else None, lab["n_unitigs"], C.byref(r),
                                      C.c_void_p(out.data_ptr()) if out is not None else None, capacity, C.byref(nb))
    return rc, int(nb.value)


def gaf_raw(ctx, b, d_offsets, d_steps, lab, k, rule):
    """a sizing call, then the text into a guarded buffer -> bytes"""
    import torch

    from biolib_amd import capi

    rc, n_bytes = gaf_call(ctx, b, d_offsets, d_steps, lab, k, rule, None, 0)
    capi.check(rc)
    out = torch.full((n_bytes + GUARD,), FILL8, dtype=torch.uint8, device=ctx.torch_device)
    rc, again = gaf_call(ctx, b, d_offsets, d_steps, lab, k, rule, out, n_bytes)
    capi.check(rc)
    assert again == n_bytes, "the sizing call agrees with the full call"
    host = out.cpu().numpy()
    assert (host[n_bytes:] == FILL8).all(), "guard bytes behind the text"
    return host[:n_bytes].tobytes()


def same(ctx, t, k, m, batch, once, rule, tag, ranges=((0, 0),)):
    lab = labels(ctx, t, k, once)
    assert lab["n_unitigs"] == len(m["strings"])
    lk = LK.links(m, k, once=once)
    b, d_offsets = upload(ctx, batch)
    nodes = SC.position_nodes(m, k, batch)
    for first, n in ranges:
        want, stats = SC.steps(m, k, batch, first, n, nodes)
        got, st, d_steps = steps_raw(ctx, b, d_offsets, t, k, lab, first, n)
        assert np.array_equal(got, want), (tag, first, n, "steps")
        assert st == stats, (tag, first, n, st, stats)
        if (first, n) == (0, 0):
            sup, sstats = SC.support(want, lk["records"])
            got_sup, got_stats = support_raw(ctx, d_steps, lab)
            assert np.array_equal(got_sup, sup) and got_stats == sstats, (tag, "support")
            assert gaf_raw(ctx, b, d_offsets, d_steps, lab, k, rule) == b"".join(SC.gaf_lines(m, k, batch, want, *rule)), (tag, "text")
    b.close()


@pytest.mark.parametrize("k", KS)
def test_named_cases(ctx, k):
    for c, (name, table) in enumerate(GC.cases(k)):
        m = GC.model(table, k)
        for w, (key_words, key_bits) in enumerate(GC.widths(k)):
            t = build(ctx, table, key_words, key_bits)
            for f, (form, batch) in enumerate(SC.batches_for(name, table, k, m)):
                ranges = ((0, 0), (batch.n_bases // 3, batch.n_bases // 2), (batch.n_bases, 0))
                same(ctx, t, k, m, batch, bool((c + w + f) & 1), SC.GAF_RULES[(c + f) % len(SC.GAF_RULES)], (name, k, key_words, form), ranges)
            t.close()


@pytest.mark.parametrize("option", (0, 1, 24))
def test_forced_prefix_bits(ctx, option):
    for name in ("fork", "hairpin", "pure_cycle", "random_keys", "empty"):
        table = dict(GC.cases(31))[name]
        m = GC.model(table, 31)
        for key_words in (1, 2):
            t = build(ctx, table, key_words, 62, option)
            same(ctx, t, 31, m, SC.batches_for(name, table, 31, m)[0][1], False, SC.GAF_RULES[1], (name, option, key_words))
            t.close()


# twelve seeded cuts and the cuts around a lane's and a tile's seam
CUTS = sorted(int(c) for c in np.random.default_rng(12).integers(1, 12399, 12)) + [15, 16, 17, 4095, 4096, 4097]


def test_seam_batch_and_cuts(ctx):
    table, m, batch = SC.seam_case()
    k = SC.SEAM_K
    t = build(ctx, table, 1, 62)
    same(ctx, t, k, m, batch, False, SC.GAF_RULES[0], "seams")
    lab = labels(ctx, t, k, False)
    b, d_offsets = upload(ctx, batch)
    nodes = SC.position_nodes(m, k, batch)
    whole, stats = SC.steps(m, k, batch, 0, 0, nodes)
    continued = 0
    for c in CUTS:
        left, sl, _ = steps_raw(ctx, b, d_offsets, t, k, lab, 0, c)
        right, sr, _ = steps_raw(ctx, b, d_offsets, t, k, lab, c, 0)
        assert np.array_equal(left, SC.steps(m, k, batch, 0, c, nodes)[0]) and np.array_equal(right, SC.steps(m, k, batch, c, 0, nodes)[0]), c
        assert np.array_equal(SC.fold(list(left) + list(right)), whole), (c, "the two ranges fold to the whole")
        assert sl["n_valid"] + sr["n_valid"] == stats["n_valid"] and sl["n_found"] + sr["n_found"] == stats["n_found"], c
        continued += len(right) > 0 and bool(int(right[0]["flags"]) & SC.CONTINUED)
    assert continued > 0
    b.close()
    t.close()


def failed(call, code):
    import biolib_amd

    with pytest.raises(biolib_amd.BiolibError) as e:
        call()
    assert e.value.code == code and len(str(e.value).split(": ", 1)[1]) > 5, e.value
    return str(e.value)


def test_capacity_leaves_the_output_untouched(ctx):
    import torch

    from biolib_amd import capi

    name, k = "fork", 31
    table = dict(GC.cases(k))[name]
    m = GC.model(table, k)
    batch = SC.batches_for(name, table, k, m)[0][1]
    want, stats = SC.steps(m, k, batch)
    t = build(ctx, table, 1, 62)
    lab = labels(ctx, t, k, False)
    b, d_offsets = upload(ctx, batch)
    for capacity in (len(want) - 1, 0):
        steps = torch.full((len(want) + GUARD, 4), FILL64, dtype=torch.int64, device=ctx.torch_device)
        rc, st = b.read_steps_raw(t, k, 0, lab["nodes"], lab["offsets"], lab["n_unitigs"], steps, capacity, 0, 0, d_offsets)
        assert rc == capi.BL_ERR_CAPACITY and st.as_dict() == stats, "complete stats in front of the refusal"
        assert bool((steps == FILL64).all()), "d_steps untouched"
    _, _, d_steps = steps_raw(ctx, b, d_offsets, t, k, lab)
    text = b"".join(SC.gaf_lines(m, k, batch, want, *SC.GAF_RULES[0]))
    for capacity in (len(text) - 1, 0):
        out = torch.full((len(text) + GUARD,), FILL8, dtype=torch.uint8, device=ctx.torch_device)
        rc, n_bytes = gaf_call(ctx, b, d_offsets, d_steps, lab, k, SC.GAF_RULES[0], out, capacity)
        assert rc == capi.BL_ERR_CAPACITY and n_bytes == len(text), "*n_bytes is written in front of the refusal"
        assert bool((out == FILL8).all()), "d_out untouched"
    b.close()
    t.close()


def test_refusals(ctx):
    import torch

    import biolib_amd
    from biolib_amd import capi

    name, k = "fork", 31
    table = dict(GC.cases(k))[name]
    m = GC.model(table, k)
    batch = SC.batches_for(name, table, k, m)[0][1]
    t = build(ctx, table, 1, 62)
    t60 = build(ctx, {x: 1 for x in list(table)[:3] if x < (1 << 60)} or {1: 1}, 1, 60)
    lab = labels(ctx, t, k, False)
    b, d_offsets = upload(ctx, batch)
    single = ctx.upload("ACGT" * 30)
    other = biolib_amd.Context(0)
    foreign = other.upload("ACGT" * 30)
    steps = torch.zeros((64, 4), dtype=torch.int64, device=ctx.torch_device)
    args = dict(table=t, k=k, flags=0, nodes=lab["nodes"], unitig_offsets=lab["offsets"], n_unitigs=lab["n_unitigs"], steps=steps, capacity=64, first=0, n=0,
                offsets=d_offsets)

    def scan(batch=b, **kw):
        return lambda: batch.read_steps_raw(**{**args, **kw})

    for kk in (0, 1, 2, 30, 64, 65):
        assert "odd" in failed(scan(k=kk), capi.BL_ERR_INVALID)
    assert "key_bits" in failed(scan(table=t60), capi.BL_ERR_INVALID), "a table too narrow for k"
    assert "key_bits" in failed(scan(k=33), capi.BL_ERR_INVALID), "a table of one-word keys holds at most 64 bits"
    assert "another context" in failed(scan(batch=foreign), capi.BL_ERR_INVALID)
    assert "d_nodes" in failed(scan(nodes=None), capi.BL_ERR_INVALID)
    assert "d_nodes" in failed(scan(unitig_offsets=None), capi.BL_ERR_INVALID)
    assert "n_unitigs" in failed(scan(n_unitigs=len(table) + 1), capi.BL_ERR_INVALID)
    assert "d_offsets" in failed(scan(offsets=None), capi.BL_ERR_INVALID)
    assert "aligned" in failed(scan(steps=steps.view(-1)[1:]), capi.BL_ERR_INVALID)
    assert "capacity" in failed(scan(steps=None), capi.BL_ERR_INVALID)
    assert "flags" in failed(scan(flags=capi.FLAG_DROP_LAST), capi.BL_ERR_INVALID)
    assert "flags" in failed(scan(flags=1 << 9), capi.BL_ERR_INVALID)
    assert "beyond" in failed(scan(first=batch.n_bases + 1), capi.BL_ERR_INVALID)
    rc, st = b.read_steps_raw(**{**args, "flags": capi.FLAG_CANONICAL | capi.FLAG_SYNC})
    assert rc == capi.BL_OK and st.n_steps == len(SC.steps(m, k, batch)[0]), "both accepted flags"
    rc, st = single.read_steps_raw(**{**args, "offsets": None})
    assert rc == capi.BL_OK, "a single sequence needs no offsets"
    assert "NULL" in failed(lambda: capi.check(ctx._lib.bl_scan_read_steps(ctx._h, None, 0, 0, k, 0, t._h, None, None, 0, None, None, 0, None)), capi.BL_ERR_INVALID)
    assert "another context" in failed(lambda: capi.check(ctx._lib.bl_scan_read_steps(other._h, foreign._h, 0, 0, k, 0, t._h, None, None, 0, None, None, 0, None)),
                                       capi.BL_ERR_INVALID), "a foreign table"

    # the text
    _, _, d_steps = steps_raw(ctx, b, d_offsets, t, k, lab)
    out = torch.zeros(4096, dtype=torch.uint8, device=ctx.torch_device)

    def gaf(rule=SC.GAF_RULES[0], kk=k, steps=d_steps, out=out, offsets=d_offsets, batch=b, flags=0, reserved=0):
        def call():
            r = capi.GafRule()
            r.flags, r.k, r.read_prefix, r.segment_prefix, r.reserved = flags, kk, rule[0].encode("latin1"), rule[2].encode("latin1"), reserved
            nb = C.c_uint64()
            capi.check(ctx._lib.bl_steps_format_gaf(ctx._h, batch._h, C.c_void_p(offsets.data_ptr()) if offsets is not None else None,
                                                    C.c_void_p(steps.data_ptr()), int(steps.shape[0]), C.c_void_p(lab["offsets"].data_ptr()), lab["n_unitigs"],
                                                    C.byref(r), C.c_void_p(out.data_ptr()), 4096, C.byref(nb)))
        return call

    assert "flag" in failed(gaf(flags=1), capi.BL_ERR_INVALID)
    assert "odd" in failed(gaf(kk=30), capi.BL_ERR_INVALID)
    assert "NUL" in failed(gaf(rule=("0123456789abcdef", 0, "", 0)), capi.BL_ERR_INVALID)
    assert "NUL" in failed(gaf(rule=("", 0, "0123456789abcdef", 0)), capi.BL_ERR_INVALID)
    assert "reserved" in failed(gaf(reserved=1), capi.BL_ERR_INVALID)
    assert "aligned" in failed(gaf(out=out[1:]), capi.BL_ERR_INVALID)
    assert "d_offsets" in failed(gaf(offsets=None), capi.BL_ERR_INVALID)
    assert "another context" in failed(gaf(batch=foreign), capi.BL_ERR_INVALID)
    cut = d_steps.clone()
    cut.view(torch.int32)[3, 7] |= SC.CONTINUED
    assert "CONTINUED" in failed(gaf(steps=cut), capi.BL_ERR_INVALID), "the caller folds first"
    # the support
    assert "d_link_offsets" in failed(lambda: capi.check(ctx._lib.bl_link_support(ctx._h, C.c_void_p(d_steps.data_ptr()), int(d_steps.shape[0]), None, None, 0, 3, None,
                                                                                   None)), capi.BL_ERR_INVALID)
    assert "d_steps" in failed(lambda: capi.check(ctx._lib.bl_link_support(ctx._h, None, 5, None, None, 0, 0, None, None)), capi.BL_ERR_INVALID)
    for x in (foreign, single, b, t60, t):
        x.close()
    other.close()


def test_empty_batch_range_and_table(ctx):
    import torch

    from biolib_amd import capi

    empty_table = ctx.count_table(torch.zeros(0, dtype=torch.int64, device="cuda"), key_bits=62)
    b = ctx.upload("ACGT" * 40)
    rc, st = b.read_steps_raw(empty_table, 31, 0, None, None, 0, None, 0)
    assert rc == capi.BL_OK and st.as_dict() == dict(n_valid=130, n_found=0, n_steps=0, n_chains=0, n_linked=0, longest_step=0)
    table = dict(GC.cases(31))["fork"]
    t = build(ctx, table, 1, 62)
    lab = labels(ctx, t, 31, False)
    rc, st = b.read_steps_raw(t, 31, 0, lab["nodes"], lab["offsets"], lab["n_unitigs"], None, 0, 160, 0)
    assert rc == capi.BL_OK and st.as_dict() == dict.fromkeys(SC.STEP_STAT_NAMES, 0), "an empty range"
    nothing = ctx.upload("")
    rc, st = nothing.read_steps_raw(t, 31, 0, lab["nodes"], lab["offsets"], lab["n_unitigs"], None, 0)
    assert rc == capi.BL_OK and st.as_dict() == dict.fromkeys(SC.STEP_STAT_NAMES, 0), "an empty batch"
    for x in (nothing, b, t, empty_table):
        x.close()


def test_kernel_timing_counts_the_node_pass(ctx):
    """with bl_ctx_kernel_timing on, every call adds its node pass to bl_ctx_kernel_time as one launch"""
    table = dict(GC.cases(31))["fork"]
    m = GC.model(table, 31)
    t = build(ctx, table, 1, 62)
    lab = labels(ctx, t, 31, False)
    b, d_offsets = upload(ctx, SC.batches_for("fork", table, 31, m)[0][1])
    ctx.kernel_timing(True)
    for _ in range(2):
        b.read_steps_raw(t, 31, 0, lab["nodes"], lab["offsets"], lab["n_unitigs"], None, 0, 0, 0, d_offsets)
    ms, launches = ctx.kernel_time()
    ctx.kernel_timing(False)
    assert launches == 2 and ms > 0
    b.read_steps_raw(t, 31, 0, lab["nodes"], lab["offsets"], lab["n_unitigs"], None, 0, 0, 0, d_offsets)
    assert ctx.kernel_time() == (0.0, 0), "nothing is recorded with the timing off"
    b.close()
    t.close()


def simulated_reads():
    """a 4-kbp genome with a planted 300-bp repeat (the branching that cleaning leaves: reads cross its links) and a second haplotype (a
    SNP every 500 bases); 12x reads of 100 bp from both strands and haplotypes, 1 % substitutions"""
    rng = np.random.default_rng(20261021)
    g = GC._rand_seq(rng, 4000)
    g = g[:2400] + g[600:900] + g[2700:]
    h = list(g)
    for p in range(250, len(g), 500):
        h[p] = GC._other(h[p])
    h = "".join(h)
    reads = []
    for i in range(12 * len(g) // 100):
        p = int(rng.integers(0, len(g) - 100 + 1))
        r = list((g, h)[i & 1][p:p + 100])
        for q in np.nonzero(rng.random(100) < 0.01)[0]:
            r[q] = GC._other(r[q], int(rng.integers(1, 4)))
        r = "".join(r)
        reads.append(GC.revcomp(r) if rng.random() < 0.5 else r)
    return reads


def test_python_surface_on_simulated_reads(ctx, tmp_path):
    import torch

    k = 21
    reads = SC.Reads(simulated_reads(), 100)
    b = ctx.upload(reads.bases, read_len=100)
    scan = b.kmers(k, canonical=True)
    values = scan["values"][scan["valid"] != 0]
    counted = ctx.count_table(torch.from_numpy(np.ascontiguousarray(values).view(np.int64)).cuda(), key_bits=2 * k)
    solid = counted.filter(2)
    cleaned, _ = solid.clean(k)
    table = dict(zip((int(x) for x in cleaned.keys.cpu().numpy().view(np.uint64)), (int(x) for x in cleaned.counts.cpu().numpy().view(np.uint32))))
    m = GC.model(table, k)
    u = cleaned.unitigs(k, links=True)
    assert u.n_unitigs == len(m["strings"])
    rs = b.read_steps(u)
    want, stats = SC.steps(m, k, reads)
    assert np.array_equal(rs.host(), want) and rs.stats == stats and rs.n_steps == len(want)
    assert stats["n_linked"] > 10 and stats["n_found"] < stats["n_valid"], "reads cross links, and erroneous k-mers have no node"
    chunked = b.read_steps(u, chunk_positions=10000)
    assert np.array_equal(chunked.host(), want) and chunked.stats == stats, "chunks that end on read boundaries: no CONTINUED"
    sup, sstats = rs.link_support()
    want_sup, want_sstats = SC.support(want, LK.links(m, k)["records"])
    assert np.array_equal(sup.cpu().numpy().view(np.uint32), want_sup) and sstats == want_sstats
    text = b"".join(SC.gaf_lines(m, k, reads, want, "read", 1, "utg", 7))
    names = dict(read_prefix="read", read_first_number=1, segment_prefix="utg", segment_first_number=7)
    assert rs.write_gaf(tmp_path / "walks.gaf", **names) == len(text) and (tmp_path / "walks.gaf").read_bytes() == text
    rs.write_gaf(tmp_path / "walks.gaf.gz", compress=True, **names)
    inflated, status = ctx.bgzf_inflate((tmp_path / "walks.gaf.gz").read_bytes())
    assert not status.any() and inflated.tobytes() == text, "the BGZF file inflates to the model's text"
    for x in (b, cleaned, solid, counted):
        x.close()
