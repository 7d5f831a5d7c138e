"""GPU tests of the unitig links and the GFA text (bl_unitig_links / bl_unitigs_format_gfa, CountTable.unitigs(links=True), Unitigs.format_gfa /
write_gfa) against the Python model of links_cases.py, word for word and byte for byte.  The cases are those of the host emulation
(test_emu_links.py), where every index path ran under the sanitizers.  Every output buffer is longer than the call may write and the rest
must keep its fill."""
import ctypes as C
import functools

import numpy as np
import pytest

import graph_cases as GC
import links_cases as LK
import lookup_cases as LC

pytestmark = pytest.mark.gpu
GUARD = 24
FILL32, FILL64, FILL8 = 0x5A5A5A5A, -7, 0xA5


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


def labels(ctx, t, k):
    """bl_table_unitigs through the raw binding: what the links take (nodes, offsets, n_unitigs) and the batch"""
    import torch

    from biolib_amd.scan import Batch

    n, dev = t.n_distinct, ctx.torch_device
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    sums = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    nodes = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
    h, n_unitigs, n_bases = t.unitigs_raw(k, True, offsets, sums, nodes, None)
    return dict(nodes=nodes, offsets=offsets[:n_unitigs + 1], sums=sums[:n_unitigs], n_unitigs=n_unitigs, batch=Batch(ctx, h))


def links_raw(ctx, t, k, lab, flags):
    """a sizing call, then the records into guarded buffers -> (host records [n, 2], host offsets, stats, the device records)"""
    import torch

    from biolib_amd import capi

    dev, nu = ctx.torch_device, lab["n_unitigs"]
    st0 = capi.LinkStats()
    n_links = t.unitig_links_raw(k, lab["nodes"], lab["offsets"], nu, flags, None, None, 0, st0)
    link_offsets = torch.full((2 * nu + 1 + GUARD,), FILL64, dtype=torch.int64, device=dev)
    links = torch.full((n_links + GUARD, 2), FILL32, dtype=torch.int32, device=dev)
    st = capi.LinkStats()
    assert t.unitig_links_raw(k, lab["nodes"], lab["offsets"], nu, flags, link_offsets, links, n_links, st) == n_links
    assert st.as_dict() == st0.as_dict(), "the sizing call counts what the full call writes"
    h_off, h_links = link_offsets.cpu().numpy(), links.cpu().numpy().view(np.uint32)
    assert (h_off[2 * nu + 1:] == FILL64).all() and (h_links[n_links:] == FILL32).all(), "guard words behind offsets and records"
    return h_links[:n_links], h_off[:2 * nu + 1], st.as_dict(), links[:n_links]


def gfa_raw(ctx, lab, d_links, k, prefix, first_number, header, sums=True):
    """a sizing call, then the text into a guarded buffer -> bytes"""
    import torch

    from biolib_amd import capi

    rule = capi.GfaRule()
    rule.flags, rule.k, rule.name_prefix, rule.first_number = (0 if header else capi.GFA_NO_HEADER), k, prefix.encode("latin1"), first_number
    n_links = int(d_links.shape[0])

    def call(out, capacity):
        nb = C.c_uint64()
        capi.check(ctx._lib.bl_unitigs_format_gfa(ctx._h, lab["batch"]._h, C.c_void_p(lab["offsets"].data_ptr()), lab["n_unitigs"],
                                                  C.c_void_p(lab["sums"].data_ptr()) if sums and lab["n_unitigs"] else None,
                                                  C.c_void_p(d_links.data_ptr()) if n_links else None, n_links, C.byref(rule),
                                                  C.c_void_p(out.data_ptr()) if out is not None else None, capacity, C.byref(nb)))
        return int(nb.value)

    n_bytes = call(None, 0)
    out = torch.full((n_bytes + GUARD,), FILL8, dtype=torch.uint8, device=ctx.torch_device)
    assert call(out, n_bytes) == n_bytes
    host = out.cpu().numpy()
    assert (host[n_bytes:] == FILL8).all(), "guard bytes behind the text"
    return host[:n_bytes].tobytes()


def same(ctx, t, k, m, rule, tag):
    lab = labels(ctx, t, k)
    assert lab["n_unitigs"] == len(m["strings"])
    for flags in (0, LK.ONCE):
        want = LK.links(m, k, once=bool(flags))
        got, off, st, d_links = links_raw(ctx, t, k, lab, flags)
        assert np.array_equal(got, want["array"]), (tag, flags, "links")
        assert off.tolist() == want["offsets"], (tag, flags, "offsets")
        assert st == want["stats"], (tag, flags, st, want["stats"])
        text = gfa_raw(ctx, lab, d_links, k, *rule)
        assert text == LK.GfaText(LK.gfa_lines(m, want["records"], k, *rule)).bytes(), (tag, flags, "text")
    lab["batch"].close()


@pytest.mark.parametrize("k", LK.KS)
def test_named_cases(ctx, k):
    for c, (name, table) in enumerate(GC.cases(k)):
        m = GC.model(table, k)
        for key_words, key_bits in GC.widths(k):
            for o, option in enumerate(GC.OPTIONS):
                t = build(ctx, table, key_words, key_bits, option)
                same(ctx, t, k, m, LK.RULES[(c + o) % len(LK.RULES)], (name, k, key_words, option))
                t.close()


@pytest.mark.parametrize("name", [c[0] for c in LK.dense_cases()])
def test_dense_cases(ctx, name):
    """many branching ends; the largest has more than 10,000 unitigs: names of one to five digits"""
    k, table, m = LK.dense_model(name)
    t = build(ctx, table, 1, 2 * k)
    same(ctx, t, k, m, LK.RULES[0] if name != "dense_300_of_512" else LK.RULES[3], name)
    t.close()


@functools.lru_cache(maxsize=None)
def forked_model(n_forks, cycle):
    return GC.model(LK.forked_path(n_forks, cycle), 31)


# unitigs 2f + 1 (+ 1), so ends 62, 64, 66 and 254, 256, 258 and search threads (ends + 1) 63, 65, 67 and 255, 257, 259: ends are even;
# records 4f (+ 2), with ONCE 2f (+ 1): 63, 64, 65 and 255, 256, 257 among them
FORKS = ((15, False), (15, True), (16, False), (31, True), (32, False), (32, True), (63, False), (63, True), (64, False), (127, True), (128, False), (128, True))


@pytest.mark.parametrize("n_forks,cycle", FORKS)
def test_counts_around_a_wave_and_a_workgroup(ctx, n_forks, cycle):
    m = forked_model(n_forks, cycle)
    full, once = LK.links(m, 31), LK.links(m, 31, once=True)
    extra = 1 if cycle else 0
    assert full["stats"]["n_ends"] == 4 * n_forks + 2 + 2 * extra and len(full["records"]) == 4 * n_forks + 2 * extra and len(once["records"]) == 2 * n_forks + extra
    for key_words in (1, 2):
        t = build(ctx, LK.forked_path(n_forks, cycle), key_words, 62)
        same(ctx, t, 31, m, LK.RULES[1 + key_words], (n_forks, cycle, key_words))
        t.close()


def test_reruns_are_bit_equal(ctx):
    k, table, m = LK.dense_model("dense_5000_of_8192")
    t = build(ctx, table, 1, 2 * k)
    lab = labels(ctx, t, k)
    first = None
    for _ in range(3):
        got, off, st, d_links = links_raw(ctx, t, k, lab, 0)
        text = gfa_raw(ctx, lab, d_links, k, "x", 7, True)
        run = (got.tobytes(), off.tobytes(), tuple(st.items()), text)
        first = first or run
        assert run == first
    lab["batch"].close()
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

    k, table, m = LK.dense_model("dense_300_of_512")
    t = build(ctx, table, 1, 2 * k)
    lab = labels(ctx, t, k)
    want = LK.links(m, k)
    n_links = len(want["records"])
    for capacity in (n_links - 1, 0):
        links = torch.full((n_links + GUARD, 2), FILL32, dtype=torch.int32, device=ctx.torch_device)
        nl = C.c_uint64(12345)
        rc = ctx._lib.bl_unitig_links(ctx._h, t._h, k, C.c_void_p(lab["nodes"].data_ptr()), C.c_void_p(lab["offsets"].data_ptr()), lab["n_unitigs"], 0, None,
                                      C.c_void_p(links.data_ptr()), capacity, C.byref(nl), None)
        assert rc == capi.BL_ERR_CAPACITY and nl.value == n_links, "*n_links is written in front of the refusal"
        assert bool((links.view(-1) == FILL32).all()), "d_links untouched"
    got, _, _, d_links = links_raw(ctx, t, k, lab, 0)
    text = LK.GfaText(LK.gfa_lines(m, want["records"], k)).bytes()
    rule = capi.GfaRule()
    rule.k = k
    for capacity in (len(text) - 1, 0):
        out = torch.full((len(text) + GUARD,), FILL8, dtype=torch.uint8, device=ctx.torch_device)
        nb = C.c_uint64(12345)
        rc = ctx._lib.bl_unitigs_format_gfa(ctx._h, lab["batch"]._h, C.c_void_p(lab["offsets"].data_ptr()), lab["n_unitigs"], C.c_void_p(lab["sums"].data_ptr()),
                                            C.c_void_p(d_links.data_ptr()), n_links, C.byref(rule), C.c_void_p(out.data_ptr()), capacity, C.byref(nb))
        assert rc == capi.BL_ERR_CAPACITY and nb.value == len(text)
        assert bool((out == FILL8).all()), "d_out untouched"
    lab["batch"].close()
    t.close()


def test_empty_table(ctx, tmp_path):
    import torch

    t = ctx.count_table(torch.zeros(0, dtype=torch.int64, device="cuda"), key_bits=62)
    u = t.unitigs(31, links=True)
    assert u.links.shape == (0, 2) and u.link_offsets.cpu().tolist() == [0]
    assert u.link_stats == dict.fromkeys(LK.LINK_STAT_NAMES, 0)
    assert bytes(u.format_gfa().cpu().numpy()) == LK.HEADER, "only the header line"
    assert u.format_gfa(header=False).numel() == 0
    assert u.write_gfa(tmp_path / "empty.gfa") == len(LK.HEADER) and (tmp_path / "empty.gfa").read_bytes() == LK.HEADER
    t.close()


def test_methods_and_defaults(ctx, tmp_path):
    k, table, m = LK.dense_model("dense_300_of_512")
    t = build(ctx, table, 1, 2 * k)
    plain = t.unitigs(k)
    assert plain.links is None and plain.link_offsets is None and plain.link_stats is None and plain.nodes is None, "the defaults are unchanged"
    with pytest.raises(ValueError):
        plain.write_gfa(tmp_path / "no_links.gfa")
    with pytest.raises(ValueError):
        t.unitigs(k, batch=False, links=True).write_gfa(tmp_path / "no_batch.gfa")
    for once in (False, True):
        want = LK.links(m, k, once)
        u = t.unitigs(k, links=True, once=once)
        assert u.nodes is None
        assert np.array_equal(u.links.cpu().numpy().view(np.uint32), want["array"]) and u.link_offsets.cpu().tolist() == want["offsets"]
        assert u.link_stats == want["stats"]
        text = LK.GfaText(LK.gfa_lines(m, want["records"], k, "utg", 5, True)).bytes()
        assert bytes(u.format_gfa("utg", 5).cpu().numpy()) == text
        assert u.write_gfa(tmp_path / "g.gfa", prefix="utg", first_number=5) == len(text) and (tmp_path / "g.gfa").read_bytes() == text
    t.close()


def test_refusals(ctx):
    import torch

    import biolib_amd
    from biolib_amd import capi

    INV = capi.BL_ERR_INVALID
    t1 = build(ctx, GC.path_case(5), 1, 62)
    t2 = build(ctx, GC.path_case(5), 2, 128)
    lab = labels(ctx, t1, 31)
    nodes, offs, nu = C.c_void_p(lab["nodes"].data_ptr()), C.c_void_p(lab["offsets"].data_ptr()), lab["n_unitigs"]
    lib = ctx._lib

    def links(ctx_h=ctx._h, table=t1, k=31, d_nodes=nodes, d_offs=offs, n_unitigs=nu, flags=0):
        nl = C.c_uint64(99)
        rc = lib.bl_unitig_links(ctx_h, table._h if table is not None else None, k, d_nodes, d_offs, n_unitigs, flags, None, None, 0, C.byref(nl), None)
        assert rc == capi.BL_OK or nl.value == 0, "*n_links is written on a refusal too"
        capi.check(rc)

    links()
    for t in (t1, t2):
        for k in (0, 1, 2, 30, 32, 64, 65, 1 << 20):
            failed(lambda: links(table=t, k=k), INV)
    assert "k = 1" in failed(lambda: links(k=1), INV)
    failed(lambda: links(ctx_h=None), INV)
    failed(lambda: links(table=None), INV)
    failed(lambda: links(flags=2), INV)
    failed(lambda: links(flags=1 << 31), INV)
    failed(lambda: links(d_nodes=None), INV)
    failed(lambda: links(d_offs=None), INV)
    failed(lambda: links(n_unitigs=6), INV)               # more unitigs than keys
    narrow = build(ctx, {3: 1}, 1, 40)
    one64 = build(ctx, {3: 1}, 1, 64)
    failed(lambda: links(table=narrow, k=21), INV)        # 2k above key_bits
    failed(lambda: links(table=one64, k=33), INV)         # one-word keys, k > 31
    other = biolib_amd.Context(0)
    foreign = build(other, GC.path_case(5), 1, 62)
    failed(lambda: links(table=foreign), INV)
    foreign_lab = labels(other, foreign, 31)

    out = torch.zeros(4096, dtype=torch.uint8, device=ctx.torch_device)

    def gfa(ctx_h=ctx._h, batch=lab["batch"], k=31, flags=0, prefix=b"", reserved=0, d_out=out.data_ptr(), d_offs=offs, n_links=0, no_rule=False):
        rule = capi.GfaRule()
        rule.flags, rule.k, rule.name_prefix, rule.reserved = flags, k, prefix, reserved
        nb = C.c_uint64(99)
        rc = lib.bl_unitigs_format_gfa(ctx_h, batch._h if batch is not None else None, d_offs, nu, None, None, n_links, None if no_rule else C.byref(rule),
                                       C.c_void_p(d_out) if d_out else None, 4096, C.byref(nb))
        assert rc == capi.BL_OK or nb.value == 0
        capi.check(rc)

    gfa()
    for k in (0, 1, 2, 30, 64, 65):
        failed(lambda: gfa(k=k), INV)
    failed(lambda: gfa(ctx_h=None), INV)
    failed(lambda: gfa(batch=None), INV)
    failed(lambda: gfa(no_rule=True), INV)
    failed(lambda: gfa(flags=2), INV)
    failed(lambda: gfa(prefix=b"sixteen_bytes_no0"[:16]), INV)
    failed(lambda: gfa(reserved=1), INV)
    failed(lambda: gfa(d_out=out.data_ptr() + 8), INV)    # not 16-byte aligned
    failed(lambda: gfa(d_offs=None), INV)
    failed(lambda: gfa(n_links=1), INV)                   # d_links NULL with records
    failed(lambda: gfa(batch=foreign_lab["batch"]), INV)  # a batch of another context
    foreign_lab["batch"].close()
    foreign.close()
    other.close()
    lab["batch"].close()
    for t in (t1, t2, narrow, one64):
        t.close()


@functools.lru_cache(maxsize=None)
def reads_case():
    """a 20-kbp genome with a planted 600-bp repeat, and a second haplotype that differs in one planted SNP; 30x reads of 100 bp from both
    strands and both haplotypes, 1 % substitutions"""
    rng = np.random.default_rng(20261020)
    g = GC._rand_seq(rng, 20000)
    g = g[:12000] + g[3000:3600] + g[12600:]
    h = g[:7000] + GC._other(g[7000]) + g[7001:]
    reads = []
    for i in range(30 * len(g) // 100):
        p = int(rng.integers(0, len(g) - 100 + 1))
        r = list((g, h)[i & 1][p:p + 100])
        for q in np.nonzero(rng.random(100) < 0.01)[0]:
            r[q] = GC._other(r[q], int(rng.integers(1, 4)))
        r = "".join(r)
        reads.append(GC.revcomp(r) if rng.random() < 0.5 else r)
    return "".join(reads)


@pytest.mark.parametrize("k", (21, 33))
def test_reads_to_gfa(ctx, tmp_path, k):
    import torch

    b = ctx.upload(reads_case(), read_len=100)
    scan = b.kmers(k, canonical=True) if k <= 32 else b.kmers128(k, canonical=True)
    values = scan["values"][scan["valid"] != 0]
    counted = ctx.count_table(torch.from_numpy(np.ascontiguousarray(values).view(np.int64)).cuda(), key_bits=2 * k)
    table = counted.filter(3)
    u = table.unitigs(k, links=True)
    assert u.n_unitigs > 4 and u.link_stats["n_links"] == u.stats["n_arcs"] - u.stats["n_linked_sides"] + 2 * u.stats["n_cycles"] > 4
    n_bytes = u.write_gfa(tmp_path / "reads.gfa")
    fasta_bytes = u.write_fasta(tmp_path / "reads.fa")
    text = (tmp_path / "reads.gfa").read_bytes()
    assert len(text) == n_bytes and fasta_bytes > 0
    lines = text.decode("ascii").split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    segs, got = {}, set()
    for line in lines[1:-1]:
        f = line.split("\t")
        if f[0] == "S":
            assert f[3] == "LN:i:%d" % len(f[2]) and f[4].startswith("KC:i:") and len(f) == 5
            segs[f[1]] = f[2]
        else:
            assert f[0] == "L" and len(f) == 6 and f[5] == "%dM" % (k - 1) and f[2] in "+-" and f[4] in "+-"
            a, b2 = LK.oriented(segs[f[1]], f[2] == "-"), LK.oriented(segs[f[3]], f[4] == "-")
            assert a[len(a) - (k - 1):] == b2[:k - 1], "every L line's overlap holds on the S strings"
            got.add(((int(f[1]) << 1) | (f[2] == "-"), (int(f[3]) << 1) | (f[4] == "-")))
    strings = [segs[str(i)] for i in range(u.n_unitigs)]
    assert len(segs) == u.n_unitigs and len(got) == u.link_stats["n_links"]
    assert got == LK.string_links(strings, k), "the link set is the string restatement"
    fasta = (tmp_path / "reads.fa").read_text().split("\n")
    assert fasta[1::2][:u.n_unitigs] == strings, "the S strings are write_fasta's sequences"
    assert [int(s.split("KC:i:")[1]) for s in fasta[0::2][:u.n_unitigs]] == [int(x) for x in u.count_sums.cpu().numpy().view(np.uint64)]
    for x in (u.batch, b, table, counted):
        x.close()
