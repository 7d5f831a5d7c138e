"""GPU tests of graph cleaning (bl_unitigs_mark / bl_table_remove_unitigs, Unitigs.mark, CountTable.remove_unitigs / clean) against the
Python model of clean_cases.py, byte for byte and word for word.  The cases are those of the host emulation (test_emu_clean.py), where
every index path ran under the sanitizers.  d_marks is longer than the call may write and the rest must keep its fill."""
import ctypes as C
import functools

import numpy as np
import pytest

import clean_cases as CC
import graph_cases as GC
import links_cases as LK
import lookup_cases as LC

pytestmark = pytest.mark.gpu
GUARD = 24
FILL8 = 0xA5


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def build(ctx, table, key_words, key_bits):
    import torch

    keys = sorted(table)
    d_keys = torch.from_numpy(LC.words(keys, key_words).view(np.int64)).cuda()
    d_counts = torch.from_numpy(np.array([table[x] for x in keys], np.uint32).view(np.int32)).cuda()
    return ctx.count_table(d_keys, d_counts, key_bits=key_bits)


def download(t):
    """the table as the model's dict"""
    keys = t.keys.cpu().numpy().view(np.uint64)
    counts = t.counts.cpu().numpy().view(np.uint32)
    if t.key_words == 2:
        keys = [(int(hi) << 64) | int(lo) for lo, hi in keys.reshape(-1, 2)]
    return dict(zip((int(x) for x in keys), (int(c) for c in counts)))


def clean_rule(r):
    from biolib_amd import capi

    rule = capi.CleanRule()
    for name, value in r.items():
        setattr(rule, name, value)
    return rule


def mark_guarded(u, r):
    """bl_unitigs_mark into a guarded buffer -> (host marks, stats, the device marks)"""
    import torch

    from biolib_amd import capi

    marks = torch.full((u.n_unitigs + GUARD,), FILL8, dtype=torch.uint8, device=u._ctx.torch_device)
    st = capi.CleanStats()
    u.mark_raw(clean_rule(r), marks, st)
    host = marks.cpu().numpy()
    assert (host[u.n_unitigs:] == FILL8).all(), "guard bytes behind the marks"
    return host[:u.n_unitigs].tolist(), st.as_dict(), marks[:u.n_unitigs].contiguous()


def removed(t, u, d_marks, table, m, marks, k, usable=False):
    """remove_unitigs: the result's keys and counts word for word, n_removed both ways, and (usable) the result as a table"""
    want = CC.remove(table, m, marks)
    h, n_removed = t.remove_unitigs_raw(u._nodes if t.n_distinct else None, d_marks if t.n_distinct else None, u.n_unitigs)
    from biolib_amd.scan import CountTable

    out = CountTable(t.ctx, h)
    lengths = [len(s) - k + 1 for s in m["strings"]]
    assert n_removed == sum(L for L, mk in zip(lengths, marks) if mk) == t.n_distinct - out.n_distinct
    assert (out.key_words, out.key_bits) == (t.key_words, t.key_bits)
    assert download(out) == want and out.n_distinct == len(want)
    got_keys = out.keys.cpu().numpy().view(np.uint64).reshape(-1)
    assert np.array_equal(got_keys, LC.words(sorted(want), t.key_words).reshape(-1)), "in order"
    if usable:
        if out.n_distinct:
            found = out.lookup(out.keys).cpu().numpy().view(np.uint32)
            assert np.array_equal(found, out.counts.cpu().numpy().view(np.uint32)), "lookup of its own keys finds all of them"
        again = out.unitigs(k, batch=False)
        assert again.n_unitigs == len(GC.model(want, k)["strings"])
    out.close()


def same(ctx, table, k, rules, tag, widths=None, usable=True):
    """every rule of `rules` on one table: the unitigs and links are made once per key width"""
    m = GC.model(table, k)
    arrays = CC.arrays_of(m, k)
    for key_words, key_bits in widths or GC.widths(k):
        t = build(ctx, table, key_words, key_bits)
        u = t.unitigs(k, batch=False, links=True)
        assert u.n_unitigs == len(m["strings"])
        for j, r in enumerate(rules):
            want, want_st = CC.mark_arrays(*arrays, r)
            marks, st, d_marks = mark_guarded(u, r)
            assert marks == want, (tag, key_words, j, "marks")
            assert st == want_st, (tag, key_words, j, st, want_st)
            removed(t, u, d_marks, table, m, marks, k, usable and j == len(rules) - 1)
        t.close()


@pytest.mark.parametrize("k", CC.KS)
def test_named_cases(ctx, k):
    for name, table in GC.cases(k):
        same(ctx, table, k, CC.rule_sets(k), (name, k))


@pytest.mark.parametrize("k", CC.CASE_KS)
def test_planted_cases(ctx, k):
    for name, table, r in CC.planted(k):
        same(ctx, table, k, (r, CC.default_rule(k)), (name, k))


@pytest.mark.parametrize("n_unitigs", (63, 64, 65, 255, 256, 257))
def test_unitig_counts_around_a_wave_and_a_workgroup(ctx, n_unitigs):
    table = CC.spur_path(n_unitigs)
    same(ctx, table, 31, (CC.rule(31, tips=3), CC.default_rule(31)), n_unitigs, widths=((1, 62), (2, 62)), usable=n_unitigs == 257)


@pytest.mark.parametrize("seed", range(2))
def test_products_beyond_64_bits(ctx, seed):
    """array sets from no table: the call reads only the arrays"""
    import torch

    from biolib_amd import capi

    for make in (CC.synthetic_tips, CC.synthetic_bubble):
        offsets, sums, link_offsets, links, r = make(seed)
        dev = ctx.torch_device
        d = [torch.from_numpy(np.array(a, np.uint64).view(np.int64)).to(dev) for a in (offsets, sums, link_offsets)]
        d_links = torch.from_numpy(np.array(links, np.uint32).reshape(-1, 2).view(np.int32)).to(dev)
        marks = torch.full((len(sums) + GUARD,), FILL8, dtype=torch.uint8, device=dev)
        st = capi.CleanStats()
        rule = clean_rule(r)
        capi.check(ctx._lib.bl_unitigs_mark(ctx._h, C.c_void_p(d[0].data_ptr()), C.c_void_p(d[1].data_ptr()), len(sums), C.c_void_p(d[2].data_ptr()),
                                            C.c_void_p(d_links.data_ptr()), len(links), C.byref(rule), C.c_void_p(marks.data_ptr()), C.byref(st)))
        want, want_st = CC.mark_arrays(offsets, sums, link_offsets, links, r)
        assert marks.cpu().numpy().tolist() == want + [FILL8] * GUARD and st.as_dict() == want_st and any(want)


# the compaction's tile is 64 * 8 keys
@pytest.mark.parametrize("n_keys", (511, 512, 513, 1023, 1024, 1025))
def test_key_counts_around_the_tile(ctx, n_keys):
    """nodes and marks made by hand (the call needs no graph): runs of 1 .. 7 keys, every second run marked, then a marked run laid
    across every seam, then every key and no key"""
    import torch

    from biolib_amd.scan import CountTable

    table = GC.path_case(n_keys)
    keys = sorted(table)
    rng = np.random.default_rng(n_keys)
    nodes, u, i = np.zeros(n_keys, GC.NODE), 0, 0
    while i < n_keys:
        step = int(rng.integers(1, 8))
        nodes["unitig"][i:i + step] = u
        i, u = i + step, u + 1
    across = [1 if any(abs(int(s) - seam) <= 3 for s in np.nonzero(nodes["unitig"] == v)[0] for seam in (512, 1024)) else 0 for v in range(u)]
    m = dict(keys=keys, nodes=nodes)
    for key_words in (1, 2):
        t = build(ctx, table, key_words, 62)
        d_nodes = torch.from_numpy(nodes.view(np.uint32).reshape(-1, 2).view(np.int32)).to(ctx.torch_device)
        for marks in ([v % 2 * 3 for v in range(u)], across, [1] * u, [0] * u):
            d_marks = torch.tensor(marks, dtype=torch.uint8, device=ctx.torch_device)
            for n_unitigs in (u, u // 2):  # (a node at or above n_unitigs keeps its key)
                h, n_removed = t.remove_unitigs_raw(d_nodes, d_marks, n_unitigs)
                out = CountTable(ctx, h)
                want = CC.remove(table, m, marks, n_unitigs)
                assert download(out) == want and n_removed == n_keys - len(want), (n_keys, key_words)
                if out.n_distinct:
                    assert np.array_equal(out.lookup(out.keys).cpu().numpy(), out.counts.cpu().numpy())
                else:
                    assert out.unitigs(31).n_unitigs == 0, "a valid empty table"
                out.close()
        t.close()


def test_reruns_are_bit_equal(ctx):
    table = CC.spur_path(257)
    t = build(ctx, table, 1, 62)
    u = t.unitigs(31, batch=False, links=True)
    first = None
    for _ in range(3):
        marks, st, d_marks = mark_guarded(u, CC.default_rule(31))
        out = t.remove_unitigs(u, d_marks)
        run = (bytes(marks), tuple(st.items()), out.keys.cpu().numpy().tobytes(), out.counts.cpu().numpy().tobytes())
        out.close()
        first = first or run
        assert run == first
    t.close()


def failed(call, code):
    import biolib_amd

    with pytest.raises(biolib_amd.BiolibError) as e:
        call()
    assert e.value.code == code and len(str(e.value).split(": ", 1)[1]) > 5, e.value
    return str(e.value)


def test_refusals(ctx):
    import torch

    import biolib_amd
    from biolib_amd import capi

    INV = capi.BL_ERR_INVALID
    t = build(ctx, CC.spur_path(5), 1, 62)
    u = t.unitigs(31, batch=False, links=True)
    marks = torch.full((u.n_unitigs + GUARD,), FILL8, dtype=torch.uint8, device=ctx.torch_device)
    lib = ctx._lib
    P = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None

    def mark(ctx_h=ctx._h, offs=u.offsets, sums=u.count_sums, nu=u.n_unitigs, lo=u.link_offsets, links=u.links, n_links=None, k=31, flags=7, reserved=0,
             d_marks=marks, no_rule=False):
        rule = clean_rule(CC.default_rule(31))
        rule.k, rule.flags, rule.reserved = k, flags, reserved
        st = capi.CleanStats()
        st.n_tips = 99
        rc = lib.bl_unitigs_mark(ctx_h, P(offs), P(sums), nu, P(lo), P(links), int(links.shape[0]) if n_links is None else n_links,
                                 None if no_rule else C.byref(rule), P(d_marks), C.byref(st))
        assert rc == capi.BL_OK or st.n_tips == 0, "the stats are zeroed on a refusal too"
        capi.check(rc)
        return st.as_dict()

    assert mark()["n_tips"] == 2
    for k in (0, 1, 2, 30, 32, 64, 65, 1 << 20):
        failed(lambda: mark(k=k), INV)
    failed(lambda: mark(ctx_h=None), INV)
    failed(lambda: mark(no_rule=True), INV)
    failed(lambda: mark(flags=8), INV)
    failed(lambda: mark(flags=1 << 31), INV)
    failed(lambda: mark(reserved=1), INV)
    failed(lambda: mark(nu=1 << 31), INV)
    for name in ("offs", "sums", "lo", "d_marks"):
        failed(lambda: mark(**{name: None}), INV)
    failed(lambda: mark(links=None, n_links=1), INV)
    marks.fill_(FILL8)
    for k in (2, 65):
        failed(lambda: mark(k=k), INV)
    assert bool((marks == FILL8).all()), "a refusal launches nothing"
    assert mark(nu=0, offs=None, sums=None, lo=None, links=None, n_links=0, d_marks=None) == dict.fromkeys(CC.STAT_NAMES, 0), "no unitigs: zero stats"

    d_marks = torch.zeros(u.n_unitigs, dtype=torch.uint8, device=ctx.torch_device)

    def remove(ctx_h=ctx._h, table=t, nodes=u._nodes, d_marks=d_marks, no_out=False):
        h, nr = C.c_void_p(77), C.c_uint64(99)
        rc = lib.bl_table_remove_unitigs(ctx_h, table._h if table is not None else None, P(nodes), P(d_marks), u.n_unitigs, None if no_out else C.byref(h), C.byref(nr))
        assert rc == capi.BL_OK or (nr.value == 0 and (no_out or not h.value)), "*out and *n_removed are cleared on a refusal"
        capi.check(rc)
        lib.bl_table_destroy(h)

    remove()
    failed(lambda: remove(ctx_h=None), INV)
    failed(lambda: remove(table=None), INV)
    failed(lambda: remove(no_out=True), INV)
    failed(lambda: remove(nodes=None), INV)
    failed(lambda: remove(d_marks=None), INV)
    other = biolib_amd.Context(0)
    foreign = build(other, CC.spur_path(5), 1, 62)
    failed(lambda: remove(table=foreign), INV)
    foreign.close()
    other.close()

    with pytest.raises(ValueError):
        t.unitigs(31, links=True, once=True).mark(tips=5)
    with pytest.raises(ValueError):
        t.unitigs(31).mark(tips=5)
    with pytest.raises(ValueError):
        t.remove_unitigs(t.unitigs(31, batch=False), d_marks)
    t.close()


def test_empty_table(ctx):
    import torch

    t = ctx.count_table(torch.zeros(0, dtype=torch.int64, device="cuda"), key_bits=62)
    u = t.unitigs(31, batch=False, links=True)
    marks, st = u.mark(tips=5, isolated=5, bubbles=5)
    assert marks.numel() == 0 and st == dict.fromkeys(CC.STAT_NAMES, 0)
    out = t.remove_unitigs(u, marks)
    assert out.n_distinct == 0 and out.unitigs(31).n_unitigs == 0
    cleaned, history = t.clean(31)
    assert cleaned.n_distinct == 0 and history == [dict.fromkeys(CC.STAT_NAMES, 0)]
    for x in (cleaned, out, t):
        x.close()


def test_methods_and_defaults(ctx):
    k = 31
    cases = {name: table for name, table, _ in CC.planted(k)}
    table = cases["tip_then_bubble_then_island"]
    t = build(ctx, table, 1, 62)
    u = t.unitigs(k, links=True)
    assert u.nodes is None, "the defaults are unchanged"
    marks, st = u.mark()
    assert not bool(marks.any()) and st["n_unitigs"] == u.n_unitigs, "every rule is off by default"
    marks, st = u.mark(tips=2 * k, isolated=2 * k, isolated_mean=2**32 - 1, bubbles=2 * k)
    want, want_st, m = CC.mark(table, k, CC.default_rule(k))
    assert marks.cpu().tolist() == want and st == want_st
    assert download(t.remove_unitigs(u, marks)) == CC.remove(table, m, want)
    assert download(t.remove_unitigs(t.unitigs(k, nodes=True), marks)) == CC.remove(table, m, want), "nodes=True serves as well"
    for kw in (dict(), dict(max_rounds=1), dict(tips=3, bubbles=False), dict(isolated=False, bubble_diff=1)):
        cleaned, history = t.clean(k, **kw)
        r = CC.rule(k, tips=kw.get("tips", 2 * k), isolated=None if kw.get("isolated") is False else 2 * k, isolated_mean=2**32 - 1,
                    bubbles=None if kw.get("bubbles") is False else 2 * k, bubble_diff=kw.get("bubble_diff", 0))
        want_table, want_history = CC.clean(table, k, r, kw.get("max_rounds", 8))
        assert download(cleaned) == want_table and history == want_history, kw
        cleaned.close()
    assert t.n_distinct == len(table), "the input stays"
    t.close()


def test_remove_unitigs_takes_only_this_tables_unitigs(ctx):
    """what the library cannot check, the method does: the kernels read one node per key of the table, so the nodes of another table's
    unitigs (fewer than this one's keys) and marks that are not on the device are refused before anything is launched"""
    import torch

    t, small = build(ctx, CC.spur_path(9), 1, 62), build(ctx, CC.spur_path(5), 1, 62)
    u, u_small = t.unitigs(31, batch=False, links=True), small.unitigs(31, batch=False, links=True)
    assert small.n_distinct < t.n_distinct
    for other in (u_small, small.unitigs(31, nodes=True)):
        with pytest.raises(ValueError, match="another table"):
            t.remove_unitigs(other, torch.zeros(other.n_unitigs, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="another table"):
        small.remove_unitigs(u, torch.zeros(u.n_unitigs, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="device"):
        t.remove_unitigs(u, torch.zeros(u.n_unitigs, dtype=torch.uint8))
    out = t.remove_unitigs(u, torch.zeros(u.n_unitigs, dtype=torch.uint8, device="cuda"))
    assert out.n_distinct == t.n_distinct
    for x in (out, small, t):
        x.close()


def test_clean_closes_its_tables_when_a_round_raises(ctx, monkeypatch):
    """the table of the rounds before belongs to nobody once a later round raises: clean closes it, and never the caller's"""
    from biolib_amd.scan import CountTable, Unitigs

    k = 31
    rng = np.random.default_rng(9)
    a, b = GC._rand_seq(rng, 3 * k), GC._rand_seq(rng, 3 * k)
    first = a + "A" + b
    table = CC.counted([(first, 30), (a + "C" + b, 12), (CC._spur(first, 3 * k - 5, k, 2, rng, by=2), 2)], k)
    assert len(CC.clean(table, k)[1]) >= 3, "a tip on a bubble's branch: three rounds"
    t = build(ctx, table, 1, 62)
    made, calls, mark = [], [], Unitigs.mark
    remove = CountTable.remove_unitigs

    def remove_and_note(self, unitigs, marks):
        made.append(remove(self, unitigs, marks))
        return made[-1]

    def mark_twice(self, **kw):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("the third round fails")
        return mark(self, **kw)

    monkeypatch.setattr(CountTable, "remove_unitigs", remove_and_note)
    monkeypatch.setattr(Unitigs, "mark", mark_twice)
    with pytest.raises(RuntimeError, match="third round"):
        t.clean(k)
    assert len(made) == 2 and all(x._h is None for x in made), "both tables of the rounds before are closed"
    assert t._h is not None and t.n_distinct == len(table), "the caller's table stays open"
    monkeypatch.undo()
    cleaned, history = t.clean(k)
    assert download(cleaned) == CC.clean(table, k)[0]
    for x in (cleaned, t):
        x.close()


@functools.lru_cache(maxsize=None)
def reads_case():
    """a 20-kbp genome with a planted 600-bp repeat, and a second haplotype with a SNP every 2,000 bases; 20x reads of 100 bp from both
    strands and both haplotypes, 1 % substitutions"""
    rng = np.random.default_rng(20261021)
    g = GC._rand_seq(rng, 20000)
    g = g[:12000] + g[3000:3600] + g[12600:]
    h = list(g)
    for p in range(1000, len(g), 2000):
        h[p] = GC._other(h[p])
    h = "".join(h)
    reads = []
    for i in range(20 * len(g) // 100):
        p = int(rng.integers(0, len(g) - 100 + 1))
        r = list((g, h)[i & 1][p:p + 100])
        for q in np.nonzero(rng.random(100) < 0.01)[0]:
            r[q] = GC._other(r[q], int(rng.integers(1, 4)))
        r = "".join(r)
        reads.append(GC.revcomp(r) if rng.random() < 0.5 else r)
    return "".join(reads)


@pytest.mark.parametrize("k", (21, 33))
def test_reads_to_clean_gfa(ctx, tmp_path, k):
    import torch

    b = ctx.upload(reads_case(), read_len=100)
    scan = b.kmers(k, canonical=True) if k <= 32 else b.kmers128(k, canonical=True)
    values = scan["values"][scan["valid"] != 0]
    counted = ctx.count_table(torch.from_numpy(np.ascontiguousarray(values).view(np.int64)).cuda(), key_bits=2 * k)
    solid = counted.filter(2)
    cleaned, history = solid.clean(k)
    want_table, want_history = CC.clean(download(solid), k)
    assert history == want_history, "every round's stats are the model's"
    assert download(cleaned) == want_table, "the cleaned table is the model's, keys and counts"
    print("rounds:", history)
    u = cleaned.unitigs(k, links=True)
    n_bytes = u.write_gfa(tmp_path / "clean.gfa")
    text = (tmp_path / "clean.gfa").read_bytes()
    assert len(text) == n_bytes
    lines = text.decode("ascii").split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    segs, n_l = {}, 0
    for line in lines[1:-1]:
        f = line.split("\t")
        if f[0] == "S":
            assert f[3] == "LN:i:%d" % len(f[2]) and f[4].startswith("KC:i:") and len(f) == 5
            segs[f[1]] = f[2]
        else:
            assert f[0] == "L" and len(f) == 6 and f[5] == "%dM" % (k - 1) and f[2] in "+-" and f[4] in "+-"
            a, b2 = LK.oriented(segs[f[1]], f[2] == "-"), LK.oriented(segs[f[3]], f[4] == "-")
            assert a[len(a) - (k - 1):] == b2[:k - 1], "every L line's overlap holds on the S strings"
            n_l += 1
    assert len(segs) == u.n_unitigs and n_l == u.link_stats["n_links"]
    assert GC.keys_of(segs.values(), k) == set(want_table), "the k-mers of the S lines are the cleaned keys"
    for x in (u.batch, b, cleaned, solid, counted):
        x.close()
