"""GPU tests of the table graph (bl_table_adjacency / bl_table_unitigs, CountTable.adjacency / unitigs) against the Python model of
graph_cases.py, byte for byte and word for word: mask, links, nodes, offsets, strings, sums, statistics.  The cases are those of the host
emulation (test_emu_graph.py), where every index path ran under the sanitizers.  Every output buffer is longer than the call may write
and the rest must keep its fill."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import graph_cases as GC
import lookup_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@functools.lru_cache(maxsize=None)
def model_of_path(n_keys):
    return GC.model(GC.path_case(n_keys), 31)


def run_raw(ctx, t, k, batch=True, labels=True):
    """both calls through the raw bindings into guarded buffers -> dict of host arrays (and the Batch)"""
    import torch

    from biolib_amd import capi
    from biolib_amd.scan import Batch

    n, dev = t.n_distinct, ctx.torch_device
    mask = torch.full((n + GUARD,), FILL8, dtype=torch.uint8, device=dev)
    links = torch.full((2 * n + GUARD,), FILL32, dtype=torch.int32, device=dev)
    st = capi.GraphStats()
    t.adjacency_raw(k, mask, links, st)
    out = dict(adj_stats=st.as_dict())
    mask, links = mask.cpu().numpy(), links.cpu().numpy().view(np.uint32)
    assert (mask[n:] == FILL8).all() and (links[2 * n:] == FILL32).all(), "guard bytes behind mask and links"
    out.update(mask=mask[:n], links=links[:2 * n])
    offsets = torch.full((n + 1 + GUARD,), FILL64, dtype=torch.int64, device=dev) if labels else None
    sums = torch.full((n + GUARD,), FILL64, dtype=torch.int64, device=dev) if labels else None
    nodes = torch.full((n + GUARD, 2), FILL32, dtype=torch.int32, device=dev) if labels else None
    st = capi.GraphStats()
    h, n_unitigs, n_bases = t.unitigs_raw(k, batch, offsets, sums, nodes, st)
    out.update(stats=st.as_dict(), n_unitigs=n_unitigs, n_bases=n_bases)
    if labels:
        offsets, sums, nodes = offsets.cpu().numpy(), sums.cpu().numpy(), nodes.cpu().numpy().view(np.uint32)
        assert (offsets[n_unitigs + 1:] == FILL64).all() and (sums[n_unitigs:] == FILL64).all() and (nodes[n:] == FILL32).all(), "guard words"
        out.update(offsets=offsets[:n_unitigs + 1].view(np.uint64), sums=sums[:n_unitigs].view(np.uint64), nodes=nodes[:n].copy().view(GC.NODE).reshape(-1))
    if batch:
        b = Batch(ctx, h)
        assert (b.n_seqs, b.n_bases) == (n_unitigs, n_bases)
        out.update(batch=b, bases=b.download() if n_bases else np.zeros(0, np.uint8))
    return out


def same(got, m, tag):
    assert np.array_equal(got["mask"], m["mask"]), (tag, "mask")
    assert np.array_equal(got["links"], m["links"]), (tag, "links")
    assert got["adj_stats"] == {**{s: 0 for s in GC.STAT_NAMES}, **{s: m["stats"][s] for s in GC.ADJ_STATS}}, (tag, got["adj_stats"])
    assert got["stats"] == m["stats"], (tag, got["stats"], m["stats"])
    assert (got["n_unitigs"], got["n_bases"]) == (len(m["strings"]), len(m["bases"])), tag
    if "nodes" in got:
        assert np.array_equal(got["nodes"], m["nodes"]), (tag, "nodes")
        assert np.array_equal(got["offsets"], m["offsets"]), (tag, "offsets")
        assert np.array_equal(got["sums"], m["sums"]), (tag, "sums")
    if "bases" in got:
        assert got["bases"].tobytes() == m["bases"].tobytes(), (tag, "strings")


@pytest.mark.parametrize("k", GC.KS)
def test_named_cases(ctx, k):
    for name, table in GC.cases(k):
        m = GC.model(table, k)
        for key_words, key_bits in GC.widths(k):
            for option in GC.OPTIONS:
                t = build(ctx, table, key_words, key_bits, option)
                got = run_raw(ctx, t, k)
                same(got, m, (name, k, key_words, option))
                got["batch"].close()
                t.close()


@pytest.mark.parametrize("n_keys", GC.PATH_LENGTHS + (GC.LONG_PATH,))
def test_path_lengths(ctx, n_keys):
    """the rounds of the doubling: chains of 2^r - 1, 2^r and 2^r + 1 keys, and one of 70,000 (274 workgroups of keys)"""
    m = model_of_path(n_keys)
    assert m["stats"]["longest_unitig"] == n_keys or n_keys == GC.LONG_PATH and m["stats"]["longest_unitig"] > n_keys // 2
    for key_words in ((1, 2) if n_keys != GC.LONG_PATH else (1,)):
        t = build(ctx, GC.path_case(n_keys), key_words, 62)
        got = run_raw(ctx, t, 31)
        same(got, m, (n_keys, key_words))
        got["batch"].close()
        t.close()


def test_sizes_around_workgroups_and_waves(ctx):
    """every kernel is one thread per key, per side or per state, 256 to a workgroup: n and 2n on both sides of 64, 256 and 512"""
    threads = core_constants()["GTPB"]
    assert threads == 256
    for n_keys in (31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513):
        m = model_of_path(n_keys)
        t = build(ctx, GC.path_case(n_keys), 2, 62)
        got = run_raw(ctx, t, 31)
        same(got, m, n_keys)
        got["batch"].close()
        t.close()


def core_constants():
    import scale_cases as SC

    return SC.constants("bl_graph_core.hpp")


def test_no_grid_is_capped():
    """the sizes past every grid cap of the unit: it has none.  Every launch is ceil(threads / GTPB) workgroups; the 70,000-key path of
    test_path_lengths runs 274 workgroups of keys and 547 of states.  A cap added later must bring its own size here."""
    names = set(core_constants())
    assert "GTPB" in names and not any("GRID" in name or "MAX_BLOCKS" in name for name in names), names
    with open(os.path.join(ROOT, "biolib_amd", "csrc", "bl_graph.hip")) as f:
        text = f.read()
    launches = re.findall(r"hipLaunchKernelGGL\((\w+)(?:<W>)?, dim3\(([^)]*\))\)", text)
    assert len(launches) == text.count("hipLaunchKernelGGL(") >= 11 and all(grid.startswith("blocks_for(") for _, grid in launches), launches


def test_reruns_are_bit_equal(ctx):
    k = 15
    table = dict(GC.cases(k))["two_letter_repeats"]
    t = build(ctx, table, 1, 30)
    first = run_raw(ctx, t, k)
    for _ in range(3):
        again = run_raw(ctx, t, k)
        for name in ("mask", "links", "nodes", "offsets", "sums", "bases"):
            assert first[name].tobytes() == again[name].tobytes(), name
        assert first["stats"] == again["stats"]
        again["batch"].close()
    first["batch"].close()
    t.close()


def test_labels_only_batch_only_and_the_methods(ctx):
    import torch

    k = 31
    table = dict(GC.cases(k))["snp_bubble"]
    m = GC.model(table, k)
    t = build(ctx, table, 1, 62)
    got = run_raw(ctx, t, k, batch=False)
    assert "bases" not in got
    same(got, m, "labels only")
    got = run_raw(ctx, t, k, labels=False)
    assert "nodes" not in got
    same(got, m, "batch only")
    got["batch"].close()
    # the methods
    mask, links, stats = t.adjacency(k, links=True)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), m["mask"])
    assert np.array_equal(links.cpu().numpy().view(np.uint32).reshape(-1), m["links"]) and stats == {s: m["stats"][s] for s in GC.ADJ_STATS}
    assert t.adjacency(k)[1] is None
    u = t.unitigs(k, nodes=True)
    assert u.stats == m["stats"] and (u.n_unitigs, u.n_bases) == (len(m["strings"]), len(m["bases"]))
    assert np.array_equal(u.offsets.cpu().numpy().view(np.uint64), m["offsets"]) and np.array_equal(u.count_sums.cpu().numpy().view(np.uint64), m["sums"])
    assert np.array_equal(u.nodes.cpu().numpy().view(np.uint32).view(GC.NODE).reshape(-1), m["nodes"])
    assert u.batch.download().tobytes() == m["bases"].tobytes() and np.array_equal(u.batch.offsets, m["offsets"])
    assert u.batch.read_len == 0, "ragged unitigs are never a fixed-length batch"
    assert t.unitigs(k).nodes is None and t.unitigs(k, batch=False).batch is None
    # unitigs that are all equally long are a fixed-length batch, as select's rule has it
    iso = GC.table_of(GC.keys_of([GC._rand_seq(np.random.default_rng(s), k) for s in range(9)], k))
    t2 = build(ctx, iso, 1, 62)
    u2 = t2.unitigs(k)
    assert u2.n_unitigs == 9 and u2.batch.read_len == k and u2.batch.download().tobytes() == GC.model(iso, k)["bases"].tobytes()
    for x in (t, t2):
        x.close()


def test_empty_table(ctx):
    import torch

    t = ctx.count_table(torch.zeros(0, dtype=torch.int64, device="cuda"), key_bits=62)
    mask, links, stats = t.adjacency(31, links=True)
    assert mask.numel() == 0 and links.numel() == 0 and stats == dict.fromkeys(GC.ADJ_STATS, 0)
    u = t.unitigs(31, nodes=True)
    assert (u.n_unitigs, u.n_bases, u.batch.n_seqs, u.batch.n_bases) == (0, 0, 0, 0) and u.stats == dict.fromkeys(GC.STAT_NAMES, 0)
    assert u.offsets.cpu().tolist() == [0] and u.count_sums.numel() == 0
    t.close()


def refused(call):
    import biolib_amd

    with pytest.raises(biolib_amd.BiolibError) as e:
        call()
    assert e.value.code == biolib_amd.capi.BL_ERR_INVALID and len(str(e.value).split(": ", 1)[1]) > 5, e.value
    return str(e.value)


def test_refusals(ctx):
    import biolib_amd

    t1 = build(ctx, GC.path_case(5), 1, 62)
    t2 = build(ctx, GC.path_case(5), 2, 128)
    narrow = build(ctx, {3: 1}, 1, 40)
    for t in (t1, t2):
        for k in (0, 2, 30, 32, 64, 65, 1 << 20):
            refused(lambda: t.adjacency(k))
            refused(lambda: t.unitigs(k))
    refused(lambda: narrow.unitigs(21))                      # 2k above key_bits
    refused(lambda: narrow.adjacency(21))
    one64 = build(ctx, {3: 1}, 1, 64)
    refused(lambda: one64.unitigs(33))                       # one-word keys, k > 31
    refused(lambda: one64.adjacency(33))
    other = biolib_amd.Context(0)
    try:
        foreign = build(other, GC.path_case(5), 1, 62)
        st = biolib_amd.capi.GraphStats()
        mask = ctx.empty_u8(64)
        refused(lambda: biolib_amd.capi.check(ctx._lib.bl_table_adjacency(ctx._h, foreign._h, 31, C.c_void_p(mask.data_ptr()), None, C.byref(st))))
        refused(lambda: biolib_amd.capi.check(ctx._lib.bl_table_unitigs(ctx._h, foreign._h, 31, None, None, None, None, None, None, None)))
        foreign.close()
    finally:
        other.close()
    refused(lambda: biolib_amd.capi.check(ctx._lib.bl_table_adjacency(ctx._h, t1._h, 31, None, None, None)))  # d_mask NULL
    refused(lambda: biolib_amd.capi.check(ctx._lib.bl_table_adjacency(None, t1._h, 31, None, None, None)))
    # not a table of canonical k-mers of this k: the first bad slot is named
    keys = sorted(GC.path_case(5))
    big = GC.rc(keys[2], 31)
    bad = build(ctx, {**GC.path_case(5), big: 1}, 1, 62)
    slot = sorted(keys + [big]).index(big)
    assert f"slot {slot} " in refused(lambda: bad.unitigs(31)) and f"slot {slot} " in refused(lambda: bad.adjacency(31))
    high = build(ctx, {3: 1, 5: 2, (1 << 30) | 1: 2, (1 << 31) | 1: 2}, 1, 62)
    assert "slot 2 " in refused(lambda: high.unitigs(15)) and "slot 2 " in refused(lambda: high.adjacency(15))
    for t in (t1, t2, narrow, one64, bad, high):
        t.close()
    # (2^31 keys or more: the same function refuses in front of everything; tests/test_emu_graph.py runs it with the count alone)


@functools.lru_cache(maxsize=None)
def reads_case():
    """a 20-kbp genome with a planted 600-bp repeat, 30x reads of 100 bp from both strands, 1 % substitutions"""
    rng = np.random.default_rng(20261019)
    g = GC._rand_seq(rng, 20000)
    g = g[:12000] + g[3000:3600] + g[12600:]
    reads = []
    for _ in range(30 * len(g) // 100):
        p = int(rng.integers(0, len(g) - 100 + 1))
        r = list(g[p:p + 100])
        for q in np.nonzero(rng.random(100) < 0.01)[0]:
            r[q] = GC._other(r[q], int(rng.integers(1, 4)))
        r = "".join(r)
        reads.append(GC.revcomp(r) if rng.random() < 0.5 else r)
    return "".join(reads)


@pytest.mark.parametrize("k", (21, 33))
def test_reads_to_unitigs(ctx, k):
    import torch

    b = ctx.upload(reads_case(), read_len=100)
    scan = b.kmers(k, canonical=True) if k <= 32 else b.kmers128(k, canonical=True)
    values = scan["values"][scan["valid"] != 0]
    kw = 1 if k <= 32 else 2
    counted = ctx.count_table(torch.from_numpy(np.ascontiguousarray(values).view(np.int64)).cuda(), key_bits=2 * k)
    table = counted.filter(3)
    assert 15000 < table.n_distinct < counted.n_distinct
    u = table.unitigs(k, nodes=True)
    # the canonical k-mers of the unitig batch are the table's keys, each exactly once
    again = u.batch.kmers(k, canonical=True) if k <= 32 else u.batch.kmers128(k, canonical=True)
    got = again["values"][again["valid"] != 0]
    host_keys = table.keys.cpu().numpy().view(np.uint64)
    if kw == 1:
        assert np.array_equal(np.sort(got.reshape(-1)), host_keys)
    else:
        order = np.lexsort((got[:, 0], got[:, 1]))
        assert np.array_equal(got[order], host_keys.reshape(-1, 2))
    counts, valid, result = u.batch.kmer_counts(table, k, canonical=True, valid=True)
    assert result["count"] == table.n_distinct == result["found"]
    assert int((counts[valid != 0] == 0).sum()) == 0, "no k-mer of a unitig is missing from the table"
    # and the unitigs are the model's
    words = host_keys if kw == 1 else host_keys.reshape(-1, 2)
    ints = [int(x) for x in words] if kw == 1 else [(int(hi) << 64) | int(lo) for lo, hi in words.tolist()]
    m = GC.model(dict(zip(ints, (int(c) for c in table.counts.cpu().numpy().view(np.uint32)))), k)
    assert u.stats == m["stats"] and u.stats["n_unitigs"] > 1
    assert u.batch.download().tobytes() == m["bases"].tobytes()
    assert np.array_equal(u.offsets.cpu().numpy().view(np.uint64), m["offsets"]) and np.array_equal(u.count_sums.cpu().numpy().view(np.uint64), m["sums"])
    assert np.array_equal(u.nodes.cpu().numpy().view(np.uint32).view(GC.NODE).reshape(-1), m["nodes"])
    for x in (u.batch, b, table, counted):
        x.close()
