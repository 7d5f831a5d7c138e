"""One scan per kernel the launchers of bl_kernels.hip can choose: the table, its inputs and what the oracle says about them.  TEST INFRASTRUCTURE
shared by test_kernel_cases.py (CPU: the table against the library's own list of names, the inputs through the emulation) and
test_gpu_kernel_census.py / test_gpu_read_lengths.py / test_gpu_capacity_guard.py (the kernels).  Nothing here runs code under test.

launch_count_frl, launch_count_mode and launch_emit_mode record a name for every kernel they launch (bl_ctx_last_scan_kernels) and the
library lists every name it can record (bl_scan_kernel_names).  ROWS holds, for every such name, the arguments of one scan that selects it:
    names            the kernels the scan must record, in launch order: pass 1, its second run where pass 1 decides on murmur64_top, pass 2
    entry            minimizers | hash_sample | super_kmers | records128 | syncmers
    unit, w          the hashed unit and the window: (unit, w) of a minimizer scan, m = unit and k = unit + w - 1 of a super-k-mer scan,
                     s = unit and k = unit + w - 1 of a syncmer scan
    offsets          syncmer offsets, else None
    canonical, exact, position_tiled    the strand flag and the two context switches (bl_ctx_set_exact_windows, option "position_tiled")
    read_len         0: the position-tiled inputs (a), (b), (b'); L: reads of L bases, input (c)

Inputs.  All borders come from tie_plant.plan_pos / plan_frl (pinned against the emulation's emu_plan by test_tie_adversaries.py).  A position tile
owns 4 * (1024 - 16 * ceil(w / 16)) positions, so about 13 k bases are three full tiles and a partial one:
    (a)  contig    one contig, upper and lower case, with a repeat island (ACGTTACA..., a homopolymer in its middle) laid across the border of
                   tiles 1 | 2: equal keys in every window there, so the leftmost-minimum rule and the exact fallback work on a tile edge
    (b)  ragged    reads of 1..700 bases; sequence starts planted at a tile border - 1, + 0, + 1 and at a wave border (stride / 4 into a tile)
                   - 1, + 0, + 1; reads shorter than unit, of exactly unit, of unit + w - 1 (one window) and one base more
    (b') ragged_n  the same reads without the planted starts, an N at each of the six places instead
    (c)  reads     two full tiles plus three reads of one length, some N's, one read of repeats
and one sub-range per row whose first base is no multiple of 16 (read-tiled rows: a multiple of the read length) and whose end lies inside
a tile.  A range reports the windows (k-mers) that START in it.  Super-k-mers: the oracle's groups that overlap the range, each cut to it
(range_groups).  Minimizers: the occurrences whose first electing window starts in the range (range_minimizers), an occurrence being one
group of the oracle; test_kernel_cases.py holds that view against oracle_lib.minimizers on every row."""
import collections
import functools

import numpy as np

import oracle_lib as O
import tie_plant as P

SEED = 0x0CE115
THRESHOLD = 1 << 62  # hash_sample: a quarter of the k-mers
Row = collections.namedtuple("Row", "names entry unit w offsets canonical exact position_tiled read_len")

MIN_FIELDS = ("values", "positions", "hashes")
SK_FIELDS = ("minimizers", "first_pos", "mm_pos", "sizes", "hashes")
FIELDS = {"minimizers": MIN_FIELDS, "hash_sample": MIN_FIELDS, "super_kmers": SK_FIELDS, "syncmers": ("positions",), "records128": ("records", "hashes")}
MODE = {"minimizers": P.MODE_MINIMIZER, "hash_sample": P.MODE_MINIMIZER, "super_kmers": P.MODE_SUPERKMER, "records128": P.MODE_SUPERKMER,
        "syncmers": P.MODE_SYNCMER}


# ----------------------------------------------------------------------------- the table

def frl_length(ns):
    """the shortest read length, 150 aside, that gives canonical (31, 11) minimizers `ns` units per lane on at least four lanes per read"""
    for L in range(41, 400):
        g = P.plan_frl(P.MODE_MINIMIZER, L * 1000, L, 31, 11, 1)
        if g and L != 150 and g["ns"] == ns and g["lpr"] >= 4 and (g["nu"] + g["lpr"] - 1) // g["lpr"] == ns:
            return L
    raise AssertionError(ns)


def _row(names, entry, unit, w, canonical, offsets=None, exact=False, position_tiled=False, read_len=0):
    return Row(tuple(names), entry, unit, w, offsets, int(canonical), exact, position_tiled, read_len)


def _rows():
    mm, sk, sy = "minimizers", "super_kmers", "syncmers"
    rows = [
        # read-tiled: the L = 150 kernel, on murmur64_top with its second run and exact
        _row(("frl<MM,W=11,NS=15,U=31,L=150,approx>", "frl_redo<MM,W=11,NS=15,U=31,L=150>", "emit<MM,C3>"), mm, 31, 11, 1, read_len=150),
        _row(("frl<MM,W=11,NS=15,U=31,L=150>", "emit<MM,C3>"), mm, 31, 11, 1, exact=True, read_len=150),
    ]
    for ns in (14, 15, 16):  # ... the read geometry from the arguments, 14 / 15 / 16 units per lane
        L = frl_length(ns)
        rows.append(_row((f"frl<MM,W=11,NS={ns},U=31,approx>", f"frl_redo<MM,W=11,NS={ns},U=31>", "emit<MM,C3>"), mm, 31, 11, 1, read_len=L))
        rows.append(_row((f"frl<MM,W=11,NS={ns},U=31>", "emit<MM,C3>"), mm, 31, 11, 1, exact=True, read_len=L))
    for unit, w, c in ((21, 5, 1), (25, 10, 0), (23, 11, 1), (21, 19, 1)):  # ... the generic widths
        rows.append(_row((f"frl<MM,W={w}>", "emit<MM>"), mm, unit, w, c, read_len=100))
    rows.append(_row(("frl<SK,W=17>", "emit<SK>"), sk, 25, 17, 1, read_len=100))
    # position-tiled: the specialised shapes, each with its exact-windows twin where it has one
    rows += [
        _row(("count<MM,W=11,U=31,C=1,approx>", "redo<MM,W=11,U=31,C=1>", "emit<MM>"), mm, 31, 11, 1),
        _row(("count<MM,W=11,U=31,C=1>", "emit<MM>"), mm, 31, 11, 1, exact=True),
        _row(("count<SK,W=17,U=15,C=1>", "emit<SK>"), sk, 15, 17, 1),
        _row(("count<SY,W=21,U=11,C=1,closed>", "redo<SY,W=21,U=11,C=1>", "emit<SY>"), sy, 11, 21, 1, offsets=(0, 20)),
        _row(("count<SY,W=21,U=11,C=1,deferred>", "redo<SY,W=21,U=11,C=1>", "emit<SY>"), sy, 11, 21, 1, offsets=(3, 9)),
        _row(("count<SY,W=21,U=11,C=1,deferred>", "redo<SY,W=21,U=11,C=1>", "emit<SY>"), sy, 11, 21, 1, offsets=(20, 0), exact=True),
        _row(("count<SY,closed,W<=17>", "emit<SY>"), sy, 12, 14, 1, offsets=(0, 13)),
        _row(("count<SY,closed,W<=32>", "emit<SY>"), sy, 8, 23, 0, offsets=(22, 0)),
    ]
    for w in range(2, 33):  # a kernel per width
        rows.append(_row((f"count<MM,W={w}>", "emit<MM>"), mm, 13 + (7 * w) % 19, w, w & 1))
        rows.append(_row((f"count<SK,W={w}>", "emit<SK>"), sk, 12 + (5 * w) % 19, w, (w >> 1) & 1))
    rows += [
        _row(("count<MM,W=1>", "emit<MM>"), mm, 21, 1, 1),
        _row(("count<MM,W=1>", "emit<MM>"), "hash_sample", 27, 1, 0),
        _row(("count<SK,W=1>", "emit<SK>"), sk, 19, 1, 1),
        _row(("count<SY,W=1>", "emit<SY>"), sy, 15, 1, 1, offsets=(0, 0), exact=True),
        _row(("count<SY,W=11>", "emit<SY>"), sy, 15, 11, 1, offsets=(2, 7)),
        _row(("count<SY,W=17>", "emit<SY>"), sy, 11, 17, 0, offsets=(0, 8)),
        _row(("count<SY,W=21>", "emit<SY>"), sy, 11, 21, 0, offsets=(5, 20)),
        _row(("count<SY,W<=16>", "emit<SY>"), sy, 20, 8, 1, offsets=(1, 6)),
        _row(("count<SY,W<=32>", "emit<SY>"), sy, 9, 19, 1, offsets=(0, 9)),
        _row(("count<SY,W<=32>", "emit<SY>"), sy, 7, 26, 0, offsets=(0, 25), exact=True),  # closed offsets under exact windows: the argmin kernels
        _row(("count<MM,W>32>", "emit<MM>"), mm, 21, 48, 1),
        _row(("count<SK,W>32>", "emit<SK>"), sk, 25, 64, 0),
        _row(("count<SK,W=31>", "emit<SK,wide>"), "records128", 21, 31, 1),  # k = 51: the 32-byte record
        # fixed-length reads kept on the position-tiled kernels by the context's switch
        _row(("count<MM,W=19>", "emit<MM>"), mm, 21, 19, 1, position_tiled=True, read_len=100),
    ]
    for r in rows:
        assert not (r.entry == mm and (r.unit, r.w, r.canonical) == (31, 11, 1)) or "U=31" in r.names[0]
        assert not (r.entry == sk and (r.unit, r.w, r.canonical) == (15, 17, 1)) or "U=15" in r.names[0]
    return rows


ROWS = _rows()


def row_id(r):
    return "-".join([r.names[0], r.entry, f"u{r.unit}", f"c{r.canonical}"] + ([f"o{r.offsets[0]}.{r.offsets[1]}"] if r.offsets else []) +
                    (["exact"] if r.exact else []) + (["pos"] if r.position_tiled else []) + ([f"L{r.read_len}"] if r.read_len else []))


def family(r):
    """what a test item of the census runs together"""
    head = r.names[0]
    if r.read_len:
        return "read_tiled"
    if "U=" in head or "closed" in head:
        return "specialised"
    if head.startswith("count<SY") or "W=1>" in head or "W>32" in head or r.entry == "records128":
        return "other"
    lo = (r.w - 1) // 8 * 8 + 1
    return f"{'MM' if head.startswith('count<MM') else 'SK'}_w{max(lo, 2)}_{lo + 7}"


FAMILIES = sorted({family(r) for r in ROWS})


# ----------------------------------------------------------------------------- inputs

ISLAND = b"ACGTTACA" * 16 + b"A" * 96 + b"ACGTTACA" * 16


def _mixed_case(seq):
    seq[::7] |= 0x20


@functools.lru_cache(None)
def contig(mode, w):
    """(a): (seq, offsets, read_len, plan)"""
    n = P.pos_length(w)
    g = P.plan_pos(mode, 0, n, w)
    assert g["n_tiles"] == 4
    seq = O.synth(11 + w, n)
    border = g["origin"] + 2 * g["stride"]
    at = border - len(ISLAND) // 2
    seq[at:at + len(ISLAND)] = np.frombuffer(ISLAND, np.uint8)
    _mixed_case(seq)
    return seq, np.array([0, n], np.uint64), 0, g


def planted_places(g):
    """the six places of (b) and (b'): a tile border and a wave border, each - 1, + 0, + 1"""
    tile = g["origin"] + g["stride"]
    wave = g["origin"] + 2 * g["stride"] + g["stride"] // 4
    return [tile - 1, tile, tile + 1, wave - 1, wave, wave + 1]


@functools.lru_cache(None)
def ragged(mode, unit, w, with_n):
    """(b) and (b'): (seq, offsets, read_len, plan)"""
    n = P.pos_length(w)
    g = P.plan_pos(mode, 0, n, w)
    rng = np.random.default_rng(7 * w + unit)
    lens = [x for x in (unit - 1, unit, unit + w - 1, unit + w, 1) if x >= 1] + rng.integers(1, 700, 80).tolist()
    starts = {0} | {int(x) for x in np.cumsum(lens) if x < n}
    seq = O.synth(23 + w, n)
    seq[rng.integers(0, n, 12)] = ord("N")
    _mixed_case(seq)
    places = planted_places(g)
    if with_n:
        starts -= set(places)
        seq[places] = ord("N")
    else:
        starts |= set(places)
    return seq, np.array(sorted(starts) + [n], np.uint64), 0, g


def reads_per_tile(mode, L, unit, w, canonical, position_tiled=False):
    """reads a tile takes: the read-tiled plan's, or what a position tile holds where the scan stays position-tiled"""
    g = None if position_tiled else P.plan_frl(mode, L * 1000, L, unit, w, canonical)
    return (g["reads_per_tile"], g) if g else (-(-P.plan_pos(mode, 0, 1, w)["stride"] // L), None)


@functools.lru_cache(None)
def reads(mode, L, unit, w, canonical, position_tiled=False):
    """(c): two full tiles plus three reads of L bases: (seq, offsets, read_len, plan or None)"""
    rpt, _ = reads_per_tile(mode, L, unit, w, canonical, position_tiled)
    n_reads = 2 * rpt + 3
    n = n_reads * L
    rng = np.random.default_rng(31 * L + w)
    seq = O.synth(37 + L, n)
    seq[rng.integers(0, n, 6)] = ord("N")
    r = rpt + 1  # one read of repeats, in the second tile
    seq[r * L:(r + 1) * L] = np.frombuffer((b"ACGTTACA" * (L // 8 + 1))[:L], np.uint8)
    _mixed_case(seq)
    g = None if position_tiled else P.plan_frl(mode, n, L, unit, w, canonical)
    return seq, O.fixed_offsets(n, L), L, g


def inputs(r):
    """[(label, seq, offsets, read_len)] of a row"""
    mode = MODE[r.entry]
    if r.read_len:
        seq, offs, L, g = reads(mode, r.read_len, r.unit, r.w, r.canonical, r.position_tiled)
        assert (g is not None) == (not r.position_tiled), "the row's read length must take the layout its kernel belongs to"
        return [("reads", seq, offs, L)]
    return [("contig",) + contig(mode, r.w)[:3], ("ragged",) + ragged(mode, r.unit, r.w, False)[:3], ("ragged_n",) + ragged(mode, r.unit, r.w, True)[:3]]


def sub_range(r):
    """(label, seq, offsets, read_len, first, n): first % 16 != 0 (read-tiled: a multiple of the read length), the end inside a tile"""
    mode = MODE[r.entry]
    if r.read_len:
        seq, offs, L, g = reads(mode, r.read_len, r.unit, r.w, r.canonical, r.position_tiled)
        rpt, _ = reads_per_tile(mode, L, r.unit, r.w, r.canonical, r.position_tiled)
        first, n = L, (rpt + 2) * L
        assert first + n < len(seq) and n % (rpt * L) != 0
        return "reads", seq, offs, L, first, n
    seq, offs, _, g = contig(mode, r.w)
    first, n = g["origin"] + g["stride"] + 37, g["stride"] + 555
    sub = P.plan_pos(mode, first, first + n, r.w)
    assert first % 16 and sub["n_tiles"] == 2 and (first + n - sub["origin"]) % sub["stride"] and first + n < len(seq)
    return "contig", seq, offs, 0, first, n


# ----------------------------------------------------------------------------- what the oracle says

def _end(seq, first, n):
    return len(seq) if n == 0 else min(first + n, len(seq))


def range_groups(seq, offs, k, m, canonical, first, n, seed=SEED):
    """the oracle's super-k-mer groups that hold a k-mer starting in [first, first + n), cut to that range:
    (minimizers, first_pos, mm_pos, sizes, hashes)"""
    mn, fp, mp, sz, hs = O.super_kmers(seq, offs, k, m, seed, bool(canonical))
    end = _end(seq, first, n)
    fp_i, last = fp.astype(np.int64), fp.astype(np.int64) + sz.astype(np.int64) - 1
    keep = (last >= first) & (fp_i < end)
    a, b = np.maximum(fp_i[keep], first), np.minimum(last[keep], end - 1)
    return mn[keep], a.astype(np.uint64), (mp[keep].astype(np.int64) - (a - fp_i[keep])).astype(np.uint8), (b - a + 1).astype(np.uint8), hs[keep]


def minimizers_from_groups(groups):
    mn, fp, mp, _, hs = groups
    return mn, fp + mp.astype(np.uint64), hs


def range_minimizers(seq, offs, unit, w, canonical, first, n, seed=SEED):
    """the minimizer occurrences whose FIRST electing window starts in [first, first + n): an occurrence that the window in front of the range
    elects too belongs to the range before (include/biolib_amd.h: consecutive ranges concatenate exactly).  An occurrence is a super-k-mer
    group of the oracle: the consecutive windows that elect it."""
    mn, fp, mp, _, hs = O.super_kmers(seq, offs, unit + w - 1, unit, seed, bool(canonical))
    keep = (fp >= np.uint64(first)) & (fp < np.uint64(_end(seq, first, n)))
    return minimizers_from_groups((mn[keep], fp[keep], mp[keep], None, hs[keep]))


def expected(r, seq, offs, read_len, first=0, n=0):
    """{field: array} for the row's entry point, plus count and the digest words the entry point reports"""
    c = bool(r.canonical)
    k = r.unit + r.w - 1
    whole = first == 0 and n == 0
    if r.entry in ("minimizers", "hash_sample"):
        v, p, h = O.minimizers(seq, offs, r.unit, r.w, SEED, c) if whole else range_minimizers(seq, offs, r.unit, r.w, c, first, n)
        if r.entry == "hash_sample":
            keep = h < np.uint64(THRESHOLD)
            v, p, h = v[keep], p[keep], h[keep]
        out = dict(values=v, positions=p, hashes=h, xor_value=O.xor_reduce(v), xor_hash=O.xor_reduce(h), xor_pos=O.xor_reduce(p))
    elif r.entry == "super_kmers":
        g = O.super_kmers(seq, offs, k, r.unit, SEED, c) if whole else range_groups(seq, offs, k, r.unit, c, first, n)
        out = dict(zip(SK_FIELDS, g), xor_value=O.xor_reduce(g[0]), xor_hash=O.xor_reduce(g[4]), xor_pos=O.xor_reduce(g[1] + g[2].astype(np.uint64)), aux=len(g[0]))
    elif r.entry == "records128":
        import records128_cases as R

        recs, hs = R.Expect(seq, offs, read_len, k, r.unit, c, seed=SEED).of_range(first, n)
        out = dict(records=recs, hashes=hs, xor_hash=O.xor_reduce(hs), aux=len(hs))
    else:
        _, pos = O.syncmers(seq, offs, k, r.unit, r.offsets[0], r.offsets[1], c)
        pos = pos[(pos >= np.uint64(first)) & (pos < np.uint64(_end(seq, first, n)))]
        out = dict(positions=pos, xor_pos=O.xor_reduce(pos))
    out["count"] = len(out[FIELDS[r.entry][0]])
    return out


# ----------------------------------------------------------------------------- every fixed read length

# (entry, unit, w, canonical): minimizers (31, 11) on both strands, (15, 5), (15, 10), (20, 19); super-k-mers (31, 15)
LENGTH_SHAPES = (("minimizers", 31, 11, 1), ("minimizers", 31, 11, 0), ("minimizers", 15, 5, 1), ("minimizers", 15, 10, 0), ("minimizers", 20, 19, 1),
                 ("super_kmers", 15, 17, 0))
LENGTH_BLOCKS = 8
BEYOND = 32  # lengths past the largest the read-tiled plan accepts: the position-tiled fallback


def frl_verdict(L, unit, w, ns_fixed):
    """plan_scan_frl's rules one by one (bl_scan_core.hpp), for the coverage claims of the read-length tests: 'ok', or the rule that refuses L;
    with it rpw, the cap on rpw, lpr and ns.  test_kernel_cases.py holds the verdict against tie_plant.plan_frl at every length."""
    nu = L - unit + 1
    nwin = nu - w + 1
    if nwin < 1 or w < 2:
        return dict(rule="no window")
    lpr = (nu + P.S - 1) // P.S
    if lpr > 64:
        return dict(rule="lanes")
    ns = ns_fixed or (nu + lpr - 1) // lpr
    if ns * lpr < nu or ns > P.S:
        return dict(rule="units per lane", lpr=lpr, ns=ns)
    if w - 1 > 3 * ns:
        return dict(rule="halo", lpr=lpr, ns=ns)
    cap = (P.NCHUNK * 16 - 64 - 32) // P.NWAVE // L
    rpw = min(64 // lpr, cap)
    if rpw < 1:
        return dict(rule="lds", lpr=lpr, ns=ns)
    frl_eff = (rpw * nwin) / (64.0 * ns)
    pos_eff = nwin / L * (64 * P.S - 16 * ((w + 15) // 16)) / (64.0 * P.S)
    return dict(rule="ok" if frl_eff > pos_eff else "efficiency", lpr=lpr, ns=ns, rpw=rpw, capped=cap < 64 // lpr)


def shape_verdict(shape, L):
    """the verdict of the plan the scan takes (plan_scan_frl_for: canonical (31, 11) first with the units per lane the length asks for)"""
    entry, unit, w, canonical = shape
    if entry == "minimizers" and (unit, w, canonical) == (31, 11, 1):
        v = frl_verdict(L, unit, w, 0)
        if v["rule"] == "ok" and 14 <= v["ns"] <= 16:
            return v
    return frl_verdict(L, unit, w, P.S)


@functools.lru_cache(None)
def lengths_of(shape):
    """every read length from one window (unit + w - 1) to the largest the read-tiled plan accepts, and BEYOND more"""
    entry, unit, w, canonical = shape
    mode = MODE[entry]
    lo = unit + w - 1
    top = max(L for L in range(lo, 4097) if P.plan_frl(mode, L * 1000, L, unit, w, canonical))
    return list(range(lo, top + BEYOND + 1))


def length_block(shape, block):
    Ls = lengths_of(shape)
    return Ls[block::LENGTH_BLOCKS]  # interleaved: every block meets short and long reads, and takes about the same time


def length_row(shape, L):
    entry, unit, w, canonical = shape
    return _row(("?",), entry, unit, w, canonical, read_len=L)


def length_input(shape, L):
    entry, unit, w, canonical = shape
    return reads.__wrapped__(MODE[entry], L, unit, w, canonical)


def assert_plan_coverage():
    """what the lengths of LENGTH_SHAPES reach in plan_scan_frl, from tie_plant.plan_frl and the rules above.  The planner's arithmetic meets every
    lanes-per-read count 1..64; it ACCEPTS only those at which 64 / lpr reads fill a wave well enough to beat the position-tiled layout (1..12,
    14..16, 20, 21, 30..32, 61..64 for 31-mers: the others are refused by the efficiency rule at every length, which is asserted here, so a
    planner that starts to accept one of them fails this test until the sweep's claims are looked at again)."""
    reached, accepted, ns_c3, capped, eff = set(), set(), set(), 0, {"ok": 0, "efficiency": 0}
    refused = collections.defaultdict(set)
    for shape in LENGTH_SHAPES:
        entry, unit, w, canonical = shape
        for L in lengths_of(shape):
            g, v = P.plan_frl(MODE[entry], L * 1000, L, unit, w, canonical), shape_verdict(shape, L)
            assert (g is not None) == (v["rule"] == "ok"), (shape, L, v)
            if v["rule"] in eff:
                eff[v["rule"]] += 1
            if "lpr" in v:
                reached.add(v["lpr"])
            if not g:
                refused[v.get("lpr")].add(v["rule"])
                continue
            assert (g["lpr"], g["ns"], g["rpw"]) == (v["lpr"], v["ns"], v["rpw"]), (shape, L)
            assert all(((lane * ((65536 + g["lpr"] - 1) // g["lpr"])) >> 16) == lane // g["lpr"] for lane in range(64)), g["lpr"]  # lpr_inv
            accepted.add(g["lpr"])
            capped += v["capped"]
            if (unit, w, canonical) == (31, 11, 1):
                ns_c3.add(g["ns"])
            else:
                assert g["ns"] == P.S, (shape, L)
    assert reached == set(range(1, 65)), sorted(set(range(1, 65)) - reached)
    assert {1, 64} <= accepted and all(refused[x] <= {"efficiency"} for x in reached - accepted), (sorted(accepted), dict(refused))
    assert {14, 15, 16} <= ns_c3, ns_c3
    assert capped > 0 and eff["ok"] > 0 and eff["efficiency"] > 0, (capped, eff)
    return dict(reached=len(reached), accepted=sorted(accepted), ns_c3=sorted(ns_c3), capped=capped, **eff)


# ----------------------------------------------------------------------------- comparing

DIGEST = {"minimizers": ("xor_value", "xor_hash", "xor_pos"), "hash_sample": ("xor_value", "xor_hash", "xor_pos"),
          "super_kmers": ("xor_value", "xor_hash", "xor_pos", "aux"), "records128": ("xor_hash", "aux"), "syncmers": ("xor_pos",)}


def assert_same(entry, got, want, what):
    """count, every array element for element, every digest word"""
    assert int(got["count"]) == want["count"], (what, "count", int(got["count"]), want["count"])
    for f in FIELDS[entry]:
        g, x = np.asarray(got[f]), want[f]
        assert g.shape == x.shape, (what, f, g.shape, x.shape)
        bad = np.nonzero(g.astype(x.dtype) != x)[0]
        assert len(bad) == 0, (what, f, "first differing record", int(bad[0]), "of", len(x))
    for d in DIGEST[entry]:
        assert int(got[d]) == int(want[d]), (what, d, hex(int(got[d])), hex(int(want[d])))
