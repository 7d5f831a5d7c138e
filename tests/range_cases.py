"""Range seams: every scan entry point cut at every kind of place.  TEST INFRASTRUCTURE shared by test_range_seams.py (the CPU emulation) and
test_gpu_range_seams.py (the kernels); nothing here runs code under test.

include/biolib_amd.h: "the union of the results of consecutive ranges equals the result of one scan over their union".  A cut set (c1 < c2 < ...)
of a batch of n bases stands for the consecutive ranges [0, c1), [c1, c2), ..., [c_last, n).  For every range this module says what the entry
point must report, derived from ONE whole-batch run of the oracle or of a model by a rule written out here:
    kmers, kmers128                          the slice [first, end) of the dense arrays, and the digest of that slice
    hash_sample(128), syncmers(128)          the records whose position lies in [first, end)
    minimizers, minimizers128                the occurrences whose FIRST electing window starts in [first, end): an occurrence is one super-k-mer
                                             group of the oracle (kernel_cases.range_minimizers' rule), minimizers128_model.minimizers(m, first, end)
    super_kmers                              the oracle's groups that hold a k-mer of the range, each clipped to the range: first_pos moves to the
                                             first k-mer inside, mm_pos shrinks by as much, sizes counts the k-mers inside (kernel_cases.range_groups' rule)
    super_kmer_records                       superkmer_model.pack of those clipped groups, and their hashes
    super_kmer_records128                    records128_cases.Expect.of_range

Where the cuts lie.  g is the plan of the WHOLE scan (tie_plant.plan_pos; H = 4096 positions per tile for the dense and the 128-bit scans), T =
g.origin + g.stride its first inner tile border, W = g.origin + 2 g.stride + g.stride / 4 a wave border:
    (a)  1 .. 17             every residue of `first` mod 16 and the three origins of the range's own plan: align_down16(first - 1) is negative
                             for first = 0, 0 up to first = 16, 16 from first = 17 on
    (b)  T - 17 .. T + 17    the borders of the second range's tiles move with its first base: what lies mid-tile in the whole scan lies on every
                             residue around a border there
    (c)  W - 2 .. W + 2
    (d)  ragged              each planted sequence start - 1, + 0, + 1, and the start behind every read shorter than `unit`
    (e)  ragged_n            each planted N - unit, - 1, + 0, + 1
    (f)  contig              the repeat island's first base, the middle of its homopolymer, its last base;
         planted             (tie_plant.pos_batch) every position at - 2 .. at + w + 2 of three planted windows with teeth
    (g)  n - unit - w - 1 .. n - 1   the last range holds one window, then none
    (h)  breaks              (128-bit entries: the batch with bytes >= 0x80 and sequence starts on tile borders) every sequence start - 1, + 0, + 1
Three-way cuts (c, c + d): c = p - 1, p, p + 1, p + 15, p + 16 around an anchor p (T; one planted place; the island's middle) and
d = 1, 2, w - 1, w, w + 1, 16: middle ranges shorter than a window, a lane and a tile; once per input d = g.stride.
Read-tiled batches (kernel_cases.reads): cuts at read multiples (the range stays read-tiled) and off them (it falls back to the position-tiled
kernels and the start bits), so that the halves of one scan run in different layouts."""
import collections
import functools

import numpy as np

import kernel_cases as K
import oracle_lib as O
import tie_plant as P

H = 4096  # positions per tile of the dense k-mer scan and of the 128-bit scans (bl_scan_core.hpp)
GUARD = 8  # elements behind every dense array that must stay untouched


# ----------------------------------------------------------------------------- shapes

def _pick(head, entry=None, offsets=None, read_len=0, exact=None):
    rows = [r for r in K.ROWS if r.names[0] == head and r.read_len == read_len and not r.position_tiled and entry in (None, r.entry)
            and offsets in (None, r.offsets) and exact in (None, r.exact)]
    assert len(rows) == 1, (head, entry, offsets, rows)
    return rows[0]


# one row of kernel_cases.ROWS per kernel family: the census stays the authority on which kernel a shape selects
POS_ROWS = [
    _pick("count<MM,W=11,U=31,C=1,approx>"),
    _pick("count<MM,W=11,U=31,C=1>"),
    _pick("count<SK,W=17,U=15,C=1>"),
    _pick("count<SY,W=21,U=11,C=1,closed>"),
    _pick("count<SY,W=21,U=11,C=1,deferred>", offsets=(3, 9)),
    _pick("count<MM,W=5>"),
    _pick("count<MM,W=19>"),
    _pick("count<MM,W>32>"),
    _pick("count<SK,W>32>"),
    _pick("count<MM,W=1>", entry="minimizers"),
    _pick("count<MM,W=1>", entry="hash_sample"),
]
FRL_ROWS = [
    _pick("frl<MM,W=11,NS=15,U=31,L=150,approx>", read_len=150),
    _pick("frl<MM,W=11,NS=15,U=31,L=150>", read_len=150),
    _pick("frl<MM,W=19>", read_len=100),
    _pick("frl<SK,W=17>", read_len=100),
]
assert [(r.unit, r.w) for r in POS_ROWS[7:9]] == [(21, 48), (25, 64)] and [(r.unit, r.w) for r in FRL_ROWS[2:]] == [(21, 19), (25, 17)]
KMER_SHAPES = [(k, d) for k in (1, 31, 32) for d in (False, True)]  # dense k-mers: (k, drop_last), canonical
# 128-bit entries: (entry, arguments)
SHAPES128 = [("kmers128", (33,)), ("kmers128", (64,)), ("hash_sample128", (51,)), ("minimizers128", (33, 16)), ("minimizers128", (64, 64)),
             ("minimizers128", (17, 11)), ("minimizers128", (40, 2)), ("syncmers128", (33, 11)), ("syncmers128", (64, 32)), ("records128", (51, 21)),
             ("records128", (64, 32))]
SEED128 = 0x9E3779B9  # (the stand-alone emulators hash with this seed)


def id128(shape):
    return shape[0] + "-" + "-".join(str(x) for x in shape[1])


# ----------------------------------------------------------------------------- inputs

Input = collections.namedtuple("Input", "label seq offs read_len seed plan extra")  # extra: planted windows (label 'planted'), else None


def seed_of(r):
    return 0 if r.entry == "syncmers" else K.SEED


def _planted(r):
    return r.entry in ("minimizers", "super_kmers") and r.w > 1 and bool(P.shape_entries("window", r.unit, r.w, r.canonical))


def pos_labels(r):
    """the labels of pos_inputs(r), without building them"""
    return ["contig", "ragged", "ragged_n"] + (["planted"] if _planted(r) else [])


def pos_inputs(r):
    """the position-tiled inputs of a row: contig, ragged, ragged_n, and for a window shape of the tie corpus the planted batch"""
    mode = K.MODE[r.entry]
    seq, offs, _, g = K.contig(mode, r.w)
    out = [Input("contig", seq, offs, 0, seed_of(r), g, None)]
    for label, with_n in (("ragged", False), ("ragged_n", True)):
        seq, offs, _, g = K.ragged(mode, r.unit, r.w, with_n)
        out.append(Input(label, seq, offs, 0, seed_of(r), g, None))
    if _planted(r):
        bt = P.pos_batch("window", r.unit, r.w, r.canonical)
        teeth = [at for at, e in bt["plants"] if P.has_teeth(e)]
        n = len(bt["seq"])
        picks = [teeth[len(teeth) // 4], teeth[len(teeth) // 2], teeth[3 * len(teeth) // 4]]
        out.append(Input("planted", bt["seq"], np.array([0, n], np.uint64), 0, bt["seed"], P.plan_pos(mode, 0, n, r.w), picks))
    return out


def frl_input(r):
    seq, offs, L, g = K.reads(K.MODE[r.entry], r.read_len, r.unit, r.w, r.canonical)
    assert g is not None
    return Input("reads", seq, offs, L, K.SEED, g, None)


def _dense_plan(n):
    return dict(origin=0, stride=H, own=H // 4, n_tiles=(n - 1) // H + 1)


@functools.lru_cache(None)
def dense_inputs(k):
    """inputs of the scans that tile by H positions (dense k-mers, every 128-bit entry), about three tiles and a partial one: a contig with the
    repeat island across tiles 1 | 2; ragged reads with starts planted at the tile and the wave border; the same with N's there instead"""
    n = 3 * H + 1391
    g = _dense_plan(n)
    seq = O.synth(511 + k, n)
    at = 2 * H - len(K.ISLAND) // 2
    seq[at:at + len(K.ISLAND)] = np.frombuffer(K.ISLAND, np.uint8)
    seq[::7] |= 0x20
    out = [Input("contig", seq, np.array([0, n], np.uint64), 0, K.SEED, g, None)]
    places = K.planted_places(g)
    for label, with_n in (("ragged", False), ("ragged_n", True)):
        rng = np.random.default_rng(13 * k + with_n)
        lens = [x for x in (k - 1, k, k + 1, 1) if x >= 1] + rng.integers(1, 700, 80).tolist()
        starts = {0} | {int(x) for x in np.cumsum(lens) if x < n}
        seq = O.synth(523 + k, n)
        seq[rng.integers(0, n, 12)] = ord("N")
        seq[::7] |= 0x20
        if with_n:
            starts -= set(places)
            seq[places] = ord("N")
        else:
            starts |= set(places)
        out.append(Input(label, seq, np.array(sorted(starts) + [n], np.uint64), 0, K.SEED, g, None))
    return out


def batch128(k, rng):
    """two tiles and 1,007 bases; reads of length k-1, k, k+1 (and 1, 150); breaks at the first and the last base of a tile; bytes >= 0x80
    (the batch of test_emu_minimizers128.py)"""
    n = 2 * H + 1007
    seq = rng.choice(np.frombuffer(b"ACGTacgtUu", np.uint8), n)
    lens = [k + 1, k, max(k - 1, 1), 1, 150]
    offs = [0]
    for length in lens:
        offs.append(offs[-1] + length)
    offs += [H - 3, H + k, 2 * H - 1, 2 * H + 500, n]
    offs = np.array(sorted(set(offs)), np.uint64)
    seq[[H, 2 * H - 1, 2 * H, 3000, 3001, n - 1 - 2 * k]] = ord("N")  # tile 1's first and last base, tile 2's first
    seq[5000] = 0x80
    seq[5200] = 0xFF
    return seq, offs


def inputs128(shape):
    """the inputs of a 128-bit shape: the three H-tiled ones above, and the batch with bytes >= 0x80 and breaks on tile borders"""
    k = shape[1][0]
    out = list(dense_inputs(k))
    seq, offs = batch128(k, np.random.default_rng(3000 + k))
    out.append(Input("breaks", seq, offs, 0, K.SEED, _dense_plan(len(seq)), None))
    return out


# ----------------------------------------------------------------------------- cut sets

def _inside(cuts, n):
    return sorted({int(c) for c in cuts if 0 < c < n})


def island_of(g):
    """(first base, middle of the homopolymer, last base) of kernel_cases.contig's repeat island"""
    border = g["origin"] + 2 * g["stride"]
    at = border - len(K.ISLAND) // 2
    return at, border, at + len(K.ISLAND) - 1


def short_read_followers(offs, unit):
    offs = np.asarray(offs, np.int64)
    return [int(b) for a, b in zip(offs[:-1], offs[1:]) if b - a < unit]


def two_way(inp, unit, w):
    """the cuts c of the two ranges [0, c), [c, n)"""
    n, g = len(inp.seq), inp.plan
    T = g["origin"] + g["stride"]
    W = g["origin"] + 2 * g["stride"] + g["stride"] // 4
    cuts = set(range(1, 18)) | set(range(T - 17, T + 18)) | set(range(W - 2, W + 3)) | set(range(n - unit - w - 1, n))
    places = K.planted_places(g)
    if inp.label == "ragged":
        cuts |= {p + d for p in places for d in (-1, 0, 1)} | set(short_read_followers(inp.offs, unit))
    elif inp.label == "ragged_n":
        cuts |= {p + d for p in places for d in (-unit, -1, 0, 1)}
    elif inp.label == "contig":
        cuts |= set(island_of(g))
    elif inp.label == "planted":
        cuts |= {at + d for at in inp.extra for d in range(-2, w + 3)}
    elif inp.label == "breaks":
        cuts |= {int(o) + d for o in inp.offs[1:-1] for d in (-1, 0, 1)}
    return _inside(cuts, n)


def anchors(inp):
    g = inp.plan
    T = g["origin"] + g["stride"]
    if inp.label in ("ragged", "ragged_n"):
        return [T, K.planted_places(g)[4]]
    if inp.label == "contig":
        return [T, island_of(g)[1]]
    if inp.label == "planted":
        return [T, inp.extra[1]]
    return [T]


def three_way(inp, unit, w):
    """the cuts (c, c + d) of the three ranges [0, c), [c, c + d), [c + d, n)"""
    n, g = len(inp.seq), inp.plan
    out = []
    for p in anchors(inp):
        for c in (p - 1, p, p + 1, p + 15, p + 16):
            for d in sorted({1, 2, w - 1, w, w + 1, 16} - {0}):
                out.append((c, c + d))
    p = anchors(inp)[0]
    out.append((p - g["stride"] // 2 + 5, p + g["stride"] // 2 + 5))  # a middle range of one tile's length whose ends lie on no border of the whole scan
    assert all(0 < a < b < n for a, b in out)
    return out


def cut_sets(inp, unit, w):
    return [(c,) for c in two_way(inp, unit, w)] + three_way(inp, unit, w)


def frl_cut_sets(inp, r):
    """cut sets of a batch of fixed-length reads: aligned cuts at reads around the tile border; unaligned ones beside it, one `unit` into a read, at
    the first base of a read's last window and behind it, and one base before the end; three-way ones that mix both"""
    n, L, rpt = len(inp.seq), inp.read_len, inp.plan["reads_per_tile"]
    last_window = (rpt + 1) * L + L - (r.unit + r.w - 1)
    aligned = [L, rpt * L - L, rpt * L, rpt * L + L, n - L]
    unaligned = [rpt * L - 1, rpt * L + 1, rpt * L + r.unit, last_window, last_window + 1, n - 1]
    sets = [(c,) for c in aligned + unaligned] + [(L, 2 * L), (L + 5, 3 * L), (2 * L, 2 * L + 7)]
    assert all(0 < cs[0] and cs[-1] < n and list(cs) == sorted(set(cs)) for cs in sets)
    assert all(c % L == 0 for c in aligned) and all(c % L for c in unaligned)
    return sets


def read_tiled(first, end, L):
    """a range of a batch of reads of L bases takes the read-tiled kernels iff it holds whole reads (plan_scan_frl); any other range takes the
    position-tiled ones, with sequence starts from the start bits"""
    return first % L == 0 and end % L == 0


def ranges_of(cuts, n):
    """[(first, end)] of a cut set"""
    edges = [0] + list(cuts) + [n]
    return list(zip(edges[:-1], edges[1:]))


def call_args(first, end, n):
    """(first, n) as a scan takes them: the last range runs 'to the end' (n = 0)"""
    return (first, 0) if end == n and first < n else (first, end - first)


# ----------------------------------------------------------------------------- what a range must report, 64-bit entries

def _xor(a):
    return O.xor_reduce(a)


class Whole:
    """one whole-batch run of the oracle for a row and an input; of_range(first, end) derives a range's result from it by the rules of the
    module docstring (dict as kernel_cases.expected gives, for kernel_cases.assert_same)"""

    def __init__(self, r, inp):
        self.r, self.inp, self.n = r, inp, len(inp.seq)
        c, k = bool(r.canonical), r.unit + r.w - 1
        if r.entry == "syncmers":
            self.count, self.pos = O.syncmers(inp.seq, inp.offs, k, r.unit, r.offsets[0], r.offsets[1], c)
        else:
            self.groups = O.super_kmers(inp.seq, inp.offs, k, r.unit, inp.seed, c)
            self.fp = self.groups[1].astype(np.int64)
            self.last = self.fp + self.groups[3].astype(np.int64) - 1
            self.kmers = int(self.groups[3].astype(np.int64).sum())  # every valid k-mer lies in exactly one group

    def whole(self):
        """the oracle's own whole-batch answer, through its own entry point"""
        r, inp = self.r, self.inp
        if r.entry == "syncmers":
            return dict(positions=self.pos, xor_pos=_xor(self.pos), count=len(self.pos))
        if r.entry == "super_kmers":
            g = self.groups
            return dict(zip(K.SK_FIELDS, g), xor_value=_xor(g[0]), xor_hash=_xor(g[4]), xor_pos=_xor(g[1] + g[2].astype(np.uint64)), aux=len(g[0]), count=len(g[0]))
        v, p, h = O.minimizers(inp.seq, inp.offs, r.unit, r.w, inp.seed, bool(r.canonical))
        return self._min(v, p, h)

    def _min(self, v, p, h, origin=0):
        if self.r.entry == "hash_sample":
            keep = h < np.uint64(K.THRESHOLD)
            v, p, h = v[keep], p[keep], h[keep]
        p = p + np.uint64(origin)
        return dict(values=v, positions=p, hashes=h, xor_value=_xor(v), xor_hash=_xor(h), xor_pos=_xor(p), count=len(v))

    def of_range(self, first, end, origin=0):
        r = self.r
        if r.entry == "syncmers":
            pos = self.pos[(self.pos >= np.uint64(first)) & (self.pos < np.uint64(end))] + np.uint64(origin)
            return dict(positions=pos, xor_pos=_xor(pos), count=len(pos))
        mn, fp, mp, sz, hs = self.groups
        if r.entry in ("minimizers", "hash_sample"):
            keep = (self.fp >= first) & (self.fp < end)  # the first electing window starts in the range
            return self._min(mn[keep], (fp + mp.astype(np.uint64))[keep], hs[keep], origin)
        keep = (self.last >= first) & (self.fp < end)
        a, b = np.maximum(self.fp[keep], first), np.minimum(self.last[keep], end - 1)
        cmp_ = (mp[keep].astype(np.int64) - (a - self.fp[keep])).astype(np.uint8)
        cfp, csz = (a + origin).astype(np.uint64), (b - a + 1).astype(np.uint8)
        return dict(minimizers=mn[keep], first_pos=cfp, mm_pos=cmp_, sizes=csz, hashes=hs[keep], xor_value=_xor(mn[keep]), xor_hash=_xor(hs[keep]),
                    xor_pos=_xor(cfp + cmp_.astype(np.uint64)), aux=int(keep.sum()), count=int(keep.sum()))

    def records_of_range(self, first, end):
        """(records uint64[g, 2], hashes) of bl_scan_super_kmer_records: superkmer_model.pack of the clipped groups, positions relative to the batch"""
        import superkmer_model as SM

        x = self.of_range(first, end)
        recs = SM.pack(self.inp.seq, x["first_pos"].astype(np.int64), x["sizes"].astype(np.int64), self.r.unit + self.r.w - 1, x["mm_pos"].astype(np.int64))
        return np.asarray(recs, np.uint64).reshape(-1, 2), x["hashes"]


def concat(parts, entry):
    """the concatenation of consecutive ranges' results: arrays end to end, digest words folded as the scan folds them"""
    out = {f: np.concatenate([np.asarray(p[f]) for p in parts]) for f in K.FIELDS[entry]}
    out["count"] = sum(int(p["count"]) for p in parts)
    for d in K.DIGEST[entry]:
        out[d] = sum(int(p[d]) for p in parts) if d == "aux" else functools.reduce(lambda a, b: a ^ b, (int(p[d]) for p in parts), 0)
    return out


class WholeKmers:
    """the dense k-mer scan of a whole batch from the oracle's units: value, hash and validity per position (0 where no k-mer starts)"""

    def __init__(self, inp, k, canonical, seed, drop_last):
        vals, valid = O.units(inp.seq, inp.offs, k, canonical)
        valid = valid.copy()
        if drop_last:  # the k-mer that ends its sequence is no item
            offs = np.asarray(inp.offs, np.int64)
            at = offs[1:] - k
            valid[at[at >= offs[:-1]]] = 0
        ok = valid.astype(bool)
        self.valid = valid
        self.values = np.where(ok, vals, np.uint64(0))
        self.hashes = np.where(ok, O.hash64_np(vals, seed), np.uint64(0))

    def of_range(self, first, end):
        s = slice(first, end)
        return dict(values=self.values[s], hashes=self.hashes[s], valid=self.valid[s], count=int(self.valid[s].sum()), xor_value=_xor(self.values[s]),
                    xor_hash=_xor(self.hashes[s]), sum_hash=int(self.hashes[s].sum(dtype=np.uint64)))


def assert_same_kmers(got, want, what):
    for d in ("count", "xor_value", "xor_hash", "sum_hash"):
        assert int(got[d]) == int(want[d]), (what, d, int(got[d]), int(want[d]))
    for f in ("values", "hashes", "valid"):
        g = np.asarray(got[f])
        assert g.shape == want[f].shape, (what, f, g.shape, want[f].shape)
        bad = np.nonzero(g != want[f])[0]
        assert len(bad) == 0, (what, f, "first differing position", int(bad[0]))


# ----------------------------------------------------------------------------- what a range must report, 128-bit entries

THRESHOLD128 = 1 << 62


class Whole128:
    """one whole-batch run of the model of a 128-bit entry; of_range(first, end) is the model's own range view (kmers128_model.digest / sample,
    minimizers128_model.minimizers, syncmers128_model.syncmers) or records128_cases.Expect.of_range"""

    def __init__(self, shape, inp, canonical=True, drop_last=False, seed=SEED128):
        import kmers128_model as KM
        import minimizers128_model as MM
        import records128_cases as R
        import syncmers128_model as SY

        self.entry, self.args, self.inp, self.n = shape[0], shape[1], inp, len(inp.seq)
        self.KM, self.MM, self.SY = KM, MM, SY
        a = shape[1]
        if self.entry in ("kmers128", "hash_sample128"):
            self.m = KM.scan(inp.seq.tobytes(), inp.offs, a[0], seed, canonical, drop_last)
        elif self.entry == "minimizers128":
            self.m = MM.scan(inp.seq.tobytes(), inp.offs, a[0], a[1], seed, canonical, drop_last, 16)
        elif self.entry == "syncmers128":
            self.m = SY.scan(inp.seq.tobytes(), inp.offs, a[0], a[1], seed, canonical, drop_last, 16)
            self.soff, self.eoff = 0, a[0] - a[1]  # closed offsets: the first and the last s-mer
        else:
            self.m = R.Expect(inp.seq, inp.offs, 0, a[0], a[1], canonical, seed=seed)

    def of_range(self, first, end, origin=0):
        """kmers128: dict(values uint64[n, 2] (low, high), hashes, valid, + digest); the samplers: dict(values[n, 2], positions, hashes, + digest);
        syncmers128: dict(positions, count, xor_pos); records128: dict(records uint64[g, 4], hashes, count)"""
        m = self.m
        if self.entry == "kmers128":
            s = slice(first, end)
            return dict(self.KM.digest(m, first, end), values=np.stack([m["lo"][s], m["hi"][s]], axis=1), hashes=m["hashes"][s], valid=m["valid"][s])
        if self.entry == "hash_sample128":
            x = self.KM.sample(m, THRESHOLD128, first, end, origin)
        elif self.entry == "minimizers128":
            x = self.MM.minimizers(m, first, end, origin)
        elif self.entry == "syncmers128":
            return self.SY.syncmers(m, self.soff, self.eoff, first, end, origin)
        else:
            recs, hs = m.of_range(first, end - first)
            return dict(records=recs, hashes=hs, count=len(hs), xor_hash=_xor(hs))
        return dict(x, values=np.stack([x["lo"], x["hi"]], axis=1))


FIELDS128 = {"kmers128": ("values", "hashes", "valid"), "hash_sample128": ("values", "positions", "hashes"), "minimizers128": ("values", "positions", "hashes"),
             "syncmers128": ("positions",), "records128": ("records", "hashes")}
DIGEST128 = {"kmers128": ("count", "xor_value", "aux", "xor_hash", "sum_hash"), "hash_sample128": ("count", "xor_value", "aux", "xor_hash", "xor_pos"),
             "minimizers128": ("count", "xor_value", "aux", "xor_hash", "xor_pos"), "syncmers128": ("count", "xor_pos"), "records128": ("count", "xor_hash")}


def assert_same128(entry, got, want, what):
    for d in DIGEST128[entry]:
        assert int(got[d]) == int(want[d]), (what, d, hex(int(got[d])), hex(int(want[d])))
    for f in FIELDS128[entry]:
        g, x = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == x.shape, (what, f, g.shape, x.shape)
        bad = np.nonzero(g.astype(x.dtype) != x)[0]
        assert len(bad) == 0, (what, f, "first differing element", int(bad[0]))
