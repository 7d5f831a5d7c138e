"""What tests/test_emu_records128.py (CPU emulation under the sanitizers) and tests/test_gpu_records128.py (the kernels) share: the
shapes, the batches, the ranges aimed at tile edges, and the expected records of a range — superkmer128_model.pack over the oracle's
groups (oracle_lib.super_kmers), cut where a range cuts a group.  TEST INFRASTRUCTURE; nothing here runs code under test.

The tile-edge ranges.  A position-tiled scan of [first, end) has its tiles at origin + t * stride, origin = 16 * floor((first - 1) / 16)
(tie_plant.plan_pos, held against the emulation's emu_plan by the CPU test).  The last wave of a tile stages the fewest chunks behind its
own positions, so a full-size group (size == w: 2k - m bases) that begins at the tile's last positions is the one whose bases reach
furthest into what only the wide-record staging holds.  Two placements per picked group, by the choice of `first`:
    'last'   the group's first k-mer IS the last position its tile owns (first_pos = origin + stride - 1)
    'next'   the group's first k-mer is the position behind it (first_pos = origin + stride): it is decided by the owner of the tile's
             last position and built by that tile — the furthest a tile's group can begin
each once with the range running on, and once with the range ending at that k-mer (end = first_pos + 1: the group is cut to one k-mer)."""
import numpy as np

import oracle_lib as O
import superkmer128_model as M
import tie_plant as P

SEED = 0x5EED128
SHAPES = ((33, 32), (64, 32), (64, 6), (63, 4), (51, 21), (48, 17), (40, 9), (31, 15))  # w <= 32, w in 33..64, (64, 6) and (63, 4): 122 bases
EDGE_PICKS = 32
BIG = 200_000  # bases of the contig the tile-edge groups are picked from


def stride_of(w):
    """positions a tile owns (position-tiled layout)"""
    return P.plan_pos(P.MODE_SUPERKMER, 0, 1, w)["stride"]


def contig(k):
    """one contig of a little over three tiles, upper and lower case, no break"""
    n = 3 * stride_of(1) + 1234 + k
    seq = O.synth(1000 + k, n)
    seq[::7] |= 0x20
    return seq, None, 0


def ragged(k):
    """reads of 1 .. ~700 bases with N's: every read shorter than k, of exactly k, and long ones"""
    rng = np.random.default_rng(2000 + k)
    lens = np.concatenate([[1, k - 1, k, k + 1, 122, 123, 700], rng.integers(1, 700, 60)])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    seq = O.synth(2000 + k, int(offs[-1]))
    seq[rng.integers(0, len(seq), 40)] = ord("N")
    return seq, offs, 0


def reads150(k):
    """150-bp reads: the read-tiled layout where the window width has one (w = 17), position-tiled elsewhere"""
    n = 150 * 300
    return O.synth(3000 + k, n), None, 150


def short(k):
    """a batch shorter than one tile (and than one wave's positions): every group lies within a few hundred bases of the batch's end"""
    return O.synth(4000 + k, 300 + k), None, 0


LAYOUTS = {"contig": contig, "ragged": ragged, "reads150": reads150, "short": short}


def offsets_of(seq, offs, read_len):
    if offs is not None:
        return offs
    return O.fixed_offsets(len(seq), read_len) if read_len else np.array([0, len(seq)], np.uint64)


class Expect:
    """the oracle's groups of one batch, packed once; expected records and hashes of any range"""

    def __init__(self, seq, offs, read_len, k, m, canonical, seed=SEED):
        self.seq, self.k, self.m = seq, k, m
        _, fp, mp, sz, hs = O.super_kmers(seq, offsets_of(seq, offs, read_len), k, m, seed, canonical)
        self.fp, self.mp, self.sz, self.hs = fp.astype(np.int64), mp.astype(np.int64), sz.astype(np.int64), hs
        self.recs = M.pack(seq, self.fp, self.sz, k, self.mp)

    def of_range(self, first=0, n=0):
        """(records uint64[g, 4], hashes uint64[g]) of the k-mers whose first base lies in [first, first + n) (n = 0: to the end)"""
        end = len(self.seq) if n == 0 else min(first + n, len(self.seq))
        last = self.fp + self.sz - 1
        keep = np.nonzero((last >= first) & (self.fp < end))[0]
        recs, hs = self.recs[keep].copy(), self.hs[keep].copy()
        for i, g in enumerate(keep.tolist()):
            a, b = max(int(self.fp[g]), first), min(int(last[g]), end - 1)
            if (a, b) != (int(self.fp[g]), int(last[g])):  # cut by the range: the same occurrence, fewer k-mers
                recs[i] = M.pack(self.seq, [a], [b - a + 1], self.k, [int(self.mp[g]) - (a - int(self.fp[g]))])[0]
        return recs, hs


def edge_jobs(exp, k, m):
    """[(first, n, placement, group index)]: EDGE_PICKS full-size groups per placement, each with the range running on and with the range
    ending at the group's first k-mer.  Asserts that every pick sits where it is meant to."""
    w = k - m + 1
    stride = stride_of(w)
    full = (exp.sz == w) & (exp.fp > stride + 64) & (exp.fp + 400 < len(exp.seq))
    assert int((exp.sz == w).sum()) >= 16 * 2 * EDGE_PICKS, "too few full-size groups to pick from"
    jobs = []
    for placement, residue, back in (("last", 15, stride - 1), ("next", 0, stride)):
        picks = np.nonzero(full & (exp.fp % 16 == residue))[0]
        assert len(picks) >= EDGE_PICKS, (placement, len(picks))
        for g in picks[np.linspace(0, len(picks) - 1, EDGE_PICKS).astype(int)].tolist():
            fp = int(exp.fp[g])
            first = fp - back + 1  # origin = 16 * floor((first - 1) / 16) = fp - back
            plan = P.plan_pos(P.MODE_SUPERKMER, first, fp + 300, w)
            assert plan["origin"] + back == fp and plan["stride"] == stride and int(exp.sz[g]) == w and first > 0
            assert (fp - plan["origin"]) // stride == (0 if placement == "last" else 1)  # 'next' lies in tile 1's positions, and tile 0 builds it
            jobs.append((first, fp + 300 - first, placement, g))  # the range runs on
            jobs.append((first, fp + 1 - first, placement, g))    # the range ends at the group's first k-mer
    return jobs


def canonical_kmers128(seq, k):
    """the canonical k-mers (32 < k <= 64) of ONE sequence of ACGT, as uint64[n - k + 1, 2] (high, low), from the oracle's 32-mers: a
    k-mer is its first 32 bases times 4^(k - 32) plus the last k - 32 of its last 32; the reverse strand the same on the reverse
    complement of the sequence"""
    assert 32 < k <= 64
    n, r = len(seq), k - 32

    def words(s):
        f32, valid = O.units(s, np.array([0, n], np.uint64), 32, False)
        assert valid[:n - 31].all()
        top, low = f32[:n - k + 1], f32[k - 32:n - 31]
        if r == 32:
            return top.copy(), low.copy()
        return top >> np.uint64(64 - 2 * r), (top << np.uint64(2 * r)) | (low & np.uint64((1 << (2 * r)) - 1))

    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGTacgt")] = list(b"TGCATGCA")
    fh, fl = words(np.ascontiguousarray(seq))
    rh, rl = (a[::-1] for a in words(np.ascontiguousarray(comp[seq][::-1])))
    rev = (rh < fh) | ((rh == fh) & (rl < fl))
    return np.stack([np.where(rev, rh, fh), np.where(rev, rl, fl)], axis=1)


def unique_counts128(hi_lo):
    """(distinct rows in ascending 128-bit order, their multiplicities)"""
    order = np.lexsort((hi_lo[:, 1], hi_lo[:, 0]))
    s = hi_lo[order]
    new = np.concatenate([[True], (s[1:] != s[:-1]).any(1)])
    starts = np.nonzero(new)[0]
    return s[starts], np.diff(np.concatenate([starts, [len(s)]]))
