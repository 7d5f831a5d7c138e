"""TEST INFRASTRUCTURE: the batches, tables and expected records of the per-read count tests (tests/test_emu_read_counts.py on the host
emulation, tests/test_gpu_read_counts.py on the device).  Expected records come from tests/kmers128_model.py and a Python dict, position
by position; nothing here shares code with the library.

The record of a sequence over a range [first, end): its valid k-mers p in the range (validity as the model's), their counts
table.get(key, 0), and the position p - offset relative to the sequence, where the sequence of p is the LAST one whose offset is <= p.
A call touches the records from the sequence of `first` to the sequence of `end - 1`, the empty ones between them included.
"""
import functools
import struct

import numpy as np

import kmers128_model as M
import lookup_cases as LC

H = 4096
N = 2 * H + 1007  # about two and a quarter tiles, as lookup_cases.make_batch
U32 = (1 << 32) - 1
U64 = (1 << 64) - 1
KS = (1, 16, 31, 32, 33, 47, 64)
MIN_COUNTS = (1, 2, U32)
FIXED = (7, 150, 4096, 5000)  # read lengths of the fixed-length batches: the last read is shorter in each (N is a multiple of none)
RECORD = np.dtype([("n_kmers", "<u4"), ("n_found", "<u4"), ("n_solid", "<u4"), ("min_count", "<u4"), ("max_count", "<u4"), ("reserved", "<u4"),
                   ("sum_counts", "<u8"), ("weak_begin", "<u8"), ("weak_end", "<u8")])
assert RECORD.itemsize == 48
FIELDS = [f for f in RECORD.names if f != "reserved"]
IDENTITY = np.array([(0, 0, 0, U32, 0, 0, 0, U64, 0)], RECORD)[0]
CANARY_BYTE = 0xC5


def _bases(rng, n):
    seq = rng.choice(np.frombuffer(b"ACGTacgtUu", np.uint8), n)
    seq[[H, 2 * H - 1, 2 * H]] = ord("N")  # the first and the last base of a tile
    seq[[3000, 3001]] = ord("N")
    seq[5000] = 0x80
    seq[5200] = 0xFF
    return seq


def ragged_batch(k, rng):
    """(seq, offsets): empty sequences first, last and two in a row in the middle; reads of k + 1, k and k - 1 bases; two runs of reads of
    every length 1 .. 17 (several whole reads inside one lane of 16 positions, reads astride a lane edge); three one-base reads of N;
    thirty reads of k + 1 bases (two k-mers each); a read across the wave edge 3072; one read over three tiles (4000 .. 8300, across
    the tile edges 4096 and 8192); reads of k + 2 bases to the end."""
    seq = _bases(rng, N)
    lens = [0, k + 1, k, max(k - 1, 1)]
    lens += [length for length in range(1, 18) for _ in range(2)]
    n_at = sum(lens)
    lens += [1, 1, 1] + [k + 1] * 30
    offs = [0]
    for length in lens:
        offs.append(offs[-1] + length)
    assert offs[-1] < 3000
    seq[n_at:n_at + 3] = ord("N")
    offs += [3000, 3100, 3100, 3100, 4000, 8300]
    while offs[-1] + k + 2 < N:
        offs.append(offs[-1] + k + 2)
    offs += [N, N]
    offs = np.array(offs, np.uint64)
    assert (np.diff(offs.astype(np.int64)) >= 0).all() and offs[0] == 0 and offs[1] == 0 and offs[-2] == N
    return seq, offs


def fixed_offsets(n, read_len):
    return np.array(list(range(0, n, read_len)) + [n], np.uint64)


def own_table(m, k, canonical):
    """the batch's own k-mers with their true multiplicities, a third dropped (lookup_cases.own_table), the smallest kept key's count
    forced to 0 and the largest one's to 2^32 - 1.  k = 1 has four keys (two canonical ones) and the hash rule may keep them all: the key
    of C is dropped there instead."""
    if k == 1:
        t = LC.own_table(m, drop=False)
        t.pop(1, None)
    else:
        t = LC.own_table(m)
    keys = sorted(t)
    if len(keys) >= 3:
        t[keys[0]] = 0
    if len(keys) >= 1:
        t[keys[-1]] = U32
    return t


def seq_index(offs, positions):
    """the last sequence whose offset is <= the position"""
    return np.searchsorted(offs, positions, side="right").astype(np.int64) - 1


def touched(offs, first, end):
    lo, hi = seq_index(offs, np.array([first, end - 1], np.uint64))
    return int(lo), int(hi)


def expected_records(m, table, offs, first, end, min_count, into=None):
    """RECORD array of len(offs) - 1 entries after one call over [first, end).  into=None: INIT on an array of canaries (untouched
    records keep CANARY_BYTE bytes); into=an earlier array: ACCUMULATE."""
    n_seqs = len(offs) - 1
    lo, hi = touched(offs, first, end)
    if into is None:
        out = np.frombuffer(bytes([CANARY_BYTE]) * (48 * n_seqs), RECORD).copy()
        out[lo:hi + 1] = IDENTITY
    else:
        out = into.copy()
    keys = LC.kmer_keys(m)
    pos = np.nonzero(m["valid"][first:end])[0] + first
    seqs = seq_index(offs, pos.astype(np.uint64))
    rows = {}  # sequence -> the eight fields as Python integers
    for p, q in zip(pos.tolist(), seqs.tolist()):
        assert lo <= q <= hi
        r = rows.setdefault(q, {f: int(out[q][f]) for f in FIELDS})
        c = table.get(keys[p], 0)
        rel = p - int(offs[q])
        r["n_kmers"] += 1
        r["n_found"] += keys[p] in table
        r["n_solid"] += c >= min_count
        r["min_count"] = min(r["min_count"], c)
        r["max_count"] = max(r["max_count"], c)
        r["sum_counts"] += c
        if c < min_count:
            r["weak_begin"] = min(r["weak_begin"], rel)
            r["weak_end"] = max(r["weak_end"], rel + 1)
    for q, r in rows.items():
        out[q] = tuple(r[f] if f != "reserved" else int(out[q]["reserved"]) for f in RECORD.names)
    return out


@functools.lru_cache(maxsize=None)
def case(name, k, canonical, drop_last):
    """dict(seq, offs, read_len, null_offsets, m, table) — name: "ragged", "single" or "fixed<L>".  read_len / null_offsets: how the batch
    is uploaded and whether the call may go without offsets."""
    rng = np.random.default_rng(7000 + 100 * k + len(name))
    if name == "ragged":
        seq, offs = ragged_batch(k, rng)
        read_len, null_ok = 0, False
    elif name == "single":
        seq, offs = _bases(rng, N), np.array([0, N], np.uint64)
        read_len, null_ok = 0, True
    else:
        read_len = int(name[5:])
        seq, offs = _bases(rng, N), fixed_offsets(N, read_len)
        assert N % read_len != 0
        null_ok = True
    m = M.scan(seq.tobytes(), offs, k, 0, canonical, drop_last)
    return dict(name=name, k=k, canonical=canonical, drop_last=drop_last, seq=seq, offs=offs, read_len=read_len, null_ok=null_ok, m=m,
                table=own_table(m, k, canonical))


def self_check(c):
    """the ragged case holds what the record logic can get wrong (min_count = 1, the whole batch)"""
    r = expected_records(c["m"], c["table"], c["offs"], 0, len(c["seq"]), 1)
    lens = np.diff(c["offs"].astype(np.int64))
    assert not (r.view(np.uint8) == CANARY_BYTE).reshape(len(r), 48).all(axis=1)[1:-1].any()
    assert int((r["n_found"] < r["n_kmers"]).sum()) >= 20, "reads with an absent k-mer"
    weak = r["weak_end"] > 0
    assert int(weak[1:-1].sum()) >= 20, "reads with a weak span"
    assert int((r["n_kmers"][1:-1] == 0).sum()) >= 5, "reads without a k-mer"
    n_weak = r["n_kmers"] - r["n_solid"]
    several = r["n_kmers"] >= 2
    assert (weak & several & (n_weak == 1) & (r["weak_begin"] == 0))[1:-1].any(), "a read whose only weak k-mer is its first"
    # (its last k-mer: the last position at which one can start, less one under drop_last)
    last = lens[:len(r)] - c["k"] - (1 if c["drop_last"] else 0)
    assert (weak & several & (n_weak == 1) & (r["weak_begin"].astype(np.int64) == last))[1:-1].any(), "a read whose only weak k-mer is its last"
    assert set(range(1, 18)) <= set(lens.tolist()) and (lens[:-1][lens[1:] == 0] == 0).any()
    assert U32 in c["table"].values() and (len(c["table"]) < 3 or 0 in c["table"].values())  # (k = 1, canonical: one key is left)


def batch_file(seq, offs):
    return struct.pack("<QQ", len(seq), len(offs) - 1) + offs.tobytes() + seq.tobytes()


def table_file(table, key_words, k):
    return LC.table_file(key_words, 2 * k, table, [], [-1])


def wrong_offsets(offs, rng):
    """shuffled, the last entry too large"""
    w = offs.copy()
    rng.shuffle(w)
    w[-1] = np.uint64(int(offs[-1]) * 3 + 12345)
    return w


def parse_records(lines):
    rows = [tuple(int(x) for x in ln[2:]) for ln in lines if ln[0] == "record"]
    return np.array(rows, RECORD)


def same(a, b):
    return a.tobytes() == b.tobytes()


def merged(a, b):
    """two record arrays of disjoint ranges, merged field by field"""
    out = a.copy()
    for f in ("n_kmers", "n_found", "n_solid", "sum_counts"):
        out[f] = a[f] + b[f]
    for f in ("min_count", "weak_begin"):
        out[f] = np.minimum(a[f], b[f])
    for f in ("max_count", "weak_end"):
        out[f] = np.maximum(a[f], b[f])
    return out
