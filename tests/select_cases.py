"""A numpy model of bl_batch_select and bl_read_spans (include/biolib_amd.h) and the named cases the emulation (test_emu_select.py) and
the GPU tests (test_gpu_select.py) share.  The model is written from the header's text, not from the kernels: it cuts python slices.

  select_model(bases, offs, spans, keep_empty)   -> dict(bases, offsets, source_index, n_seqs, n_bases, fixed_len)
  read_spans_model(lengths, records, rule, stat) -> uint64 [n_seqs, 2]
  batch()                                        -> the case batch: about 200 named sequences, about 94,000 bases
  variants()                                     -> {name: dict(bases, offs | None, read_len, spans, keep_empty)}: the other sources
  span_cases()                                   -> (lengths, records, stat, {name: rule}) for bl_read_spans
"""
import numpy as np

U64 = (1 << 64) - 1
LENGTHS = (0, 1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 151, 1000, 5000)
TRIM = dict(none=0, prefix=1, suffix=2, longer=3)
RECORD = np.dtype([("n_kmers", "<u4"), ("n_found", "<u4"), ("n_solid", "<u4"), ("min_count", "<u4"), ("max_count", "<u4"), ("reserved", "<u4"),
                   ("sum_counts", "<u8"), ("weak_begin", "<u8"), ("weak_end", "<u8")])


def fixed_offsets(n_bases, read_len):
    """the offsets of a fixed-read-length batch: multiples of read_len, the last read cut at n_bases"""
    n = (n_bases + read_len - 1) // read_len
    return np.minimum(np.arange(n + 1, dtype=np.uint64) * np.uint64(read_len), np.uint64(n_bases))


def read_lengths(offs, n_bases):
    """(first, length) per read with the header's safety rule: offsets clamped to [0, n_bases], a decreasing pair is length 0"""
    o = np.minimum(np.asarray(offs, np.uint64), np.uint64(n_bases)).astype(np.int64)
    return o[:-1], np.maximum(o[1:] - o[:-1], 0)


def select_model(bases, offs, spans, keep_empty=False):
    bases = np.asarray(bases, np.uint8)
    first, length = read_lengths(offs, len(bases))
    spans = np.asarray(spans, np.uint64).reshape(-1, 2)
    assert len(spans) == len(first)
    pieces, offsets, index = [], [0], []
    for i in range(len(first)):
        L = int(length[i])
        b, e = min(int(spans[i, 0]), L), min(int(spans[i, 1]), L)
        if e <= b:
            if keep_empty:
                offsets.append(offsets[-1])
                index.append(i)
            continue
        pieces.append(bases[int(first[i]) + b:int(first[i]) + e])
        offsets.append(offsets[-1] + e - b)
        index.append(i)
    out = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    offsets = np.array(offsets, np.uint64)
    lens = np.diff(offsets.astype(np.int64))
    # the parser's rule: more than one sequence, every length equal (and not 0: a batch of empty sequences has nothing to tile)
    fixed = int(lens[0]) if len(lens) > 1 and lens[0] > 0 and (lens == lens[0]).all() else 0
    return dict(bases=out, offsets=offsets, source_index=np.array(index, np.uint64), n_seqs=len(index), n_bases=len(out), fixed_len=fixed)


def rule(trim="prefix", k=31, min_len=None, min_kmers=0, solid_min=(0, 1), solid_max=(1, 1), stat=(0, 2**32 - 1)):
    return dict(trim=TRIM[trim], k=k, min_len=k if min_len is None else min_len, min_kmers=min_kmers, solid_min=solid_min, solid_max=solid_max, stat=stat)


def rule_words(r):
    """the twelve numbers of a bl_span_rule in field order (min_len as one 64-bit number)"""
    return [r["trim"], r["k"], r["min_len"], r["min_kmers"], r["solid_min"][0], r["solid_min"][1], r["solid_max"][0], r["solid_max"][1], r["stat"][0],
            r["stat"][1], r.get("reserved", 0)]


def read_spans_model(lengths, records, r, stat=None):
    out = np.zeros((len(lengths), 2), np.uint64)
    for i, L in enumerate(int(x) for x in lengths):
        rec = records[i]
        nk, ns = int(rec["n_kmers"]), int(rec["n_solid"])
        keep = nk >= r["min_kmers"] and ns * r["solid_min"][1] >= nk * r["solid_min"][0] and ns * r["solid_max"][1] <= nk * r["solid_max"][0]
        if stat is not None:
            keep = keep and r["stat"][0] <= int(stat[i]) <= r["stat"][1]
        if not keep:
            continue
        b, e = 0, L
        wb, we = int(rec["weak_begin"]), int(rec["weak_end"])
        if wb != U64 and r["trim"] != TRIM["none"]:
            pe, sb = min(L, wb + r["k"] - 1), min(L, we)
            if r["trim"] == TRIM["prefix"] or (r["trim"] == TRIM["longer"] and pe >= L - sb):
                e = pe
            else:
                b = sb
        if e - b >= r["min_len"]:
            out[i] = (b, e)
    return out


# ---- bl_batch_select: the case batch

def span_kinds(L):
    """{kind: (begin, end)} for a read of L bases"""
    return {"whole": (0, L), "empty": (0, 0), "begin_at_L": (L, L + 5), "begin_past_L": (L + 3, U64), "end_past_L": (0, L + 100),
            "begin_gt_end": (min(L, 5) + 2, 2), "first_byte": (0, 1), "last_byte": (max(L, 1) - 1, L), "prefix": (0, L // 2), "suffix": (L // 3, U64),
            "middle": (L // 4, L - L // 4)}


def special_bytes(rng, n):
    """mostly ACGT; N, lower case, 0 and 255 sprinkled in"""
    a = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    odd = rng.random(n) < 0.04
    a[odd] = rng.choice(np.array([0, 255, ord("N"), ord("a"), ord("c"), ord("g"), ord("t"), ord("n")], np.uint8), int(odd.sum()))
    return a


def batch():
    rng = np.random.default_rng(20261)
    reads = [(f"{kind}_{L}", L, span) for L in LENGTHS for kind, span in span_kinds(L).items()]
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    reads[60:60] = [(f"long_{j}", 5000, span) for j, span in enumerate(((1, 4999), (0, 5000), (17, 4990), (3, U64)))]  # whole waves inside one read
    reads += [(f"run_len_{n}", 40, (3, 3 + n)) for n in range(1, 18)]      # every destination residue mod 16
    reads += [(f"one_byte_{j}", 5, (2, 3)) for j in range(17)]             # seventeen sequences inside two chunks
    reads += [("last_reaches_n_bases", 77, (10, U64))]
    lengths = np.array([r[1] for r in reads], np.int64)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    bases = special_bytes(rng, int(offs[-1]))
    bases[-1] = 255  # the source's very last byte is recognisable
    spans = np.array([r[2] for r in reads], np.uint64)
    return dict(names=[r[0] for r in reads], bases=bases, offs=offs, spans=spans)


def self_check(b):
    """the case batch holds what its description promises"""
    m = select_model(b["bases"], b["offs"], b["spans"])
    first, length = read_lengths(b["offs"], len(b["bases"]))
    src = [(int(first[i]) + min(int(b["spans"][i, 0]), int(length[i]))) % 16 for i in m["source_index"].astype(np.int64)]
    assert set(src) == set(range(16)), "every source residue mod 16"
    assert set(int(x) % 16 for x in m["offsets"][:-1]) == set(range(16)), "every destination residue mod 16"
    assert 190 <= len(b["names"]) <= 230 and 60_000 <= len(b["bases"]) <= 100_000
    assert m["n_bases"] > 2 * 16384, "three workgroups of the gather (16 KiB of the result each), eleven waves"
    assert m["bases"][-1] == 255 and int(m["source_index"][-1]) == len(b["names"]) - 1, "the last span reaches n_bases"
    for byte in (0, 255, ord("N"), ord("a")):
        assert (m["bases"] == byte).any()
    lens = np.diff(m["offsets"].astype(np.int64))
    assert max(np.convolve(lens == 1, np.ones(17, int), "valid")) == 17, "seventeen one-byte sequences in a row"
    return m


def variants():
    rng = np.random.default_rng(20262)
    b = batch()
    out = {"keep_empty": dict(bases=b["bases"], offs=b["offs"], read_len=0, spans=b["spans"], keep_empty=True),
           "all_dropped": dict(bases=b["bases"], offs=b["offs"], read_len=0, spans=np.zeros_like(b["spans"]), keep_empty=False),
           "all_dropped_keep_empty": dict(bases=b["bases"], offs=b["offs"], read_len=0, spans=np.zeros_like(b["spans"]), keep_empty=True)}
    # fixed-length source, NULL offsets, the last read cut short
    n_bases, read_len = 150 * 40 + 77, 150
    kinds = [list(span_kinds(150).values())[i % 11] for i in range(41)]
    out["fixed_source"] = dict(bases=special_bytes(rng, n_bases), offs=None, read_len=read_len, spans=np.array(kinds, np.uint64), keep_empty=False)
    out["fixed_source_keep_empty"] = dict(out["fixed_source"], keep_empty=True)
    out["single_sequence"] = dict(bases=special_bytes(rng, 3001), offs=None, read_len=0, spans=np.array([[7, 2990]], np.uint64), keep_empty=False)
    out["single_sequence_whole"] = dict(bases=special_bytes(rng, 3001), offs=None, read_len=0, spans=np.array([[0, U64]], np.uint64), keep_empty=False)
    # results that are, and just fail to be, fixed-length: every second read kept, 100 bases of each
    spans = np.array([(10, 110) if i % 2 == 0 else (0, 0) for i in range(100)], np.uint64)
    fixed = dict(bases=special_bytes(rng, 100 * 150), offs=None, read_len=150, spans=spans, keep_empty=False)
    out["result_fixed"] = fixed
    out["result_whole_reads"] = dict(fixed, spans=np.array([(0, 150) if i % 3 else (150, 150) for i in range(100)], np.uint64))
    short = spans.copy()
    short[42] = (10, 109)
    out["result_just_not_fixed"] = dict(fixed, spans=short)
    out["result_one_sequence"] = dict(fixed, spans=np.array([(0, 150) if i == 7 else (0, 0) for i in range(100)], np.uint64))
    # three hundred three-byte sequences: more than the 63 a wave of the gather keeps in registers
    tiny = np.tile(np.array([[1, 4]], np.uint64), (300, 1))
    out["many_tiny"] = dict(bases=special_bytes(rng, 300 * 5), offs=None, read_len=5, spans=tiny, keep_empty=False)
    return out


# ---- bl_batch_select past the sizes of the cases above: the depth of the wave's search, the switch between its two lookups, runs of
# empty kept sequences, totals around a wave's bytes.  The two helpers are written from the prose of bl_select_core.hpp ("The gather is
# output-centric ..", "The wave's search"), not from the kernel.

def _wave_bytes():
    import os
    import re

    source = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "biolib_amd", "csrc", "bl_select_core.hpp")
    with open(source) as f:
        text = f.read()
    names = {}
    for name, expr in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*([^;]+);", text):
        names[name] = int(eval(expr, {"__builtins__": {}}, dict(names)))
    assert "WAVE_BYTES" in names, f"WAVE_BYTES not found in {source}"
    return names["WAVE_BYTES"]


WAVE_BYTES = _wave_bytes()  # output bytes of a wave of the gather
DEPTH_N_OUT = (1, 2, 63, 64, 65, 66, 4095, 4096, 4097, 4098, 262144, 262145, 262146)
EMPTY_RUNS = (64, 65, 66, 70, 130, 4097)


def search_depth(n_out):
    """steps of the 64-ary search over [0, n_out): every step narrows an interval of w entries to at most ceil(w / 64)"""
    depth, w = 0, int(n_out)
    while w > 1:
        w = (w + 63) // 64
        depth += 1
    return depth


def wave_inside(offsets):
    """per wave of the gather: the number of the 64 offsets after the wave's first sequence that are at or below its last byte.  The
    first sequence is the LAST one whose offset is <= the wave's first byte; entry n_out (the total) is the last offset there is.
    Below 64 the wave keeps its sequences in registers, at 64 it looks them up in memory."""
    offsets = np.asarray(offsets, np.uint64).astype(np.int64)
    n_out, total = len(offsets) - 1, int(offsets[-1])
    first = np.arange(0, total, WAVE_BYTES, dtype=np.int64)
    last = np.minimum(first + WAVE_BYTES - 1, total - 1)
    lo = np.searchsorted(offsets[:n_out], first, side="right") - 1
    upto = np.searchsorted(offsets, last, side="right")  # entries 0 .. upto - 1 are <= the last byte
    return np.clip(upto - (lo + 1), 0, 64)


def wave_paths(offsets):
    """(waves that keep their sequences in registers, waves that look them up in memory)"""
    inside = wave_inside(offsets)
    return int((inside < 64).sum()), int((inside == 64).sum())


def _ragged(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.uint64)


def _empty_runs_lengths():
    """result lengths, 0 = an empty kept sequence: a run at the result's start, runs whose shared offset is a wave's first byte, runs in
    the middle of a wave, a run behind the last byte; every length of EMPTY_RUNS occurs"""
    W = WAVE_BYTES
    out = [0] * 70 + [W - 100, 100]                      # 70 at byte 0 (the start, and wave 0's first byte); then up to byte W
    out += [0] * 65 + [500] + [0] * 64 + [300] + [0] * 66 + [200]  # 65 at byte W: wave 1's first byte; 64 and 66 inside wave 1
    out += [7] * 40 + [0] * 4097 + [33]                   # 4,097 in the middle of wave 1
    at = sum(out)
    out += [3 * W - at]                                   # pad onto a later wave boundary ..
    out += [0] * 130 + [W // 2] + [0] * 70 + [W // 2 + 11]  # .. 130 at wave 3's first byte, 70 in the middle of it
    out += [0] * 64                                       # behind the last byte
    assert at < 3 * W and sorted(set(_runs(out))) == sorted(EMPTY_RUNS)
    return out


def _runs(lengths):
    runs, n = [], 0
    for x in list(lengths) + [1]:
        if x == 0:
            n += 1
        elif n:
            runs.append(n)
            n = 0
    return runs


def scale_variants():
    """{name: dict(bases, offs | None, read_len, spans, keep_empty)} as variants()"""
    return _scale_variants()


def _memo(f):
    cache = []

    def g():
        if not cache:
            cache.append(f())
        return cache[0]
    return g


@_memo
def _scale_variants():
    rng = np.random.default_rng(20263)
    out = {}
    # depth_N: n_out = N fixed-length reads of 6 bases, spans (1, 1 + i % 6), empty ones kept: one sequence in six is empty
    for n in DEPTH_N_OUT:
        i = np.arange(n, dtype=np.uint64)
        spans = np.stack([np.ones(n, np.uint64), np.uint64(1) + i % np.uint64(6)], axis=1)
        out[f"depth_{n}"] = dict(bases=special_bytes(rng, 6 * n), offs=None, read_len=6 if n > 1 else 0, spans=spans, keep_empty=True)
    out[f"depth_{DEPTH_N_OUT[-1]}_dropped"] = dict(out[f"depth_{DEPTH_N_OUT[-1]}"], keep_empty=False)
    # switch: 62, 63 and 64 of a wave's 64 lane offsets at or below its last byte
    lengths = np.random.default_rng(5).integers(60, 70, 3000)
    whole = lambda n: np.tile(np.array([[0, U64]], np.uint64), (n, 1))
    out["switch"] = dict(bases=special_bytes(rng, int(lengths.sum())), offs=_ragged(lengths), read_len=0, spans=whole(3000), keep_empty=False)
    for first in (0, 1):  # 64-byte reads behind a first read of 0 bytes (63 in every full wave) and of 1 byte (64: the memory path)
        lengths = [first] + [64] * 300
        out[f"switch_first{first}"] = dict(bases=special_bytes(rng, sum(lengths)), offs=_ragged(lengths), read_len=0, spans=whole(301), keep_empty=True)
    # empty_runs: a source read of 3 bases with the span (1, 1) per empty sequence
    lengths = _empty_runs_lengths()
    src = [x if x else 3 for x in lengths]
    spans = np.array([(0, x) if x else (1, 1) for x in lengths], np.uint64)
    out["empty_runs"] = dict(bases=special_bytes(rng, sum(src)), offs=_ragged(src), read_len=0, spans=spans, keep_empty=True)
    # totals around a wave's bytes: from a single sequence and from 7-byte sequences (the last one cut)
    W = WAVE_BYTES
    for total in (W - 1, W, W + 1, 3 * W, 3 * W + 16):
        out[f"total_{total}_single"] = dict(bases=special_bytes(rng, total + 10), offs=None, read_len=0, spans=np.array([[5, 5 + total]], np.uint64), keep_empty=False)
        n = (total + 6) // 7
        spans = np.tile(np.array([[0, 7]], np.uint64), (n, 1))
        spans[-1, 1] = total - 7 * (n - 1)
        out[f"total_{total}_sevens"] = dict(bases=special_bytes(rng, 7 * n), offs=None, read_len=7, spans=spans, keep_empty=False)
    return out


def scale_self_check(name, v, m):
    """a scale variant holds what its name promises; m: the model's result"""
    offsets = m["offsets"]
    inside = wave_inside(offsets)
    if name.startswith("depth_"):
        n = int(name.split("_")[1])
        if name.endswith("_dropped"):
            assert m["n_seqs"] == n - (n + 5) // 6 and search_depth(m["n_seqs"]) == 3
        else:
            assert m["n_seqs"] == n and int((np.diff(offsets.astype(np.int64)) == 0).sum()) == (n + 5) // 6
    if name == "switch":
        assert {62, 63, 64} <= set(inside.tolist()), sorted(set(inside.tolist()))
    if name == "switch_first0":
        assert set(inside[:-1].tolist()) == {63}
    if name == "switch_first1":
        assert set(inside[:-1].tolist()) == {64} and len(inside) >= 4 and inside[-1] < 64
    if name == "empty_runs":
        lens = np.diff(offsets.astype(np.int64))
        assert sorted(set(_runs(lens))) == sorted(EMPTY_RUNS)
        assert lens[0] == 0 and lens[-1] == 0 and int(offsets[-65]) == m["n_bases"], "a run at the start and one behind the last byte"
        shared = 0
        for w in range(0, m["n_bases"], WAVE_BYTES):
            at = np.nonzero(offsets[:-1] == np.uint64(w))[0]
            if len(at) > 64:
                shared += 1
                holder = int(at[-1])  # the last sequence whose offset is the wave's first byte holds that byte
                assert lens[holder] > 0 and (lens[at[:-1]] == 0).all() and int(m["source_index"][holder]) == holder
        assert shared >= 3, "waves that start at an offset more than 64 sequences share"
        assert (inside == 64).any() and (inside < 64).any()
    if name.startswith("total_"):
        assert m["n_bases"] == int(name.split("_")[1])
    return inside


def scale_depths():
    return {n: search_depth(n) for n in DEPTH_N_OUT}


def variant_offsets(v):
    """the offsets the model cuts a variant's source by"""
    if v["offs"] is not None:
        return v["offs"]
    n = len(v["bases"])
    return fixed_offsets(n, v["read_len"]) if v["read_len"] else np.array([0, n], np.uint64)


def expected(v):
    m = select_model(v["bases"], variant_offsets(v), v["spans"], v["keep_empty"])
    return m


def wrong_offsets(offs, rng):
    """non-monotone and out of range: shuffled, some entries beyond any batch"""
    bad = np.array(offs, np.uint64)
    rng.shuffle(bad)
    bad[rng.integers(0, len(bad), 5)] = np.array([U64, 1 << 40, U64 - 15, 1 << 63, 0], np.uint64)
    return bad


def garbage_spans(n, rng):
    g = rng.integers(0, 1 << 63, (n, 2), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 2)).astype(np.uint64)
    small = rng.random(n) < 0.5
    g[small] = rng.integers(0, 6000, (int(small.sum()), 2)).astype(np.uint64)
    return g


# ---- bl_read_spans

def span_cases(k=31):
    """(lengths, records, stat, rules): reads whose records put weak_begin + k - 1 below, at and above L, weak_end at L, no weak k-mer,
    n_kmers = 0, solid fractions at exact equality, and stat words at both ends of a range"""
    rows = []  # (L, n_kmers, n_solid, weak_begin, weak_end, stat)
    for L in (0, 1, k - 1, k, k + 1, 100, 150, 151):
        nk = max(L - k + 1, 0)
        rows.append((L, nk, nk, U64, 0, 50))                                   # no weak k-mer
        rows.append((L, 0, 0, U64, 0, 50))                                     # no k-mer at all
        for wb in sorted({0, 1, max(L - k - 1, 0), max(L - k, 0), max(L - k + 1, 0), max(L - k + 2, 0), max(L - 1, 0), L // 2}):
            for we in sorted({wb + 1, L, (wb + L) // 2 + 1, max(L - k + 1, wb + 1)}):
                rows.append((L, nk, max(nk - 1, 0), wb, we, 50))
        rows.append((L, nk, nk // 2, L + 7, L + 9, 50))                        # garbage: a weak span behind the read
        rows.append((L, nk, nk // 2, U64 - 3, U64, 50))                        # garbage: weak_begin + k - 1 wraps
    for we in (100 - (20 + k - 1) - 1, 100 - (20 + k - 1), 100 - (20 + k - 1) + 1):  # "longer": the suffix one longer, a tie (PREFIX), one shorter
        rows.append((100, 100 - k + 1, 60, 20, we, 50))
    for nk, ns in ((10, 5), (10, 4), (10, 6), (3, 1), (3, 2), (0, 0), (2**32 - 1, 2**32 - 1), (2**32 - 1, 2**31)):  # fractions at equality
        rows.append((150, nk, ns, 40, 90, 50))
    for st in (0, 9, 10, 11, 19, 20, 21, 2**32 - 1):                          # stat bounds (10, 20)
        rows.append((150, 120, 100, 40, 90, st))
    rec = np.zeros(len(rows), RECORD)
    rec["n_kmers"], rec["n_solid"] = [r[1] for r in rows], [r[2] for r in rows]
    rec["n_found"], rec["min_count"], rec["max_count"], rec["sum_counts"] = rec["n_solid"], 1, 9, 1234
    rec["weak_begin"], rec["weak_end"] = np.array([r[3] for r in rows], np.uint64), np.array([r[4] for r in rows], np.uint64)
    lengths = np.array([r[0] for r in rows], np.int64)
    stat = np.array([r[5] for r in rows], np.uint32)
    rules = {f"{t}_k{kk}": rule(t, kk) for t in TRIM for kk in (k,)}
    rules.update(prefix_k1=rule("prefix", 1), longer_k64=rule("longer", 64), suffix_min_len_0=rule("suffix", k, min_len=0),
                 prefix_min_len_60=rule("prefix", k, min_len=60), min_kmers_1=rule("none", k, min_len=0, min_kmers=1),
                 solid_at_least_half=rule("none", k, min_len=0, solid_min=(1, 2)), solid_at_most_half=rule("none", k, min_len=0, solid_max=(1, 2)),
                 solid_band=rule("longer", k, solid_min=(1, 3), solid_max=(2, 3)), stat_10_20=rule("prefix", k, stat=(10, 20)),
                 stat_all=rule("prefix", k, stat=(0, 2**32 - 1)))
    return lengths, rec, stat, rules
