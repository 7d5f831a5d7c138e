"""Plain Python model of the 32-byte super-k-mer record (biolib_amd/csrc/bl_superkmer128_core.hpp) and of how bl_count_super_kmers128
cuts one bucket into rounds: the reference side of tests/test_gpu_superkmer128.py and tests/test_emu_superkmer128.py, itself checked
without a GPU in tests/test_superkmer128_model.py.

TEST INFRASTRUCTURE, nothing clever on purpose: bases are strings, k-mers are Python ints read in base 4 (up to 128 bits), the
canonical form is the minimum of a string and its reverse complement.  The table's limits are READ from the kernel sources
(limits()), so the directed cases built on them stay on their edges when a constant is retuned."""
import os
import re

import numpy as np

from superkmer_model import kmer_value, rounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, "biolib_amd", "csrc", "bl_superkmer128_core.hpp")
SOURCE = os.path.join(ROOT, "biolib_amd", "csrc", "bl_superkmer128.hip")

MAX_BASES = 122  # of one record
MAX_SIZE = 64    # k-mers of one record
_DIGITS = str.maketrans("ACGT", "0123")
M64 = (1 << 64) - 1
LOW12 = 0xFFF


# ----------------------------------------------------------------------------- the record

def _words(bases, mp, size):
    """four words from a string of ACGT (at most 122), mm_pos and size"""
    assert len(bases) <= MAX_BASES
    digits = bases.translate(_DIGITS).ljust(128, "0")
    w = [int(digits[32 * i:32 * i + 32], 4) for i in range(4)]
    assert w[3] & LOW12 == 0
    w[3] |= ((int(mp) & 63) << 6) | ((int(size) - 1) & 63)
    return w


def pack(seq, fp, sz, k, mp):
    """records of groups that lie inside the batch: uint64[n, 4]"""
    text = bytes(np.asarray(seq, np.uint8)).decode("latin1").upper().replace("U", "T")
    out = np.zeros((len(fp), 4), np.uint64)
    for g, (p, s, q) in enumerate(zip(np.asarray(fp).tolist(), np.asarray(sz).tolist(), np.asarray(mp).tolist())):
        bases = text[p:p + s + k - 1]
        assert len(bases) == s + k - 1 and set(bases) <= set("ACGT")
        out[g] = _words(bases, q, s)
    return out


def pack_clipped(seq, first_pos, sizes, k, mm_pos, origin=0):
    """What bl_pack_super_kmers128 promises for ANY position: the bases of the group that lie inside the batch [origin, origin +
    len(seq)), code 0 for those behind its end, no base at all for a group that starts in front of the origin or at / behind the end;
    mm_pos and size - 1 in bits 11..0 as given, always.  first_pos are the caller's 64-bit values."""
    text = bytes(np.asarray(seq, np.uint8)).decode("latin1").upper().replace("U", "T")
    n = len(text)
    out = np.zeros((len(first_pos), 4), np.uint64)
    for g, (fp, s, mp) in enumerate(zip(first_pos, sizes, mm_pos)):
        p = (int(fp) - int(origin)) & M64  # as the kernel sees it: unsigned
        bases = text[p:p + min(int(s) + k - 1, MAX_BASES)] if p < n else ""
        bases = "".join(ch if ch in "ACGT" else "A" for ch in bases)  # anything else packs code 0 (groups never hold such a base)
        out[g] = _words(bases, mp, s)
    return out


def records_from_bases(strings, k, mm_pos=0):
    """hand-built records: one per string of ACGT, size = len - k + 1 k-mers; mm_pos one value or one per record"""
    mps = [mm_pos] * len(strings) if np.isscalar(mm_pos) else list(mm_pos)
    assert len(mps) == len(strings)
    out = np.zeros((len(strings), 4), np.uint64)
    for g, (s, mp) in enumerate(zip(strings, mps)):
        size = len(s) - k + 1
        assert 1 <= size <= MAX_SIZE and len(s) <= MAX_BASES and set(s) <= set("ACGT") and 0 <= mp < 64, (s, k)
        out[g] = _words(s, mp, size)
    return out


def record_size(rec):
    return (int(rec[3]) & 63) + 1


def record_mm_pos(rec):
    return (int(rec[3]) >> 6) & 63


def record_bases(rec, k):
    """the size + k - 1 bases of one record as a string (bases the record cannot hold read as A, as the kernel reads zeros)"""
    n = record_size(rec) + k - 1
    whole = (int(rec[0]) << 192) | (int(rec[1]) << 128) | (int(rec[2]) << 64) | (int(rec[3]) & ~LOW12)
    return "".join("ACGT"[(whole >> (254 - 2 * i)) & 3] if i < 128 else "A" for i in range(n))


def expand_each(records, k, canonical):
    """per record: the list of its k-mers (Python ints), in order"""
    out = []
    for rec in np.asarray(records, np.uint64).reshape(-1, 4):
        s = record_bases(rec, k)
        out.append([kmer_value(s[j:j + k], canonical) for j in range(record_size(rec))])
    return out


def to_words(values):
    """Python ints -> uint64[n, 2] (low, high)"""
    out = np.zeros((len(values), 2), np.uint64)
    for i, v in enumerate(values):
        out[i] = (int(v) & M64, int(v) >> 64)
    return out


def from_words(arr):
    """uint64[n, 2] (low, high) -> list of Python ints"""
    a = np.asarray(arr).view(np.uint64).reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in a.tolist()]


def expand(records, k, canonical):
    """the k-mers of each record in order, record after record (list of Python ints)"""
    return [v for ks in expand_each(records, k, canonical) for v in ks]


def expected_counts(records, k, canonical):
    """dict: k-mer -> multiplicity"""
    out = {}
    for v in expand(records, k, canonical):
        out[v] = out.get(v, 0) + 1
    return out


def minimizer_of(rec, k, m, canonical):
    """the m-mer the counter buckets a record by: m bases at mm_pos of the first k-mer, canonical as the scan took it"""
    s = record_bases(rec, k) + "A" * 96  # (a hand-built mm_pos may point behind the record's bases: zeros there)
    mp = record_mm_pos(rec)
    return kmer_value(s[mp:mp + m], canonical)


def assert_bucketable(records, k, m, canonical):
    """The counter's precondition: every occurrence of a k-mer has the same minimizer (true of real super-k-mers)."""
    owner = {}
    for rec, ks in zip(np.asarray(records, np.uint64).reshape(-1, 4), expand_each(records, k, canonical)):
        mn = minimizer_of(rec, k, m, canonical)
        for v in ks:
            assert owner.setdefault(v, mn) == mn, "one k-mer under two minimizers: not a valid input of the counter"


def groups(seq, offsets, k, m, seed, canonical, hash64):
    """The super-k-mers of a batch by the plain rule (what bl_scan_super_kmers reports): a k-mer is k good bases inside one sequence; its
    minimizer occurrence is the leftmost smallest hash64(m-mer, seed) among its w = k - m + 1 m-mers; a group is a maximal run of
    consecutive k-mers with one occurrence.  Returns lists minimizers, first_pos, mm_pos, sizes, hashes."""
    text = bytes(np.asarray(seq, np.uint8)).decode("latin1").upper().replace("U", "T")
    w = k - m + 1
    mn, fp, mp, sz, hs = [], [], [], [], []
    for a, e in zip(np.asarray(offsets)[:-1].tolist(), np.asarray(offsets)[1:].tolist()):
        cur = None  # (occurrence position, first k-mer, size)
        hashes = {}

        def flush():
            if cur is not None:
                v = kmer_value(text[cur[0]:cur[0] + m], canonical)
                mn.append(v); fp.append(cur[1]); mp.append(cur[0] - cur[1]); sz.append(cur[2]); hs.append(hashes[cur[0]])

        for p in range(a, e - k + 1):
            if not set(text[p:p + k]) <= set("ACGT"):
                flush()
                cur = None
                continue
            for q in range(p, p + w):
                if q not in hashes:
                    hashes[q] = hash64(kmer_value(text[q:q + m], canonical), seed)
            occ = min(range(p, p + w), key=lambda q: (hashes[q], q))
            if cur is not None and cur[0] == occ and cur[1] + cur[2] == p:
                cur = (occ, cur[1], cur[2] + 1)
            else:
                flush()
                cur = (occ, p, 1)
        flush()
    return mn, fp, mp, sz, hs


# ----------------------------------------------------------------------------- the counter's limits and rounds

_CORE_PATTERNS = {
    "CT_SLOTS": r"constexpr\s+int\s+CT128_SLOTS\s*=\s*(\d+)\s*;",
    "CT_CAP": r"constexpr\s+int\s+CT128_CAP\s*=\s*(\d+)\s*;",
    "CT_FULL": r"constexpr\s+int\s+CT128_FULL\s*=\s*(\d+)\s*;",
    "CT_RECS": r"constexpr\s+int\s+CT128_RECS\s*=\s*(\d+)\s*;",
    "CT_MAXREC": r"constexpr\s+int\s+CT128_MAXREC\s*=\s*(\d+)\s*;",
    "SLOT_MUL_HI": r"table128_slot\(uint64_t lo, uint64_t hi\)\s*\{\s*return\s*\(uint32_t\)\(\(\(lo \^ \(hi \* (0x[0-9A-Fa-f]+)ULL\)\)",
    "SLOT_MUL": r"table128_slot\(uint64_t lo, uint64_t hi\)\s*\{[^}]*\)\)\s*\*\s*(0x[0-9A-Fa-f]+)ULL\)\s*>>",
    "SLOT_BITS": r"table128_slot\(uint64_t lo, uint64_t hi\)\s*\{[^}]*>>\s*\(64\s*-\s*(\d+)\)\)",
}
_SOURCE_PATTERNS = {"BUCKET_RECS": r"want_buckets\s*=\s*\(n_groups\s*\+\s*\d+\)\s*/\s*(\d+)\s*;"}


def limits(core=CORE, source=SOURCE):
    """the constants of the counter, read from the kernel sources; every one must be found"""
    out = {}
    for path, pats in ((core, _CORE_PATTERNS), (source, _SOURCE_PATTERNS)):
        with open(path) as f:
            text = f.read()
        for name, pat in pats.items():
            found = re.findall(pat, text)
            assert len(found) == 1, f"{name}: {len(found)} matches in {path}"
            out[name] = int(found[0], 0)
        if pats is _SOURCE_PATTERNS:
            rounding = re.findall(r"want_buckets\s*=\s*\(n_groups\s*\+\s*(\d+)\)\s*/\s*\d+\s*;", text)
            assert len(rounding) == 1 and int(rounding[0]) == out["BUCKET_RECS"] - 1, "bucket count is not ceil(n / BUCKET_RECS)"
    assert 1 << out["SLOT_BITS"] == out["CT_SLOTS"], "table128_slot does not span the table"
    return out


def n_buckets(n_records, lim=None):
    lim = lim or limits()
    return max(1, -(-n_records // lim["BUCKET_RECS"]))


def table_slot(key, lim=None):
    lim = lim or limits()
    lo, hi = int(key) & M64, int(key) >> 64
    return (((lo ^ ((hi * lim["SLOT_MUL_HI"]) & M64)) * lim["SLOT_MUL"]) & M64) >> (64 - lim["SLOT_BITS"])


def table_slots_np(lo, hi, lim=None):
    lim = lim or limits()
    with np.errstate(over="ignore"):
        x = np.asarray(lo, np.uint64) ^ (np.asarray(hi, np.uint64) * np.uint64(lim["SLOT_MUL_HI"]))
        return ((x * np.uint64(lim["SLOT_MUL"])) >> np.uint64(64 - lim["SLOT_BITS"])).astype(np.int64)


def bucket_fate(records, k, canonical, lim=None):
    """What the counter does with ONE bucket holding `records` in this order: dict(path = "table" | "fallback", rounds, totals, held =
    distinct k-mers in the table BEFORE each round, distinct).  The fallback is taken by more than CT_MAXREC records, or when held +
    total of a round exceeds CT_FULL."""
    lim = lim or limits()
    each = expand_each(records, k, canonical)
    sizes = [len(ks) for ks in each]
    cut = rounds(sizes, lim["CT_CAP"], lim["CT_RECS"])
    seen, held, totals, at = set(), [], [], 0
    path = "fallback" if len(sizes) > lim["CT_MAXREC"] else "table"
    for n in cut:
        total = sum(sizes[at:at + n])
        held.append(len(seen))
        totals.append(total)
        if len(seen) + total > lim["CT_FULL"]:
            path = "fallback"
        for ks in each[at:at + n]:
            seen.update(ks)
        at += n
    return dict(path=path, rounds=cut, totals=totals, held=held, distinct=len(seen))


# ----------------------------------------------------------------------------- directed buckets, derived from limits()
# Every case is ONE bucket: all its records carry the same m-mer at mm_pos 0, so they share a bucket whatever the bucket hash does,
# and the stable sort keeps their order: rounds() predicts what the kernel does with them.  check_case() asserts every claim.

CASE_M, CASE_MMER, CASE_K = 5, "GATTC", 40


def _random_records(rng, sizes, k, mmer=CASE_MMER):
    strings = [mmer + "".join("ACGT"[c] for c in rng.integers(0, 4, s + k - 1 - len(mmer))) for s in sizes]
    return records_from_bases(strings, k, 0)


def _case(name, k, records, canonical=False, **claims):
    return dict(name=name, k=k, m=CASE_M, canonical=canonical, records=np.ascontiguousarray(records, np.uint64), **claims)


def _fill(total, s=MAX_SIZE):
    return [s] * (total // s) + ([total % s] if total % s else [])


def round_cases(lim=None):
    """k = 40 and sizes up to 64 (103 bases): one round against two, at each of the two limits of a round"""
    lim = lim or limits()
    cap, nrec, k, S = lim["CT_CAP"], lim["CT_RECS"], CASE_K, MAX_SIZE
    rng = np.random.default_rng(4001)
    nS, s_lo = cap // S, cap // nrec
    first_hi = cap // (s_lo + 1)
    assert cap % S and first_hi < nrec and (nrec - first_hi) * (s_lo + 1) <= cap and nrec + 1 <= cap
    shapes = [
        ("cap_floor", [S] * nS, dict(rounds=[nS])),
        ("cap_floor_plus_1", [S] * (nS + 1), dict(rounds=[nS, 1])),
        ("recs_limit", [1] * nrec, dict(rounds=[nrec])),
        ("recs_limit_plus_1", [1] * (nrec + 1), dict(rounds=[nrec, 1])),
        ("recs_bind", [s_lo] * nrec, dict(rounds=[nrec])),
        ("kmers_bind", [s_lo + 1] * nrec, dict(rounds=[first_hi, nrec - first_hi])),
        ("total_eq_cap", _fill(cap), dict(rounds=[nS + 1], totals=[cap])),
        ("total_eq_cap_plus_1", _fill(cap)[:-1] + [cap % S + 1], dict(rounds=[nS, 1], totals=[S * nS, cap % S + 1])),
    ]
    return [_case(name, k, _random_records(rng, sizes, k), path="table", distinct=sum(sizes), **claims) for name, sizes, claims in shapes]


def full_cases(lim=None):
    """held + total of the last round exactly CT_FULL (the table keeps the bucket) and one more (the fallback takes it), over two rounds
    and over several; and a bucket of many rounds whose few distinct k-mers never come near CT_FULL"""
    lim = lim or limits()
    cap, nrec, full, k, S = lim["CT_CAP"], lim["CT_RECS"], lim["CT_FULL"], CASE_K, MAX_SIZE
    rng = np.random.default_rng(4002)
    nS = cap // S
    rest = full - S * nS
    assert S <= rest < cap and cap % S, "the second round must open with a record that did not fit the first"
    ones = 2
    while full - nrec * ones > cap:
        ones += 1
    assert full - nrec * ones >= S
    out = []
    for extra, path in ((0, "table"), (1, "fallback")):
        sizes = [S] * nS + _fill(rest + extra)
        out.append(_case(f"full_2_rounds_{path}", k, _random_records(rng, sizes, k), path=path, edge=full + extra, distinct=sum(sizes), n_rounds=2))
        sizes = [1] * (nrec * ones) + _fill(full - nrec * ones + extra)
        out.append(_case(f"full_{ones + 1}_rounds_{path}", k, _random_records(rng, sizes, k), path=path, edge=full + extra, distinct=sum(sizes), n_rounds=ones + 1))
        can = _random_records(rng, [S] * nS + _fill(rest + extra), k)
        out.append(_case(f"full_2_rounds_canonical_{path}", k, can, canonical=True, path=path, edge=full + extra, distinct=S * nS + rest + extra, n_rounds=2))
    few = (full - S * nS) // S
    assert few >= 2
    pool = _random_records(rng, [S] * few, k)
    order = np.concatenate([np.arange(few), rng.integers(0, few, 24 * nS - few)])
    out.append(_case("many_rounds_of_repeats", k, pool[order], path="table", distinct=S * few, n_rounds=24, edge=S * few + S * nS))
    return out


def count_width_cases(lim=None):
    """One k-mer counted up to the edge of its 16 bits, its neighbour in the other half of the same 32-bit count word untouched: a
    homopolymer record of k + 63 bases holds its k-mer 64 times; CT_MAXREC of them come to 64 CT_MAXREC <= 65535."""
    lim = lim or limits()
    top = lim["CT_MAXREC"]
    assert MAX_SIZE * top <= 0xFFFF < MAX_SIZE * (top + 1)
    rng = np.random.default_rng(4003)
    out = []
    for k, base in ((40, "A"), (64 - 5, "T"), (33, "C")):
        hot_slot = table_slot(kmer_value(base * k, False), lim)
        neighbour = None
        for _ in range(200 * lim["CT_SLOTS"]):
            s = base * CASE_M + "".join("ACGT"[c] for c in rng.integers(0, 4, k - CASE_M))
            if table_slot(kmer_value(s, False), lim) == hot_slot ^ 1:
                neighbour = s
                break
        assert neighbour is not None and neighbour != base * k
        hot = records_from_bases([base * (k + MAX_SIZE - 1)], k, 0)
        nb = records_from_bases([neighbour], k, 0)
        tag = f"k{k}_poly{base}"
        slots = dict(slots={hot_slot: 1, hot_slot ^ 1: 1}, mmer=base * CASE_M)
        only = dict(slots={hot_slot: 1}, mmer=base * CASE_M)
        out.append(_case(f"{tag}_max_alone", k, np.repeat(hot, top, 0), path="table", distinct=1, top_count=MAX_SIZE * top, **only))
        mixed = np.repeat(hot, top, 0)
        mixed[[0, top // 2, top - 1]] = nb[0]
        out.append(_case(f"{tag}_max_with_neighbour", k, mixed, path="table", distinct=2, top_count=MAX_SIZE * (top - 3), other_count=3, **slots))
        out.append(_case(f"{tag}_one_record_more", k, np.repeat(hot, top + 1, 0), path="fallback", distinct=1, top_count=MAX_SIZE * (top + 1), **only))
        out.append(_case(f"{tag}_neighbour_makes_it_one_more", k, np.concatenate([np.repeat(hot, top, 0), nb]), path="fallback", distinct=2,
                         top_count=MAX_SIZE * top, other_count=1, **slots))
    return out


_POOLS = {}


def _probe_pool(canonical, lim):
    """1.5 * 10^6 seeded 40-mers that open with the m-mer (as high, low words), and the table slot of each one's (canonical) value"""
    key = (canonical, lim["SLOT_MUL"], lim["SLOT_MUL_HI"], lim["SLOT_BITS"])
    if key not in _POOLS:
        k = CASE_K
        rng = np.random.default_rng(4100 + int(canonical))
        n = 1_500_000
        prefix = kmer_value(CASE_MMER, False) << (2 * (k - CASE_M) - 64)  # the m-mer on top of the high word
        hi = np.uint64(prefix) | rng.integers(0, 1 << (2 * k - 64 - 2 * CASE_M), n, dtype=np.uint64)
        lo = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)
        vlo, vhi = lo, hi
        if canonical:  # (bit tricks as a search aid only: check_case() takes the canonical form of what was found the plain way)
            rlo, rhi = np.zeros_like(lo), np.zeros_like(hi)
            two, three = np.uint64(2), np.uint64(3)
            for i in range(k):
                c = (lo >> np.uint64(2 * i)) & three if i < 32 else (hi >> np.uint64(2 * (i - 32))) & three
                rhi = (rhi << two) | (rlo >> np.uint64(62))
                rlo = (rlo << two) | (three - c)
            less = (rhi < hi) | ((rhi == hi) & (rlo < lo))
            vlo, vhi = np.where(less, rlo, lo), np.where(less, rhi, hi)
        _POOLS[key] = (lo, hi, table_slots_np(vlo, vhi, lim))
    return _POOLS[key]


def _kmer_string(v, k):
    return "".join("ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def probe_cases(lim=None):
    """k = 40, m = 5, size 1: keys searched for their table slot — the longest chain the table can hold, wrapping from the last slot to
    slot 0; a cluster over the last four slots; duplicates inside the cluster; the same with canonical k-mers"""
    lim = lim or limits()
    full, last, k = lim["CT_FULL"], lim["CT_SLOTS"] - 1, CASE_K
    out = []
    for canonical in (False, True):
        lo, hi, slots = _probe_pool(canonical, lim)
        rng = np.random.default_rng(4102 + int(canonical))
        tag = "canonical_" if canonical else ""

        def take(slot, n):
            idx = np.nonzero(slots == slot)[0][:n]
            assert len(idx) == n, f"only {len(idx)} of {n} keys with slot {slot} in the pool"
            return [int(lo[i]) | (int(hi[i]) << 64) for i in idx]

        recs = lambda keys: records_from_bases([_kmer_string(v, k) for v in keys], k, 0)
        chain = take(last, full)
        out.append(_case(f"{tag}chain_of_CT_FULL_wraps", k, recs(chain), canonical=canonical, path="table", distinct=full, edge=full, slots={last: full}))
        per = full // 8
        cluster = [v for s in range(last - 3, last + 1) for v in take(s, per)]
        cluster = [cluster[i] for i in rng.permutation(len(cluster))]
        out.append(_case(f"{tag}cluster_on_last_slots", k, recs(cluster), canonical=canonical, path="table", distinct=4 * per,
                         slots={s: per for s in range(last - 3, last + 1)}))
        per = full // 16
        keys = [v for s in range(last - 3, last + 1) for v in take(s, per)]
        dup = [v for i, v in enumerate(keys) for _ in range(1 + i % 5)]
        dup = [dup[i] for i in rng.permutation(len(dup))]
        out.append(_case(f"{tag}cluster_with_duplicates", k, recs(dup), canonical=canonical, path="table", distinct=4 * per, top_count=5,
                         slots={s: per for s in range(last - 3, last + 1)}))
    return out


def all_count_cases(lim=None):
    lim = lim or limits()
    return round_cases(lim) + full_cases(lim) + count_width_cases(lim) + probe_cases(lim)


def check_case(case, lim=None):
    """assert, on the model alone, that a directed case sits where it says; returns bucket_fate() of it"""
    lim = lim or limits()
    recs, k, m, canonical, name = case["records"], case["k"], case["m"], case["canonical"], case["name"]
    mmer = case.get("mmer", CASE_MMER)
    for rec in list(recs[:: max(1, len(recs) // 64)]) + list(recs[-3:]):
        assert record_mm_pos(rec) == 0 and record_bases(rec, k)[:m] == mmer, name  # one minimizer: one bucket
    fate = bucket_fate(recs, k, canonical, lim)
    assert fate["path"] == case["path"], (name, fate["path"], fate["rounds"][:4], fate["held"][-3:], fate["totals"][-3:])
    assert fate["distinct"] == case["distinct"], (name, fate["distinct"])
    if "rounds" in case:
        assert fate["rounds"] == case["rounds"], (name, fate["rounds"])
    if "totals" in case:
        assert fate["totals"] == case["totals"], (name, fate["totals"])
    if "n_rounds" in case:
        assert len(fate["rounds"]) == case["n_rounds"], (name, fate["rounds"])
    if "edge" in case:
        assert max(h + t for h, t in zip(fate["held"], fate["totals"])) == case["edge"], (name, fate["held"], fate["totals"])
    if case["path"] == "table":
        assert len(recs) <= lim["CT_MAXREC"] and fate["distinct"] <= lim["CT_FULL"] < lim["CT_SLOTS"], name
    counts = expected_counts(recs, k, canonical)
    if "slots" in case:
        got = {}
        for v in counts:
            got[table_slot(v, lim)] = got.get(table_slot(v, lim), 0) + 1
        assert got == case["slots"], (name, got)
    if "top_count" in case:
        assert max(counts.values()) == case["top_count"], (name, max(counts.values()))
        if case["path"] == "table":
            assert case["top_count"] <= 0xFFFF, name
    if "other_count" in case:
        assert min(counts.values()) == case["other_count"] and len(counts) == 2, name
    return fate
