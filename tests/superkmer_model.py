"""Plain numpy / Python model of the 16-byte super-k-mer record (biolib_amd/csrc/bl_superkmer.hip) and of how
bl_count_super_kmers cuts one bucket into rounds: the reference side of tests/test_gpu_superkmer_edges.py, itself checked
against the C oracle without a GPU in tests/test_superkmer_model.py.

Nothing here is clever on purpose: bases are strings, k-mers are Python ints read in base 4, the canonical form is the
minimum of a string and its reverse complement.  The table's limits are READ from the kernel source (limits()), so the
directed cases built on them stay on their edges when a constant is retuned."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "biolib_amd", "csrc", "bl_superkmer.hip")

MAX_BASES = 59  # of one record
_DIGITS = str.maketrans("ACGT", "0123")
_COMPLEMENT = str.maketrans("ACGT", "TGCA")
M64 = (1 << 64) - 1


# ----------------------------------------------------------------------------- the record

def pack(seq, fp, sz, k, mp=None):
    """numpy restatement of the 16-byte packed super-k-mer record"""
    code = np.zeros(256, np.uint64)
    for ch, c in zip(b"ACGTUacgtu", (0, 1, 2, 3, 3, 0, 1, 2, 3, 3)):
        code[ch] = c
    out = np.zeros((len(fp), 2), np.uint64)
    for g, (p, s) in enumerate(zip(fp.tolist(), sz.tolist())):
        nb = s + k - 1
        c = code[seq[p:p + nb]]
        hi = 0
        for i in range(min(nb, 32)):
            hi |= int(c[i]) << (62 - 2 * i)
        lo = (s - 1) | ((int(mp[g]) if mp is not None else 0) << 5)
        for i in range(32, nb):
            lo |= int(c[i]) << (62 - 2 * (i - 32))
        out[g] = (hi, lo)
    return out


def pack_clipped(seq, first_pos, sizes, k, mm_pos, origin=0):
    """What bl_pack_super_kmers promises for ANY position (include/biolib_amd.h): the bases of the group that lie inside the
    batch [origin, origin + len(seq)), code 0 for those behind its end, no base at all (all base bits zero) for a group
    that starts in front of the origin or at / behind the end; mm_pos and size - 1 in bits 9..0 as given, always.
    first_pos are the caller's 64-bit values (a position in front of origin 0 is a wrapped one)."""
    text = bytes(np.asarray(seq, np.uint8)).decode("latin1").upper().replace("U", "T")
    n = len(text)
    out = np.zeros((len(first_pos), 2), np.uint64)
    for g, (fp, s, mp) in enumerate(zip(first_pos, sizes, mm_pos)):
        p = (int(fp) - int(origin)) & M64  # as the kernel sees it: unsigned
        bases = text[p:p + int(s) + k - 1] if p < n else ""
        hi = lo = 0
        for i, ch in enumerate(bases):
            c = "ACGT".find(ch)
            c = 0 if c < 0 else c
            if i < 32:
                hi |= c << (62 - 2 * i)
            else:
                lo |= c << (62 - 2 * (i - 32))
        out[g] = (hi, lo | ((int(mp) & 31) << 5) | ((int(s) - 1) & 31))
    return out


def records_from_bases(strings, k, mm_pos=0):
    """hand-built records: one per string of ACGT, size = len - k + 1 k-mers; mm_pos one value or one per record"""
    mps = [mm_pos] * len(strings) if np.isscalar(mm_pos) else list(mm_pos)
    assert len(mps) == len(strings)
    out = np.zeros((len(strings), 2), np.uint64)
    for g, (s, mp) in enumerate(zip(strings, mps)):
        size = len(s) - k + 1
        assert 1 <= size <= 32 and len(s) <= MAX_BASES and set(s) <= set("ACGT"), (s, k)
        assert 0 <= mp < 32
        digits = s.translate(_DIGITS)
        hi = int(digits[:32].ljust(32, "0"), 4)
        lo = int(digits[32:].ljust(32, "0"), 4) if len(s) > 32 else 0
        assert lo & 0x3FF == 0
        out[g] = (hi, lo | (int(mp) << 5) | (size - 1))
    return out


def record_size(rec):
    return (int(rec[1]) & 31) + 1


def record_mm_pos(rec):
    return (int(rec[1]) >> 5) & 31


def record_bases(rec, k):
    """the size + k - 1 bases of one record as a string"""
    n = record_size(rec) + k - 1
    both = (int(rec[0]) << 64) | (int(rec[1]) & ~0x3FF)
    return "".join("ACGT"[(both >> (126 - 2 * i)) & 3] for i in range(n))


def kmer_value(s, canonical):
    """a k-mer string as its 2-bit number (first base most significant); canonical: the smaller of it and its reverse complement"""
    v = int(s.translate(_DIGITS), 4)
    if canonical:
        v = min(v, int(s[::-1].translate(_COMPLEMENT).translate(_DIGITS), 4))
    return v


def expand_each(records, k, canonical):
    """per record: the list of its k-mers (Python ints), in order"""
    out = []
    for rec in np.asarray(records, np.uint64).reshape(-1, 2):
        s = record_bases(rec, k)
        out.append([kmer_value(s[j:j + k], canonical) for j in range(record_size(rec))])
    return out


def expand(records, k, canonical):
    """the k-mers of each record in order, record after record (uint64)"""
    flat = [v for ks in expand_each(records, k, canonical) for v in ks]
    return np.array(flat, dtype=np.uint64) if flat else np.zeros(0, np.uint64)


def expected_counts(records, k, canonical):
    """(distinct k-mers ascending, multiplicities)"""
    u, c = np.unique(expand(records, k, canonical), return_counts=True)
    return u, c.astype(np.int64)


def minimizer_of(rec, k, m, canonical):
    """the m-mer the counter buckets a record by: m bases at mm_pos of the first k-mer, canonical as the scan took it"""
    s = record_bases(rec, k)
    mp = record_mm_pos(rec)
    assert mp + m <= len(s)
    return kmer_value(s[mp:mp + m], canonical)


def assert_bucketable(records, k, m, canonical):
    """The counter's precondition: every occurrence of a k-mer has the same minimizer, so that all of them meet in one bucket
    (true of real super-k-mers; hand-built records must be checked)."""
    owner = {}
    for rec, ks in zip(np.asarray(records, np.uint64).reshape(-1, 2), expand_each(records, k, canonical)):
        mn = minimizer_of(rec, k, m, canonical)
        for v in ks:
            assert owner.setdefault(v, mn) == mn, "one k-mer under two minimizers: not a valid input of the counter"


# ----------------------------------------------------------------------------- the counter's limits and rounds

_PATTERNS = {
    "CT_SLOTS": r"constexpr\s+int\s+CT_SLOTS\s*=\s*(\d+)\s*;",
    "CT_CAP": r"constexpr\s+int\s+CT_CAP\s*=\s*(\d+)\s*;",
    "CT_FULL": r"constexpr\s+int\s+CT_FULL\s*=\s*(\d+)\s*;",
    "CT_RECS": r"constexpr\s+int\s+CT_RECS\s*=\s*(\d+)\s*;",
    "CT_MAXREC": r"constexpr\s+int\s+CT_MAXREC\s*=\s*(\d+)\s*;",
    "CT_CHUNK": r"constexpr\s+unsigned\s+int\s+CT_CHUNK\s*=\s*(\d+)\s*;",
    "SLOT_MUL": r"table_slot\s*\(\s*unsigned long long key\s*\)\s*\{\s*return\s*\(uint32_t\)\s*\(\(key\s*\*\s*(0x[0-9A-Fa-f]+)ULL\)\s*>>\s*\(64\s*-\s*\d+\)\)",
    "SLOT_BITS": r"table_slot\s*\(\s*unsigned long long key\s*\)\s*\{\s*return\s*\(uint32_t\)\s*\(\(key\s*\*\s*0x[0-9A-Fa-f]+ULL\)\s*>>\s*\(64\s*-\s*(\d+)\)\)",
    "BUCKET_RECS": r"want_buckets\s*=\s*\(n_groups\s*\+\s*\d+\)\s*/\s*(\d+)\s*;",
}


def limits(source=SOURCE):
    """the constants of the counter, read from the kernel source; every one must be found"""
    with open(source) as f:
        text = f.read()
    out = {}
    for name, pat in _PATTERNS.items():
        found = re.findall(pat, text)
        assert len(found) == 1, f"{name}: {len(found)} matches in {source}"
        out[name] = int(found[0], 0)
    assert 1 << out["SLOT_BITS"] == out["CT_SLOTS"], "table_slot does not span the table"
    rounding = re.findall(r"want_buckets\s*=\s*\(n_groups\s*\+\s*(\d+)\)\s*/\s*\d+\s*;", text)
    assert len(rounding) == 1 and int(rounding[0]) == out["BUCKET_RECS"] - 1, "bucket count is not ceil(n / BUCKET_RECS)"
    return out


def n_buckets(n_records, lim=None):
    lim = lim or limits()
    return max(1, -(-n_records // lim["BUCKET_RECS"]))


def table_slot(key, lim=None):
    lim = lim or limits()
    return ((int(key) * lim["SLOT_MUL"]) & M64) >> (64 - lim["SLOT_BITS"])


def table_slots_np(keys, lim=None):
    """table_slot of a uint64 array"""
    lim = lim or limits()
    with np.errstate(over="ignore"):
        return ((np.asarray(keys, np.uint64) * np.uint64(lim["SLOT_MUL"])) >> np.uint64(64 - lim["SLOT_BITS"])).astype(np.int64)


def rounds(sizes, ct_cap, ct_recs):
    """How the counter cuts one bucket's records (their sizes, in bucket order) into rounds: a round is the longest prefix of
    at most ct_recs records whose sizes sum to at most ct_cap.  Returns the number of records of every round."""
    sizes = [int(s) for s in sizes]
    assert all(1 <= s <= ct_cap for s in sizes)
    out, at = [], 0
    while at < len(sizes):
        take = total = 0
        while at + take < len(sizes) and take < ct_recs and total + sizes[at + take] <= ct_cap:
            total += sizes[at + take]
            take += 1
        out.append(take)
        at += take
    return out


def bucket_fate(records, k, canonical, lim=None):
    """What the counter does with ONE bucket holding `records` in this order: dict(path = "table" | "fallback", rounds = records
    per round, totals = k-mers per round, held = distinct k-mers in the table BEFORE each round, distinct = of the bucket).
    The fallback is taken by more than CT_MAXREC records, or when held + total of a round exceeds CT_FULL."""
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
# Every case is ONE bucket: all its records carry the same m-mer at mm_pos, so they share a bucket whatever the bucket hash
# does (the other ceil(R / BUCKET_RECS) - 1 buckets of the call stay empty), and the stable sort keeps their order: rounds()
# predicts what the kernel does with them.  A case states where it sits ("path", "rounds", "totals", "edge" = the largest
# held + total any round reaches, "distinct", "slots"); check_case() asserts every statement on the model.

CASE_M, CASE_MMER = 5, "GATTC"


def _random_records(rng, sizes, k, mmer=CASE_MMER):
    """one record per size: the m-mer first (mm_pos 0), random bases behind it"""
    strings = [mmer + "".join("ACGT"[c] for c in rng.integers(0, 4, s + k - 1 - len(mmer))) for s in sizes]
    return records_from_bases(strings, k, 0)


def _case(name, k, records, canonical=False, **claims):
    return dict(name=name, k=k, m=CASE_M, canonical=canonical, records=np.ascontiguousarray(records, np.uint64), **claims)


def _fill(total):
    """record sizes that sum to `total`: 32s and one remainder"""
    return [32] * (total // 32) + ([total % 32] if total % 32 else [])


def round_cases(lim=None):
    """k = 28 and sizes up to 32 (59 bases, the widest record): one round against two, at each of the two limits of a round"""
    lim = lim or limits()
    cap, nrec, k = lim["CT_CAP"], lim["CT_RECS"], 28
    rng = np.random.default_rng(2801)
    n32, s_lo = cap // 32, cap // nrec
    first_hi = cap // (s_lo + 1)  # records of size s_lo + 1 that fit one round: fewer than CT_RECS
    assert cap % 32 and first_hi < nrec and (nrec - first_hi) * (s_lo + 1) <= cap and nrec + 1 <= cap
    shapes = [
        ("cap_floor", [32] * n32, dict(rounds=[n32])),
        ("cap_floor_plus_1", [32] * (n32 + 1), dict(rounds=[n32, 1])),
        ("recs_limit", [1] * nrec, dict(rounds=[nrec])),
        ("recs_limit_plus_1", [1] * (nrec + 1), dict(rounds=[nrec, 1])),
        ("recs_bind", [s_lo] * nrec, dict(rounds=[nrec])),
        ("kmers_bind", [s_lo + 1] * nrec, dict(rounds=[first_hi, nrec - first_hi])),
        ("total_eq_cap", _fill(cap), dict(rounds=[n32 + 1], totals=[cap])),
        ("total_eq_cap_plus_1", _fill(cap)[:-1] + [cap % 32 + 1], dict(rounds=[n32, 1], totals=[32 * n32, cap % 32 + 1])),
    ]
    return [_case(name, k, _random_records(rng, sizes, k), path="table", distinct=sum(sizes), **claims) for name, sizes, claims in shapes]


def full_cases(lim=None):
    """held + total of the last round exactly CT_FULL (the table keeps the bucket) and one more (the fallback takes it), over two
    rounds and over three or more; and a bucket of many rounds whose few distinct k-mers never come near CT_FULL"""
    lim = lim or limits()
    cap, nrec, full, k = lim["CT_CAP"], lim["CT_RECS"], lim["CT_FULL"], 28
    rng = np.random.default_rng(2802)
    n32 = cap // 32
    rest = full - 32 * n32  # what the second round may bring
    assert 32 <= rest < cap and cap % 32, "the second round must open with a record that did not fit the first"
    ones = 2  # rounds of CT_RECS records of size 1 in front of the last round
    while full - nrec * ones > cap:
        ones += 1
    assert full - nrec * ones >= 32
    out = []
    for extra, path in ((0, "table"), (1, "fallback")):
        sizes = [32] * n32 + _fill(rest + extra)
        out.append(_case(f"full_2_rounds_{path}", k, _random_records(rng, sizes, k), path=path, edge=full + extra, distinct=sum(sizes), n_rounds=2))
        sizes = [1] * (nrec * ones) + _fill(full - nrec * ones + extra)
        out.append(_case(f"full_{ones + 1}_rounds_{path}", k, _random_records(rng, sizes, k), path=path, edge=full + extra, distinct=sum(sizes), n_rounds=ones + 1))
        can = _random_records(rng, [32] * n32 + _fill(rest + extra), k)
        out.append(_case(f"full_2_rounds_canonical_{path}", k, can, canonical=True, path=path, edge=full + extra, distinct=32 * n32 + rest + extra, n_rounds=2))
    few = (full - 32 * n32) // 32  # distinct records of size 32 that leave room for a whole round of new k-mers
    assert few >= 2
    pool = _random_records(rng, [32] * few, k)
    order = rng.integers(0, few, 24 * n32)
    out.append(_case("many_rounds_of_repeats", k, pool[order], path="table", distinct=32 * few, n_rounds=24, edge=32 * few + 32 * n32))
    return out


def sixteen_bit_cases(lim=None):
    """One k-mer counted up to the edge of its 16 bits, its neighbour in the other half of the same 32-bit count word untouched.
    A k-mer that comes 32 times in one record is a homopolymer; those of k = 28 have even slots (low half), poly-C and poly-T
    of k = 27 odd ones (high half) — asserted here, from the multiplier limits() read."""
    lim = lim or limits()
    top = lim["CT_MAXREC"]
    rng = np.random.default_rng(2803)
    out = []
    for k, base, half in ((28, "A", 0), (28, "T", 0), (27, "C", 1), (27, "T", 1)):
        hot_slot = table_slot(kmer_value(base * k, False), lim)
        assert hot_slot & 1 == half, (k, base, hot_slot)
        neighbour = None
        for _ in range(200 * lim["CT_SLOTS"]):
            s = base * CASE_M + "".join("ACGT"[c] for c in rng.integers(0, 4, k - CASE_M))
            if table_slot(kmer_value(s, False), lim) == hot_slot ^ 1:
                neighbour = s
                break
        assert neighbour is not None and neighbour != base * k
        hot = records_from_bases([base * (k + 31)], k, 0)
        nb = records_from_bases([neighbour], k, 0)
        tag = f"k{k}_poly{base}"
        slots = dict(slots={hot_slot: 1, hot_slot ^ 1: 1}, mmer=base * CASE_M)  # with the neighbour
        only = dict(slots={hot_slot: 1}, mmer=base * CASE_M)
        out.append(_case(f"{tag}_max_alone", k, np.repeat(hot, top, 0), path="table", distinct=1, top_count=32 * top, **only))
        mixed = np.repeat(hot, top, 0)
        mixed[[0, top // 2, top - 1]] = nb[0]
        out.append(_case(f"{tag}_max_with_neighbour", k, mixed, path="table", distinct=2, top_count=32 * (top - 3), other_count=3, **slots))
        out.append(_case(f"{tag}_one_record_more", k, np.repeat(hot, top + 1, 0), path="fallback", distinct=1, top_count=32 * top + 32, **only))
        out.append(_case(f"{tag}_neighbour_makes_it_one_more", k, np.concatenate([np.repeat(hot, top, 0), nb]), path="fallback", distinct=2,
                         top_count=32 * top, other_count=1, **slots))
    return out


_POOLS = {}


def _probe_pool(canonical, lim):
    """2 * 10^6 seeded 31-mers that open with the m-mer, and the table slot of each one's (canonical) value"""
    key = (canonical, lim["SLOT_MUL"], lim["SLOT_BITS"])
    if key not in _POOLS:
        k = 31
        rng = np.random.default_rng(3100 + int(canonical))
        free = 2 * (k - CASE_M)
        fwd = (np.uint64(kmer_value(CASE_MMER, False)) << np.uint64(free)) | rng.integers(0, 1 << free, 2_000_000, dtype=np.uint64)
        fwd = np.unique(fwd)
        fwd = fwd[rng.permutation(len(fwd))]
        val = fwd
        if canonical:  # (bit tricks as a search aid only: check_case() takes the canonical form of what was found the plain way)
            rc, x = np.zeros_like(fwd), fwd.copy()
            for _ in range(k):
                rc = (rc << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
                x >>= np.uint64(2)
            val = np.minimum(fwd, rc)
        _POOLS[key] = (fwd, table_slots_np(val, lim))
    return _POOLS[key]


def _kmer_string(v, k):
    return "".join("ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def probe_cases(lim=None):
    """k = 31, m = 5, size 1: keys searched for their table slot — the longest chain the table can hold, wrapping from the last
    slot to slot 0; a cluster over the last four slots; duplicates inside the cluster; the same with canonical k-mers"""
    lim = lim or limits()
    full, last, k = lim["CT_FULL"], lim["CT_SLOTS"] - 1, 31
    out = []
    for canonical in (False, True):
        fwd, slots = _probe_pool(canonical, lim)
        rng = np.random.default_rng(3102 + int(canonical))
        tag = "canonical_" if canonical else ""

        def take(slot, n):
            found = fwd[slots == slot][:n]
            assert len(found) == n, f"only {len(found)} of {n} keys with slot {slot} in the pool"
            return found

        chain = take(last, full)
        out.append(_case(f"{tag}chain_of_CT_FULL_wraps", k, records_from_bases([_kmer_string(v, k) for v in chain], k, 0), canonical=canonical, path="table",
                         distinct=full, edge=full, slots={last: full}))
        per = full // 8
        cluster = np.concatenate([take(s, per) for s in range(last - 3, last + 1)])
        cluster = cluster[rng.permutation(len(cluster))]
        out.append(_case(f"{tag}cluster_on_last_slots", k, records_from_bases([_kmer_string(v, k) for v in cluster], k, 0), canonical=canonical, path="table",
                         distinct=4 * per, slots={s: per for s in range(last - 3, last + 1)}))
        per = full // 16
        keys = np.concatenate([take(s, per) for s in range(last - 3, last + 1)])
        dup = np.repeat(keys, 1 + np.arange(len(keys)) % 5)
        dup = dup[rng.permutation(len(dup))]
        out.append(_case(f"{tag}cluster_with_duplicates", k, records_from_bases([_kmer_string(v, k) for v in dup], k, 0), canonical=canonical, path="table",
                         distinct=4 * per, top_count=5, slots={s: per for s in range(last - 3, last + 1)}))
    return out


def all_count_cases(lim=None):
    lim = lim or limits()
    return round_cases(lim) + full_cases(lim) + sixteen_bit_cases(lim) + probe_cases(lim)


def check_case(case, lim=None):
    """assert, on the model alone, that a directed case sits where it says; returns bucket_fate() of it"""
    lim = lim or limits()
    recs, k, m, canonical, name = case["records"], case["k"], case["m"], case["canonical"], case["name"]
    mmer = case.get("mmer", CASE_MMER)
    for rec in recs[:: max(1, len(recs) // 64)]:
        assert record_mm_pos(rec) == 0 and record_bases(rec, k)[:m] == mmer, name  # one minimizer: one bucket
    assert all(record_bases(rec, k)[:m] == mmer for rec in recs[-3:]), name
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
    keys, counts = expected_counts(recs, k, canonical)
    if "slots" in case:
        got = {}
        for v in keys.tolist():
            got[table_slot(v, lim)] = got.get(table_slot(v, lim), 0) + 1
        assert got == case["slots"], (name, got)
    if "top_count" in case:
        assert int(counts.max()) == case["top_count"], (name, int(counts.max()))
        if case["path"] == "table":
            assert case["top_count"] <= 0xFFFF, name
    if "other_count" in case:
        assert sorted(counts.tolist())[0] == case["other_count"] and len(counts) == 2, name
    return fate
