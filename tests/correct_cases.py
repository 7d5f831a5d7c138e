"""The model of bl_scan_read_edits / bl_batch_apply_edits (include/biolib_amd.h: the rule) in plain Python, and the named reads the
emulation and the GPU tests run: one read per way the kernels can go wrong, hand-built tables, three layouts.  No device, no library."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WEAK, SOLID = 0, 1, 2
KS = (1, 2, 5, 31, 32, 33, 63, 64)
MIN_COUNT = 3
EDIT = np.dtype([("pos", "<u8"), ("from", "u1"), ("to", "u1"), ("support", "u1"), ("anchor", "u1"), ("reserved", "<u4")])
STAT_NAMES = ("n_runs", "n_edits", "n_ambiguous", "n_no_base", "n_misfit", "n_low_support")

_CODE = np.full(256, 4, np.uint8)
for _i, _letters in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _ch in _letters:
        _CODE[ord(_ch)] = _i


def constants():
    """the launch constants of biolib_amd/csrc/bl_correct_core.hpp, read from the source so that the tests move with a retuned value"""
    text = open(os.path.join(ROOT, "biolib_amd", "csrc", "bl_correct_core.hpp")).read()
    ctpb = int(re.search(r"constexpr int CTPB = (\d+);", text).group(1))
    assert re.search(r"constexpr int TEST_WAVES = CTPB / 64;", text)
    return dict(CTPB=ctpb, TEST_WAVES=ctpb // 64, MAX_RUN=int(re.search(r"constexpr int MAX_RUN = (\d+);", text).group(1)))


def as_bytes(x):
    return np.frombuffer(x.encode() if isinstance(x, str) else bytes(x), np.uint8) if not isinstance(x, np.ndarray) else x.astype(np.uint8)


# ---- k-mers
def read_kmers(codes, k, canonical):
    """per k-mer position of one read (len(codes) - k + 1 of them): (forward value, reverse complement value, key) or None where invalid"""
    L = len(codes)
    out = [None] * max(L - k + 1, 0)
    mask = (1 << (2 * k)) - 1
    fwd = rc = run = 0
    for i in range(L):
        c = int(codes[i])
        if c > 3:
            run = 0
            continue
        fwd = ((fwd << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
        run += 1
        if run >= k:
            out[i + 1 - k] = (fwd, rc, min(fwd, rc) if canonical else fwd)
    return out


def kmer_keys(text, k, canonical):
    """the keys of every valid k-mer of a string"""
    return [t[2] for t in read_kmers(_CODE[as_bytes(text)], k, canonical) if t is not None]


def states_of(kmers, table, min_count):
    return [INVALID if t is None else (SOLID if table.get(t[2], 0) >= min_count else WEAK) for t in kmers]


def weak_runs(states):
    runs, j, n = [], 0, len(states)
    while j < n:
        if states[j] == WEAK:
            a = j
            while j + 1 < n and states[j + 1] == WEAK:
                j += 1
            runs.append((a, j))
        j += 1
    return runs


# ---- the rule for one run of one read
def judge_run(a, b, states, kmers, k, table, min_count, min_support, canonical):
    """-> (class, p, anchor, code): class is one of edit / ambiguous / no_base / misfit / low_support"""
    n = len(states)
    if a >= 1 and states[a - 1] == SOLID:
        anchor, p = 0, a + k - 1
        fits = b == min(p, n - 1)
    elif b <= n - 2 and states[b + 1] == SOLID:
        anchor, p = 1, b
        fits = a == max(0, b - k + 1)
    else:
        return "misfit", None, None, None
    if not fits:
        return "misfit", None, None, None
    if b - a + 1 < min_support:
        return "low_support", p, anchor, None
    qualifying = []
    orig = (kmers[a][0] >> (2 * (k - 1 - (p - a)))) & 3
    for c in range(4):
        if c == orig:
            continue
        ok = True
        for j in range(a, b + 1):
            f, r, _ = kmers[j]
            at = p - j
            f = (f & ~(3 << (2 * (k - 1 - at)))) | (c << (2 * (k - 1 - at)))
            r = (r & ~(3 << (2 * at))) | ((3 - c) << (2 * at))
            key = min(f, r) if canonical else f
            if table.get(key, 0) < min_count:
                ok = False
                break
        if ok:
            qualifying.append(c)
    if len(qualifying) == 1:
        return "edit", p, anchor, qualifying[0]
    return ("no_base" if not qualifying else "ambiguous"), p, anchor, None


def model(bases, offs, k, table, min_count, min_support=1, canonical=False, first=0, n=0):
    """-> (edits: EDIT record array in ascending pos, stats: dict, detail: list of (read, a, b, class) with absolute a, b)"""
    bases = as_bytes(bases)
    offs = [int(x) for x in offs]
    n_bases = len(bases)
    end = n_bases if n == 0 or first + n > n_bases else first + n
    stats = dict.fromkeys(STAT_NAMES, 0)
    edits, detail = [], []
    for q in range(len(offs) - 1):
        lo, hi = offs[q], offs[q + 1]
        if hi - lo < k or hi <= first or lo >= end:
            continue
        codes = _CODE[bases[lo:hi]]
        kmers = read_kmers(codes, k, canonical)
        states = states_of(kmers, table, min_count)
        for a, b in weak_runs(states):
            if not first <= lo + a < end:
                continue
            cls, p, anchor, c = judge_run(a, b, states, kmers, k, table, min_count, min_support, canonical)
            stats["n_runs"] += 1
            stats["n_" + cls + ("s" if cls == "edit" else "")] += 1
            detail.append((q, lo + a, lo + b, cls))
            if cls == "edit":
                frm = int(bases[lo + p])
                edits.append((lo + p, frm, ord("ACGT"[c]) | (frm & 0x20), b - a + 1, anchor, 0))
    out = np.array(edits, dtype=EDIT) if edits else np.zeros(0, EDIT)
    assert (np.diff(out["pos"].astype(np.int64)) > 0).all(), "edits come in strictly ascending pos"
    return out, stats, detail


def apply_model(bases, edits):
    """bl_batch_apply_edits: pos >= n_bases ignored, among equal neighbours the first wins"""
    out = as_bytes(bases).copy()
    for i in range(len(edits)):
        pos = int(edits["pos"][i])
        if pos >= len(out) or (i > 0 and int(edits["pos"][i - 1]) == pos):
            continue
        out[pos] = edits["to"][i]
    return out


def position_states(bases, offs, k, table, min_count, canonical):
    """(state, count) of every position of the batch (INVALID / 0 where no valid k-mer starts)"""
    bases = as_bytes(bases)
    st, cnt = np.zeros(len(bases), np.uint8), np.zeros(len(bases), np.int64)
    for q in range(len(offs) - 1):
        lo, hi = int(offs[q]), int(offs[q + 1])
        for j, t in enumerate(read_kmers(_CODE[bases[lo:hi]], k, canonical)):
            if t is not None:
                cnt[lo + j] = table.get(t[2], 0)
                st[lo + j] = SOLID if cnt[lo + j] >= min_count else WEAK
    return st, cnt


# ---- the named reads
def _sub(s, p, shift=1):
    """s with the base at p replaced by another one"""
    return s[:p] + "ACGT"[("ACGT".index(s[p].upper().replace("U", "T")) + shift) % 4] + s[p + 1:]


@functools.lru_cache(maxsize=None)
def cases(k, canonical):
    """-> dict(names, reads (list of str), table {key: count}, min_count).  The table holds the k-mers of hand-chosen truths, every one
    with count exactly MIN_COUNT unless a case says otherwise."""
    rng = np.random.default_rng(1000 * k + int(canonical))
    names, reads, table = [], [], {}

    def truth(text, count=MIN_COUNT, skip=()):
        if k <= 2 and "T" in text:  # (keeps T out of the small tables)
            return
        for j, t in enumerate(read_kmers(_CODE[as_bytes(text)], k, canonical)):
            if t is not None and j not in skip:
                table[t[2]] = count

    def gen(n):  # (k <= 2: no T in the truths, so that an error can make a weak k-mer at all)
        alphabet = "ACG" if k <= 2 else "ACGT"
        return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))

    def err(text, p, shift=1):
        return text[:p] + "T" + text[p + 1:] if k <= 2 else _sub(text, p, shift)

    def add(name, text):
        names.append(name)
        reads.append(text)

    # an error at every base of a read of length k + 3, 2k and 2k + 5: interior runs, runs that reach the read's end, runs at its start
    for L in (k + 3, 2 * k, 2 * k + 5):
        g = gen(L)
        truth(g)
        for p in range(L):
            add(f"every_base_L{L}_p{p}", err(g, p, 1 + p % 3))
    # weak runs of exactly k, k - 1 and k + 1 k-mers next to each other, made by holes in the table
    g = gen(5 * k + 12)
    holes, at = set(), 2
    for length in (k, k - 1, k + 1):
        holes.update(range(at, at + length))
        at += length + 2
    truth(g, skip=holes)
    add("runs_k_km1_kp1", g)
    # an error in the first and in the last base: support 1
    g = gen(2 * k + 5)
    truth(g)
    add("first_base", err(g, 0))
    add("last_base", err(g, len(g) - 1))
    # a read of length k (one unanchored weak k-mer), k - 1 and 0
    g = gen(k)
    truth(err(g, k // 2))
    add("length_k", g)
    add("length_km1", gen(k - 1))
    add("length_0", "")
    # a run bounded by an N on either side
    g = gen(3 * k + 8)
    truth(g)
    p = k + 3
    e = err(g, p)
    add("N_behind", e[:p + 3] + "N" + e[p + 4:])
    add("N_in_front", e[:p - 2] + "N" + e[p - 1:])
    add("N_both", e[:p - 2] + "N" + e[p - 1:p + 3] + "N" + e[p + 4:])
    # a weak last k-mer of one read followed by a weak first k-mer of the next: runs do not join across reads
    g = gen(2 * k + 2)
    truth(g)
    add("weak_tail", err(g, len(g) - 1))
    add("weak_head", err(g, 0))
    # alternatives stored with exactly min_count (repaired) and exactly min_count - 1 (no base)
    g = gen(2 * k + 5)
    truth(g)
    add("alt_at_min_count", err(g, k + 1))
    g = gen(2 * k + 5)
    truth(g)
    mid = read_kmers(_CODE[as_bytes(g)], k, canonical)[2]  # one of the k-mers that hold base k + 1 (all of them where k = 1, 2)
    table[mid[2]] = MIN_COUNT - 1
    e = err(g, min(k + 1, len(g) - 1))
    add("alt_below_min_count", e)
    # two qualifying alternatives
    g = gen(2 * k + 5)
    truth(g)
    truth(err(g, k + 2, 1))
    add("ambiguous", err(g, k + 2, 2))
    # lower case, and U / u originals
    g = gen(2 * k + 5)
    truth(g)
    add("lower_case", err(g, k).lower())
    g = gen(2 * k + 5)
    gt = g[:k + 1] + "A" + g[k + 2:]
    truth(gt)
    add("U_original", (gt[:k + 1] + "T" + gt[k + 2:]).replace("T", "U"))
    add("u_original", (gt[:k + 1] + "T" + gt[k + 2:]).replace("T", "U").lower())
    # two errors k - 1 apart (one run too long or two joined: misfit) and k + 1 apart (two edits)
    g = gen(3 * k + 6)
    truth(g)
    add("two_errors_km1_apart", err(err(g, k + 1), 2 * k) if k > 1 else err(g, 1))
    add("two_errors_kp1_apart", err(err(g, k), 2 * k + 1))
    return dict(names=names, reads=reads, table=table, min_count=MIN_COUNT, k=k, canonical=canonical)


def layout(c, kind):
    """the reads as a batch: 'offsets' (ragged), 'fixed' (every read cut or N-padded to 2k + 5 bases: a fixed-length batch) or 'single'
    (joined by N into one sequence) -> dict(bases, offs, read_len)"""
    reads, k = c["reads"], c["k"]
    if kind == "offsets":
        offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
        return dict(bases=as_bytes("".join(reads)), offs=offs, read_len=0)
    if kind == "fixed":
        R = 2 * k + 5
        text = "".join((r + "N" * R)[:R] for r in reads)
        return dict(bases=as_bytes(text), offs=np.arange(0, len(text) + 1, R, dtype=np.uint64), read_len=R)
    assert kind == "single"
    text = "N".join(reads)
    return dict(bases=as_bytes(text), offs=np.array([0, len(text)], np.uint64), read_len=0)


LAYOUTS = ("offsets", "fixed", "single")


def table_arrays(table, k):
    """the table as the library takes it: (keys uint64 [n] or [n, 2] (low, high), counts uint32 [n]), sorted by key"""
    items = sorted(table.items())
    counts = np.array([v for _, v in items], np.uint32)
    if k <= 32:
        return np.array([key for key, _ in items], np.uint64), counts
    keys = np.array([[key & (2**64 - 1), key >> 64] for key, _ in items], np.uint64).reshape(-1, 2)
    return keys, counts


# ---- simulated reads (the issue's experiment): a random genome, reads from both strands, substitutions
def simulate(seed, genome_len, read_len, coverage, rate):
    """-> (reads with errors as one uint8 array, the error-free reads, offsets, planted: list of (pos in batch, true byte))"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len).astype(np.uint8)
    n_reads = genome_len * coverage // read_len
    starts = rng.integers(0, genome_len - read_len + 1, n_reads)
    rev = rng.integers(0, 2, n_reads).astype(bool)
    idx = starts[:, None] + np.arange(read_len)[None, :]
    codes = genome[idx]
    codes[rev] = 3 - codes[rev][:, ::-1]
    truth = codes.copy()
    err = rng.random(codes.shape) < rate
    codes[err] = (codes[err] + rng.integers(1, 4, int(err.sum()))) % 4
    letters = np.frombuffer(b"ACGT", np.uint8)
    offs = np.arange(0, (n_reads + 1) * read_len, read_len, dtype=np.uint64)
    planted = [(int(p), int(letters[truth.reshape(-1)[p]])) for p in np.nonzero(err.reshape(-1))[0]]
    return letters[codes].reshape(-1), letters[truth].reshape(-1), offs, planted


def counted_table(bases, offs, k, canonical):
    """the table counted from a batch's own k-mers"""
    table = {}
    bases = as_bytes(bases)
    for q in range(len(offs) - 1):
        for t in read_kmers(_CODE[bases[int(offs[q]):int(offs[q + 1])]], k, canonical):
            if t is not None:
                table[t[2]] = table.get(t[2], 0) + 1
    return table
