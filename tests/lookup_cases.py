"""TEST INFRASTRUCTURE: the tables, queries and scan cases of the count-table tests (tests/test_emu_lookup.py on the host emulation,
tests/test_gpu_lookup.py on the device).  Keys are Python integers below 2^(64 * key_words); a table is a dict key -> count.  Expected
answers are dict lookups; the scan's expected arrays come from tests/kmers128_model.py.  Shares no code with the library.
"""
import struct

import numpy as np

import kmers128_model as M

M64 = (1 << 64) - 1
SIZES = (0, 1, 2, 3, 63, 64, 65, 4097)
OPTIONS = (0, 1, 24, -1)  # "table_prefix_bits": forced 0, 1, the maximum (24, clamped to key_bits), automatic
H = 4096
SCAN_KS = (1, 16, 31, 32, 33, 47, 64)
RANGES = ((0, 0), (37, 8200))


def _rand_key(rng, bits):
    return int.from_bytes(rng.bytes(16), "little") & ((1 << bits) - 1)


def _rand_counts(rng, n):
    c = [int(x) for x in rng.integers(1, 1 << 32, n, dtype=np.uint64)]
    if n > 2:
        c[0], c[1], c[2] = 0, 1, (1 << 32) - 1  # a stored 0 answers like an absent key; both ends of the count's range
    return c


def queries_for(keys, key_words, key_bits):
    """below the smallest key, above the largest, between every pair of neighbours, equal to every key, and with a bit above key_bits"""
    top = (1 << (64 * key_words)) - 1
    ks = sorted(keys)
    q = set(ks)
    for a, b in zip(ks[:-1], ks[1:]):
        if b - a > 1:
            q.update((a + 1, b - 1, (a + b) // 2))
    if ks:
        q.update(x for x in (ks[0] - 1, ks[0] // 2, 0) if x >= 0)
        q.update(x for x in (ks[-1] + 1, (1 << key_bits) - 1) if x < (1 << key_bits))
    else:
        q.update((0, 1, (1 << key_bits) - 1))
    above = set()
    for bit in {key_bits, key_bits + 1, 63, 64, 64 * key_words - 1}:
        if key_bits <= bit < 64 * key_words:
            above.update((1 << bit) | k for k in ([0] + ks[:8] + ks[-8:]))
    out = sorted(q) + sorted(above - q)
    assert all(0 <= x <= top for x in out)
    return out


def table_cases():
    """(name, key_words, key_bits, table dict, queries, options)"""
    rng = np.random.default_rng(20260419)
    out = []
    for kw, kb in ((1, 62), (2, 102)):
        for n in SIZES:
            keys = set()
            while len(keys) < n:
                keys.add(_rand_key(rng, kb))
            keys = sorted(keys)
            out.append((f"random{n}", kw, kb, dict(zip(keys, _rand_counts(rng, n)))))
        # all keys in one prefix bucket (the top 8 bits), the buckets in front of it and behind it empty; in the first; in the last
        for name, prefix in (("one_bucket", 0x5A), ("first_bucket", 0x00), ("last_bucket", 0xFF)):
            keys = {(prefix << (kb - 8)) | _rand_key(rng, kb - 8) for _ in range(65)}
            if name == "first_bucket":
                keys.add(0)
            if name == "last_bucket":
                keys.add((1 << kb) - 1)
            keys = sorted(keys)
            out.append((name, kw, kb, dict(zip(keys, _rand_counts(rng, len(keys))))))
        # key 0 alone; key_bits = 2, where P is clamped to 2: every table of 0 .. 4 keys
        out.append(("zero", kw, kb, {0: 7}))
        for n in range(5):
            out.append((f"two_bits{n}", kw, 2, {k: 10 + k for k in range(4)[4 - n:]}))
        # the all-ones key of the full width
        full = 64 * kw
        keys = sorted({(1 << full) - 1, (1 << full) - 2, 0, 1} | {_rand_key(rng, full) for _ in range(61)})
        out.append(("all_ones", kw, full, dict(zip(keys, _rand_counts(rng, len(keys))))))
    # pairs that differ only in the high word, pairs that differ only in the low word (two-word keys; key_bits 102 and 128)
    for kb in (102, 128):
        hi_bits = kb - 64
        keys = set()
        for _ in range(20):
            lo, hi = _rand_key(rng, 64), _rand_key(rng, hi_bits)
            keys.update(((hi << 64) | lo, ((hi ^ 1) << 64) | lo, ((hi ^ (1 << (hi_bits - 1))) << 64) | lo))  # same low word
            keys.update(((hi << 64) | (lo ^ 1), (hi << 64) | (lo ^ (1 << 63))))                                # same high word
        keys = sorted(keys)
        out.append((f"word_pairs{kb}", 2, kb, dict(zip(keys, _rand_counts(rng, len(keys))))))
    # one-word keys of the low-word pairs, and a two-word table whose keys all fit one word (key_bits <= 64: any high word is above)
    keys = sorted({_rand_key(rng, 40) for _ in range(64)})
    out.append(("narrow_in_two_words", 2, 40, dict(zip(keys, _rand_counts(rng, len(keys))))))
    return [(name, kw, kb, t, queries_for(t.keys(), kw, kb), OPTIONS) for name, kw, kb, t in out]


def words(keys, key_words):
    """uint64 array: one word per key, or (low, high) pairs"""
    if key_words == 1:
        return np.array([int(k) for k in keys], np.uint64).reshape(-1)
    return np.array([[int(k) & M64, int(k) >> 64] for k in keys], np.uint64).reshape(-1, 2)


def table_file(key_words, key_bits, table, queries, options):
    keys = sorted(table)
    return (struct.pack("<5Q", key_words, key_bits, len(keys), len(queries), len(options)) + np.array(options, np.int64).tobytes()
            + words(keys, key_words).tobytes() + np.array([table[k] for k in keys], np.uint64).tobytes() + words(queries, key_words).tobytes())


def make_batch(k, rng):
    """the batch of test_emu_kmers128.make_batch: two tiles and a ragged end; reads of length k-1, k, k+1 (and 1, 150); N at the first and the
    last base of a tile; bytes 0x80 and 0xFF"""
    n = 2 * H + 1007
    seq = rng.choice(np.frombuffer(b"ACGTacgtUu", np.uint8), n)
    lens = [k + 1, k, max(k - 1, 1), 1, 150]
    offs = [0]
    for length in lens:
        offs.append(offs[-1] + length)
    offs += [H - 3, H + k, 2 * H - 1, 2 * H + 500, n]
    offs = np.array(sorted(set(offs)), np.uint64)
    seq[[H, 2 * H - 1, 2 * H, 3000, 3001, n - 1 - 2 * k]] = ord("N")
    seq[5000] = 0x80
    seq[5200] = 0xFF
    return seq, offs


def kmer_keys(m):
    """the model's k-mers as Python integers, by position (0 where none starts)"""
    return [(int(h) << 64) | int(l) for l, h in zip(m["lo"], m["hi"])]


def own_table(m, drop=True):
    """the scan's own distinct k-mers with their true multiplicities, minus those with hash_u128(lo, hi, 7) % 3 == 0"""
    t = {}
    for key, ok in zip(kmer_keys(m), m["valid"]):
        if ok:
            t[key] = t.get(key, 0) + 1
    if drop:
        t = {k: c for k, c in t.items() if M.hash_u128(k & M64, k >> 64, 7) % 3 != 0}
    return t


def expected_scan(m, table, first, end):
    """counts, valid (numpy) and the five digest words over [first, end)"""
    keys = kmer_keys(m)
    valid = m["valid"][first:end]
    counts = np.array([table.get(keys[p], 0) if m["valid"][p] else 0 for p in range(first, end)], np.uint32)
    found = sum(1 for p in range(first, end) if m["valid"][p] and keys[p] in table)
    d = M.digest(m, first, end)
    return counts, valid, dict(count=d["count"], xor_value=d["xor_value"], aux=d["aux"], xor_hash=found, xor_pos=int(counts.sum(dtype=np.uint64)) & M64)


def scan_cases(ks=SCAN_KS):
    """(k, canonical, drop_last, seq, offs, model, [tables]) — for k = 1 three explicit tables (empty, {A}, all four keys), otherwise the
    batch's own table; for k >= 8 every range has at least 100 valid positions found, 100 not found and 10 invalid ones (checked here)"""
    for k in ks:
        seq, offs = make_batch(k, np.random.default_rng(1000 + k))
        for canonical in (False, True):
            for drop_last in (False, True):
                m = M.scan(seq.tobytes(), offs, k, 0, canonical, drop_last)
                tables = [{}, {0: 5}, {0: 5, 1: 7, 2: 11, 3: 13}] if k == 1 else [own_table(m)]
                if k >= 8:
                    for first, n in RANGES:
                        end = len(seq) if n == 0 else first + n
                        counts, valid, d = expected_scan(m, tables[0], first, end)
                        assert d["xor_hash"] >= 100 and d["count"] - d["xor_hash"] >= 100 and int((valid == 0).sum()) >= 10, (k, first, d)
                yield k, canonical, drop_last, seq, offs, m, tables
