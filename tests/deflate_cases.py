"""TEST INFRASTRUCTURE: the specification of bl_bgzf_deflate (biolib_amd/csrc/bl_deflate_core.hpp) as a Python model, and the named
cases.  The model returns the exact bytes the device call writes, its member table, and counters: members per block form, whether the
length limiter ran, the longest and shortest match and the furthest and nearest distance taken.

The rules, restated from the core header (a member is text[i * 65280 : (i + 1) * 65280], compressed on its own):
  price     LIT4 = max(4, sum_b count[b] * q(b) // n), q(b) = 4 * (e - 16) + ((x >> (e - 2)) & 3), x = (n << 16) // count[b], e = floor(log2 x)
  parse     steps of 64 positions.  Position p (at or behind `next`, 3 bytes or more left) has up to three candidates, in this order: p - 1;
            T3[hash3(p)] where 3 bytes are left; T8[hash8(p)] where 8 bytes are left.  The tables hold the highest position of every EARLIER
            step with that hash.  A candidate at distance <= 32768 with match length len >= 3 (at most 258, at most the bytes left) scores
            len * LIT4 - 4 * (12 + extra bits of the distance's symbol); below 0 it is out; the highest score wins, ties go to the smaller
            distance.  Greedy: from `next`, literals up to the first position with a match, the match, and on behind it.
  codes     Huffman lengths from the histograms (end of block counted once): used symbols sorted by (count, symbol), two-queue merge with a
            merge before a leaf of equal weight, depths folded at 15, the Kraft repair, lengths reassigned in sorted order, the rarest the
            longest.  Fewer than two used symbols: two 1-bit codes, the used symbol and the lowest other one.
  form      stored n + 5 bytes, fixed and dynamic from their bit counts; the smallest in bytes, ties stored < fixed < dynamic
  header    dynamic: HLIT / HDIST up to the highest coded symbol, HCLEN 19, code-length symbols 0..15 four bits each and no repeats
The bit writer and the symbol tables are deflate_writer.py's."""
import functools
import struct
import zlib

import numpy as np

import deflate_writer as DW

MEMBER = 65280
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
T3_BITS, T8_BITS = 12, 13
MAX_LEN, MAX_DIST = 258, 32768
MATCH_BASE_BITS = 12
GROUP_MEMBERS = 1024  # members the device call compresses side by side (bl_deflate.hip)

_LEN_BASE, _LEN_EXTRA = np.array(DW.LEN_BASE), np.array(DW.LEN_EXTRA)
_DIST_BASE, _DIST_EXTRA = np.array(DW.DIST_BASE), np.array(DW.DIST_EXTRA)


def bound(n_bytes, eof=True):
    return n_bytes + 31 * ((n_bytes + MEMBER - 1) // MEMBER) + (28 if eof else 0)


def _lit4(a):
    n, s = len(a), 0
    for c in np.bincount(a, minlength=256):
        c = int(c)
        if c:
            x = (n << 16) // c
            e = x.bit_length() - 1
            s += c * (4 * (e - 16) + ((x >> (e - 2)) & 3))
    return max(4, s // n)


def _match_lengths(pad, c, p, max_len):
    """bytes that pad[c ..] and pad[p ..] share, at most max_len, for arrays of positions"""
    k = np.zeros(len(p), np.int64)
    live = np.arange(len(p))
    step = np.arange(8)
    while len(live):
        at = k[live][:, None] + step
        same = (pad[c[live][:, None] + at] == pad[p[live][:, None] + at]) & (at < max_len[live][:, None])
        run = np.where(same.all(axis=1), 8, np.argmin(same, axis=1))
        k[live] += run
        live = live[run == 8]
    return k


def parse(text):
    """the tokens of one member: (literal bytes or -1, lengths, distances) as arrays, one entry per token"""
    n = len(text)
    a = np.frombuffer(text, np.uint8)
    pad = np.zeros(n + MAX_LEN + 16, np.uint8)
    pad[:n] = a
    w = np.zeros(n, np.uint64)
    for i in range(8):
        w |= pad[i:i + n].astype(np.uint64) << np.uint64(8 * i)
    h3 = (((w & np.uint64(0xFFFFFF)).astype(np.uint32) * np.uint32(0x9E3779B1)) >> np.uint32(32 - T3_BITS)).astype(np.int64)
    h8 = ((w * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - T8_BITS)).astype(np.int64)
    lit4 = _lit4(a)
    t3, t8 = np.zeros(1 << T3_BITS, np.int64), np.zeros(1 << T8_BITS, np.int64)
    lits, lens, dists = [], [], []

    def literals(lo, hi):
        if hi > lo:
            lits.append(a[lo:hi].astype(np.int64))
            lens.append(np.zeros(hi - lo, np.int64))
            dists.append(np.zeros(hi - lo, np.int64))

    nxt = 0
    for b in range(0, n, 64):
        end = min(b + 64, n)
        if nxt < end:
            p = np.arange(max(b, nxt), end)
            p = p[n - p >= 3]
            max_len = np.minimum(n - p, MAX_LEN)
            best_len, best_dist, best_score = np.zeros(len(p), np.int64), np.zeros(len(p), np.int64), np.zeros(len(p), np.int64)
            c8 = np.where(p + 8 <= n, t8[h8[p]], 0) - 1
            for c in (p - 1, t3[h3[p]] - 1, c8):
                dist = p - c
                ok = (c >= 0) & (dist <= MAX_DIST)
                ln = np.zeros(len(p), np.int64)
                ln[ok] = _match_lengths(pad, c[ok], p[ok], max_len[ok])
                ok &= ln >= 3
                sym = np.searchsorted(_DIST_BASE, np.where(ok, dist, 1), "right") - 1
                score = ln * lit4 - 4 * (MATCH_BASE_BITS + _DIST_EXTRA[sym])
                ok &= score >= 0
                better = ok & ((best_len == 0) | (score > best_score) | ((score == best_score) & (dist < best_dist)))
                best_len[better], best_dist[better], best_score[better] = ln[better], dist[better], score[better]
            for i in np.flatnonzero(best_len):
                at = int(p[i])
                if at < nxt:
                    continue
                literals(nxt, at)
                lits.append(np.array([-1]))
                lens.append(best_len[i:i + 1])
                dists.append(best_dist[i:i + 1])
                nxt = at + int(best_len[i])
            if nxt < end:
                literals(nxt, end)
                nxt = end
        q = np.arange(b, end)
        q3, q8 = q[q + 3 <= n], q[q + 8 <= n]
        t3[h3[q3]] = q3 + 1  # (ascending positions: the highest stays)
        t8[h8[q8]] = q8 + 1
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return cat(lits), cat(lens), cat(dists)


def code_lengths(freq):
    """(lengths, whether the limiter ran) of the Huffman code of `freq`"""
    n_sym = len(freq)
    lens = [0] * n_sym
    order = sorted((s for s in range(n_sym) if freq[s]), key=lambda s: (freq[s], s))
    m = len(order)
    if m < 2:
        s0 = order[0] if m else 0
        lens[s0] = 1
        lens[1 if s0 == 0 else 0] = 1
        return lens, False
    weight = [int(freq[s]) for s in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    li, ii, nn = 0, m, m
    for _ in range(m - 1):
        pick = []
        for _ in range(2):
            if li < m and (ii >= nn or weight[li] < weight[ii]):
                pick.append(li)
                li += 1
            else:
                pick.append(ii)
                ii += 1
        weight[nn] = weight[pick[0]] + weight[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nn
        nn += 1
    depth = [0] * (2 * m - 1)
    for i in range(2 * m - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    count = [0] * 16
    for i in range(m):
        count[min(depth[i], 15)] += 1
    limited = max(depth[:m]) > 15
    kraft = sum(count[k] << (15 - k) for k in range(1, 16))
    while kraft > 32768:
        bits = max(k for k in range(1, 15) if count[k])
        count[bits] -= 1
        count[bits + 1] += 2
        count[15] -= 1
        kraft -= 1
    at = 0
    for k in range(15, 0, -1):
        for _ in range(count[k]):
            lens[order[at]] = k
            at += 1
    return lens, limited


def _pack(values, n_bits):
    """(the pieces, each LSB first, one behind the other, as one integer; its bit count)"""
    total = int(n_bits.sum())
    if total == 0:
        return 0, 0
    bits = ((values[:, None] >> np.arange(48, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    bits = bits[np.arange(48) < n_bits[:, None]]
    return int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little"), total


def _token_bits(lits, lens, dists, ll_lens, d_lens):
    """every token and the end of block as (value, bit count) under the two codes"""
    rev = lambda codes: (np.array([DW._reverse(c, n) for c, n in codes], np.uint64), np.array([n for _, n in codes], np.int64))
    ll_code, ll_n = rev(DW.canonical_codes(ll_lens))
    d_code, d_n = rev(DW.canonical_codes(d_lens))
    is_match = lits < 0
    ls = np.searchsorted(_LEN_BASE, np.where(is_match, lens, 3), "right") - 1
    ds = np.searchsorted(_DIST_BASE, np.where(is_match, dists, 1), "right") - 1
    sym = np.where(is_match, 257 + ls, lits)
    value, n_bits = ll_code[sym].copy(), ll_n[sym].copy()
    assert (n_bits > 0).all()
    u = lambda x: x.astype(np.uint64)
    for piece, width in ((u(lens - _LEN_BASE[ls]), _LEN_EXTRA[ls]), (d_code[ds], d_n[ds]), (u(dists - _DIST_BASE[ds]), _DIST_EXTRA[ds])):
        width = np.where(is_match, width, 0)
        assert (width[is_match] >= 0).all()
        value |= np.where(is_match, piece, np.uint64(0)) << u(n_bits)
        n_bits = n_bits + width
    assert not is_match.any() or (d_n[ds[is_match]] > 0).all()
    return np.append(value, ll_code[256]), np.append(n_bits, ll_n[256])


@functools.lru_cache(maxsize=4096)
def member_model(text):
    """one member: (its bytes, info) — info: form 0 stored / 1 fixed / 2 dynamic, limited, max_len, min_len, max_dist, min_dist (0: no match),
    data_bits (of the deflate data, before the padding to a byte), crc"""
    n = len(text)
    assert 1 <= n <= MEMBER
    lits, lens, dists = parse(text)
    is_match = lits < 0
    ls = np.searchsorted(_LEN_BASE, lens[is_match], "right") - 1
    ds = np.searchsorted(_DIST_BASE, dists[is_match], "right") - 1
    ll_freq = np.bincount(np.concatenate([lits[~is_match], 257 + ls, [256]]), minlength=286)
    d_freq = np.bincount(ds, minlength=30)
    ll_lens, lim1 = code_lengths(ll_freq)
    d_lens, lim2 = code_lengths(d_freq)
    hlit = max(257, max(s + 1 for s in range(286) if ll_lens[s]))
    hdist = max(s + 1 for s in range(30) if d_lens[s])
    ll_x = np.array([0] * 257 + DW.LEN_EXTRA)
    dyn_bits = 3 + 14 + 57 + 4 * (hlit + hdist) + int((ll_freq * (np.array(ll_lens) + ll_x)).sum()) + int((d_freq * (np.array(d_lens) + _DIST_EXTRA)).sum())
    fix_bits = 3 + int((ll_freq * (np.array(DW.FIXED_LL[:286]) + ll_x)).sum()) + int((d_freq * (5 + _DIST_EXTRA)).sum())
    sizes = [n + 5, (fix_bits + 7) // 8, (dyn_bits + 7) // 8]
    form = sizes.index(min(sizes))
    d = DW.DeflateWriter()
    if form == 0:
        d.stored(text, final=True)
        data_bits = 8 * (n + 5)
    else:
        if form == 1:
            d.header(True, 1)
            value, n_bits = _token_bits(lits, lens, dists, DW.FIXED_LL, DW.FIXED_D)
        else:
            d.header(True, 2)
            d.dynamic_header(ll_lens, d_lens, cl_lens=[4] * 16 + [0] * 3, cl_stream=DW.plain_cl_stream(ll_lens[:hlit] + d_lens[:hdist]), hlit=hlit - 257,
                             hdist=hdist - 1, hclen=15)
            value, n_bits = _token_bits(lits, lens, dists, ll_lens[:hlit], d_lens[:hdist])
        d.w.bits(*_pack(value, n_bits))
        data_bits = d.w.bit_length()
        assert data_bits == (fix_bits if form == 1 else dyn_bits), "the size computed before the bits is the size"
    data = d.getvalue()
    assert len(data) == sizes[form]
    m = DW.bgzf_member(data, text)
    assert len(m) <= n + 31
    info = dict(form=form, limited=bool(lim1 or lim2), max_len=int(lens.max(initial=0)), min_len=int(lens[is_match].min(initial=999)) % 999,
                max_dist=int(dists.max(initial=0)), min_dist=int(dists[is_match].min(initial=99999)) % 99999, data_bits=data_bits,
                crc=zlib.crc32(text) & 0xFFFFFFFF, n_matches=int(is_match.sum()))
    return m, info


def bgzf_model(text, eof=True):
    """the bytes of bl_bgzf_deflate, the counters, and the member table as rows (src_off, dst_off, src_len, isize, crc)"""
    out, table, at = [], [], 0
    c = dict(forms=[0, 0, 0], limited=0, max_len=0, min_len=0, max_dist=0, min_dist=0)
    for i in range(0, len(text), MEMBER):
        part = bytes(text[i:i + MEMBER])
        m, info = member_model(part)
        out.append(m)
        table.append((at + 18, i, len(m) - 26, len(part), info["crc"]))
        at += len(m)
        c["forms"][info["form"]] += 1
        c["limited"] += info["limited"]
        c["max_len"], c["max_dist"] = max(c["max_len"], info["max_len"]), max(c["max_dist"], info["max_dist"])
        for k in ("min_len", "min_dist"):
            if info[k]:
                c[k] = min(c[k], info[k]) if c[k] else info[k]
    if eof:
        out.append(EOF_MARKER)
    return b"".join(out), c, table


def check_members(data, text, eof=True, full_members=True):
    """every member's header, BSIZE, CRC-32 and ISIZE; every member at most ISIZE + 31 bytes; the EOF marker.  full_members: every member
    but the last holds 65,280 bytes (False: a file several calls appended to).  Returns the member count."""
    at, done, n = 0, 0, 0
    while at < len(data):
        head = data[at:at + 18]
        assert head[:16] == bytes.fromhex("1f8b08040000000000ff0600") + b"BC\x02\x00", (n, head.hex())
        size = struct.unpack("<H", head[16:18])[0] + 1
        crc, isize = struct.unpack("<II", data[at + size - 8:at + size])
        part = zlib.decompress(data[at + 18:at + size - 8], -15)
        assert len(part) == isize and zlib.crc32(part) & 0xFFFFFFFF == crc and size <= isize + 31, n
        assert part == text[done:done + isize], n
        if isize == 0:
            assert eof and at + size == len(data) and data[at:] == EOF_MARKER, "an empty member only as the EOF marker"
        else:
            assert isize == min(MEMBER, len(text) - done) if full_members else isize <= MEMBER, n
            n += 1
        at, done = at + size, done + isize
    assert at == len(data) and done == len(text)
    assert (data[-28:] == EOF_MARKER) == bool(eof) or (not eof and not text)
    return n


# ----------------------------------------------------------------------------- the named cases

def _rng(seed):
    return np.random.default_rng(5150 + seed)


def random_bytes(n, seed=0):
    return _rng(seed).integers(0, 256, int(n)).astype(np.uint8).tobytes()


def dna_lines(n, seed=0, width=151):
    """uniform random ACGT with a newline every (width + 1)-th byte"""
    a = _rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), int(n))
    a[width::width + 1] = 10
    return a.tobytes()


def simulated_fastq(n_reads=4000, read_len=150, genome_len=20000, seed=1):
    """reads at uniform positions of a random genome; names @read<i>/1 pos=<p>; qualities clip(normal(36, 4), 2, 40) + 33"""
    r = _rng(seed)
    genome = r.choice(np.frombuffer(b"ACGT", np.uint8), genome_len)
    pos = r.integers(0, genome_len - read_len + 1, n_reads)
    qual = (np.clip(np.rint(r.normal(36, 4, (n_reads, read_len))), 2, 40) + 33).astype(np.uint8)
    return b"".join(b"@read%d/1 pos=%d\n%s\n+\n%s\n" % (i, int(p), genome[int(p):int(p) + read_len].tobytes(), qual[i].tobytes()) for i, p in enumerate(pos))


def repeated_line(seed=2, length=1000, times=300):
    line = _rng(seed).integers(33, 127, length).astype(np.uint8).tobytes() + b"\n"
    return line * times


def no_match_text():
    """every 3-byte string over 8 letters exactly once (a de Bruijn sequence, unrolled): nothing to match, no distance symbol used"""
    k, n, seq, a = 8, 3, [], [0] * 24

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return bytes(65 + s for s in seq + seq[:n - 1])


def fibonacci_text():
    """byte frequencies 1, 1, 2, 3, 5, 8, ... over 18 symbols: the unlimited Huffman code is 17 deep.  The bytes are drawn at random
    without replacement; a draw that would repeat an 8-byte string of the text so far, or a 6-byte string of its last 600 bytes, is drawn
    again: at this text's literal price no candidate the parse looks at is long enough for its distance, so nothing matches."""
    f = [1, 1]
    while len(f) < 18:
        f.append(f[-1] + f[-2])
    for seed in range(64):
        r, left, seen6, seen8, t = _rng(100 + seed), np.array(f), {}, set(), bytearray()
        while left.sum():
            w = left ** 1.1  # (the frequent bytes a little sooner: what is left at the end is easy to place)
            for _ in range(200):
                s = int(r.choice(18, p=w / w.sum()))
                g6, g8 = bytes(t[-5:]) + bytes([97 + s]), bytes(t[-7:]) + bytes([97 + s])
                if (len(g6) < 6 or len(t) - seen6.get(g6, -1000) > 600) and (len(g8) < 8 or g8 not in seen8):
                    break
            else:
                break  # (stuck: the next seed)
            seen6[g6] = len(t)
            seen8.add(g8)
            t.append(97 + s)
            left[s] -= 1
        if not left.sum() and not (parse(bytes(t))[0] < 0).any():
            return bytes(t)
    raise AssertionError("no shuffle without a match")


def far_repeat(distance):
    """300 random bytes, random filler, and the 300 bytes again `distance` behind their first occurrence"""
    s = random_bytes(300, 11)
    return s + random_bytes(distance - 300, 12) + s + random_bytes(100, 13)


@functools.lru_cache(maxsize=None)
def bit_offset_texts():
    """eight short texts whose deflate data end at bit offset 0, 1, ... 7 of a byte"""
    found, k = {}, 0
    while len(found) < 8 and k < 4000:
        t = dna_lines(600 + k % 97, 300 + k, width=30) + b"@r%d\n" % k
        found.setdefault(member_model(t)[1]["data_bits"] % 8, t)
        k += 1
    assert len(found) == 8
    return [found[r] for r in range(8)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (text, eof)"""
    import format_cases as FC

    fc = FC.cases()
    fastq = max((c["text"] for c in fc.values() if c["text"] and c["text"][:1] == b"@"), key=len)
    fasta = max((c["text"] for c in fc.values() if c["text"] and c["text"][:1] == b">"), key=len)
    mixed = dna_lines(MEMBER, 3) + simulated_fastq(260, seed=4)[:MEMBER] + random_bytes(MEMBER, 5) + b"A" * 17
    assert len(mixed) == 3 * MEMBER + 17
    c = {
        "empty": (b"", True),
        "empty_no_eof": (b"", False),
        "bytes_1": (b"A", True),
        "bytes_2": (b"AC", True),
        "bytes_3": (b"AAA", True),
        "bytes_4": (b"ACGT", False),
        "member_minus_1": (simulated_fastq(210, seed=6)[:MEMBER - 1], True),
        "member_exact": (simulated_fastq(210, seed=6)[:MEMBER], True),
        "member_plus_1": (simulated_fastq(210, seed=6)[:MEMBER + 1], True),
        "four_kinds": (mixed, True),
        "one_byte_repeated": (b"G" * MEMBER, True),
        "no_match": (no_match_text(), True),
        "twenty_bytes": (b"ACGTTGCATTGACCAGTACG", True),
        "random_bytes": (random_bytes(5000, 7), True),
        "fibonacci": (fibonacci_text(), True),
        "far_32768": (far_repeat(32768), True),
        "far_32769": (far_repeat(32769), True),
        "format_fastq": (fastq, True),
        "format_fasta": (fasta, False),
        "simulated_fastq": (simulated_fastq(300, seed=8), True),
    }
    for r, t in enumerate(bit_offset_texts()):
        c["ends_at_bit_%d" % r] = (t, True)
    return c


def ratio_texts():
    """the three texts of the ratio caps: name -> (text, cap on compressed size / text size)"""
    return {
        "random_dna_lines": (dna_lines(1 << 20, 21), 0.35),
        "simulated_fastq": (simulated_fastq(), 0.52),
        "repeated_line": (repeated_line(), 0.03),
    }


def zlib_bgzf_size(text, level):
    """what zlib at `level` makes of the same 65,280-byte blocks, 26 bytes of framing a member"""
    total = 0
    for i in range(0, len(text), MEMBER):
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(z.compress(text[i:i + MEMBER]) + z.flush()) + 26
    return total
