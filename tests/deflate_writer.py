"""TEST INFRASTRUCTURE: a symbol-level DEFLATE writer, written from RFC 1951 (and RFC 1952 / SAM §4.1 for the BGZF wrapper).

An encoder decides which symbols a stream holds; this writer lets the TEST decide: every literal, every (length, distance)
pair, every code length, every field of a dynamic block's header, sound or not.  Nothing here decodes; zlib is the judge of
what the streams mean (tests/inflate_corpus.py).

A symbol list is a sequence of
    int 0..255            a literal
    (length, distance)    a match, 3 <= length <= 258, 1 <= distance <= 32768
    ("ll", s)             the bare literal/length symbol s (no extra bits): reserved symbols, a length without a distance
    ("d", s)              the bare distance symbol s (no extra bits)
"""
import struct
import zlib

END = 256
# RFC 1951 §3.2.5
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
# §3.2.6 (symbols 286, 287 and distance symbols 30, 31 take part in the fixed codes and never occur in a sound stream)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
# §3.2.7: the order in which the lengths of the code-length code are sent
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# a complete code over all 19 code-length symbols (13 / 16 + 6 / 32 = 1): what dynamic() uses when the caller gives none
CL_ALL = [4] * 13 + [5] * 6


class NoCode(Exception):
    """the symbol has no code in the code set in use (the writer does not emit it unless forced)"""


def length_symbol(length):
    """(symbol, number of extra bits, their value) of a match length"""
    if not 3 <= length <= 258:
        raise ValueError(f"match length {length}")
    if length == 258:
        return 285, 0, 0
    c = max(i for i in range(28) if LEN_BASE[i] <= length)
    assert length - LEN_BASE[c] < (1 << LEN_EXTRA[c])
    return 257 + c, LEN_EXTRA[c], length - LEN_BASE[c]


def distance_symbol(distance):
    if not 1 <= distance <= 32768:
        raise ValueError(f"match distance {distance}")
    c = max(i for i in range(30) if DIST_BASE[i] <= distance)
    assert distance - DIST_BASE[c] < (1 << DIST_EXTRA[c])
    return c, DIST_EXTRA[c], distance - DIST_BASE[c]


_LEN_SYM = [None] * 3 + [length_symbol(n) for n in range(3, 259)]
_DIST_SYM = {}


def _dist_sym(d):
    s = _DIST_SYM.get(d)
    if s is None:
        s = _DIST_SYM[d] = distance_symbol(d)
    return s


def canonical_codes(lengths):
    """§3.2.2: the code of every symbol from the code lengths, [(code, length)], whatever the Kraft sum of the lengths is (an
    over-subscribed set gets codes that overflow their length; they are masked, as a careless encoder would)"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for n in lengths:
        if n:
            out.append((nxt[n] & ((1 << n) - 1), n))
            nxt[n] += 1
        else:
            out.append((0, 0))
    return out


_FIXED_CODES = {}


def _codes(lengths):
    """[(code as it goes into the stream: first bit lowest, length)] of canonical_codes; the two fixed codes computed once"""
    fixed = lengths is FIXED_LL or lengths is FIXED_D
    if fixed and id(lengths) in _FIXED_CODES:
        return _FIXED_CODES[id(lengths)]
    codes = [(_reverse(c, n), n) for c, n in canonical_codes(lengths)]
    if fixed:
        _FIXED_CODES[id(lengths)] = codes
    return codes


def kraft(lengths):
    """sum of 2^-len over the coded symbols, in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - n) for n in lengths if n)


def _reverse(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


class BitWriter:
    """fields go in LSB-first (§3.1.1), Huffman codes MSB-first"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        if n:
            assert 0 <= value < (1 << n), (value, n)
            self.acc |= value << self.n
            self.n += n
            if self.n >= 8:
                k = self.n >> 3
                self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
                self.acc >>= 8 * k
                self.n -= 8 * k

    def code(self, code, n):
        self.bits(_reverse(code, n), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def bit_length(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        """the bytes so far, the last one filled up with zero bits"""
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def plain_cl_stream(lengths):
    """the lengths one by one, no repeats"""
    return list(lengths)


def rle_cl_stream(lengths):
    """the lengths with repeats 16 / 17 / 18 wherever they fit (greedy)"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [0] * run
        else:
            out.append(v)
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k))
                run -= k
            out += [v] * run
        i = j
    return out


def cl_stream_length(stream):
    """how many code lengths a code-length stream stands for"""
    return sum(1 if isinstance(s, int) else s[1] for s in stream)


class DeflateWriter:
    def __init__(self):
        self.w = BitWriter()

    def getvalue(self):
        return self.w.getvalue()

    def header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, len_=None, nlen=None):
        """a stored block; LEN and NLEN as given where given (the bytes that follow are `data` whatever LEN says)"""
        self.header(final, 0)
        self.w.align()
        n = len(data) if len_ is None else len_
        self.w.bits(n, 16)
        self.w.bits((n ^ 0xFFFF) if nlen is None else nlen, 16)
        self.w.raw(data)

    def symbols(self, symbols, ll_lens, d_lens, force=False):
        """the symbols with the codes that the two arrays of code lengths define.  A symbol whose code length is 0 (or that
        lies beyond the arrays) raises NoCode; with force=True it goes out as a code of no bits and its extra bits"""
        ll, d, w = _codes(ll_lens), _codes(d_lens), self.w

        def put(codes, s, what):
            if s >= len(codes) or codes[s][1] == 0:
                if not force:
                    raise NoCode(f"{what} symbol {s} has no code")
                return
            w.bits(*codes[s])

        for s in symbols:
            if isinstance(s, int):
                if not 0 <= s <= 256:
                    raise ValueError(f"literal {s}")
                put(ll, s, "literal/length")
            elif s[0] == "ll":
                put(ll, s[1], "literal/length")
            elif s[0] == "d":
                put(d, s[1], "distance")
            else:
                length, dist = s
                sym, nx, x = _LEN_SYM[length] if 3 <= length <= 258 else length_symbol(length)
                put(ll, sym, "literal/length")
                w.bits(x, nx)
                sym, nx, x = _dist_sym(dist)
                put(d, sym, "distance")
                w.bits(x, nx)

    def fixed(self, symbols, final=False, end=True, force=False):
        self.header(final, 1)
        self.symbols(list(symbols) + ([END] if end else []), FIXED_LL, FIXED_D, force)

    def dynamic_header(self, ll_lens, d_lens, cl_lens=None, cl_stream=None, hlit=None, hdist=None, hclen=None, force=False, cut_bits=None):
        """HLIT, HDIST, HCLEN, the code-length code and the code lengths.  By default the fields are what the arrays need
        (trailing zero lengths are not sent, down to 257 / 1 / 4), the code-length code is CL_ALL and the lengths go out with
        repeats; every one of them can be given instead: hlit / hdist / hclen are the RAW field values, cl_stream a list of
        lengths 0..15 and repeats (16, 3..6), (17, 3..10), (18, 11..138) that is written as it stands, whatever it adds up to."""
        w = self.w
        n_ll = max(257, max((i + 1 for i, n in enumerate(ll_lens) if n), default=0)) if hlit is None else hlit + 257
        n_d = max(1, max((i + 1 for i, n in enumerate(d_lens) if n), default=0)) if hdist is None else hdist + 1
        if cl_lens is None:
            cl_lens = CL_ALL
        n_cl = max(4, max((i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]), default=0)) if hclen is None else hclen + 4
        if cl_stream is None:
            pad = lambda a, n: (list(a) + [0] * n)[:n]
            cl_stream = rle_cl_stream(pad(ll_lens, n_ll) + pad(d_lens, n_d))
        w.bits(n_ll - 257, 5)
        w.bits(n_d - 1, 5)
        w.bits(n_cl - 4, 4)
        for s in CL_ORDER[:n_cl]:
            w.bits(cl_lens[s], 3)
        cl = canonical_codes(cl_lens)
        for s in cl_stream:
            sym, count = (s, 0) if isinstance(s, int) else s
            if not 0 <= sym <= 18:
                raise ValueError(f"code-length symbol {sym}")
            if cl[sym][1] == 0 or CL_ORDER.index(sym) >= n_cl:
                if not force:
                    raise NoCode(f"code-length symbol {sym} has no code")
            else:
                w.code(*cl[sym])
            if sym == 16:
                w.bits(count - 3, 2)
            elif sym == 17:
                w.bits(count - 3, 3)
            elif sym == 18:
                w.bits(count - 11, 7)
        return n_ll, n_d

    def dynamic(self, symbols, ll_lens, d_lens, final=False, end=True, force=False, **header):
        """a dynamic block: its header (see dynamic_header) and the symbols, coded with the first HLIT + 257 / HDIST + 1 lengths"""
        self.header(final, 2)
        n_ll, n_d = self.dynamic_header(ll_lens, d_lens, force=force, **header)
        self.symbols(list(symbols) + ([END] if end else []), list(ll_lens)[:n_ll], list(d_lens)[:n_d], force)


def model_text(symbols, prefix=b""):
    """the text that `symbols` produce after `prefix`, prefix included, by plain byte copying"""
    t = bytearray(prefix)
    for s in symbols:
        if isinstance(s, int):
            if s == END:
                continue
            t.append(s)
        elif isinstance(s[0], str):
            raise ValueError("a bare symbol has no text")
        else:
            length, dist = s
            if dist > len(t):
                raise ValueError(f"distance {dist} at text position {len(t)}")
            if dist >= length:
                a = len(t) - dist
                t += t[a:a + length]
            else:
                for _ in range(length):
                    t.append(t[-dist])
    return bytes(t)


def bgzf_member(deflate_data, text, crc=None, isize=None):
    """one BGZF member (gzip member whose extra field holds 'B' 'C' 2 BSIZE) around raw deflate data; CRC-32 and ISIZE of
    `text` unless given"""
    total = 12 + 6 + len(deflate_data) + 8
    if total > 65536:
        raise ValueError("a BGZF member holds at most 64 KiB")
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1)
    return head + bytes(deflate_data) + struct.pack("<II", (zlib.crc32(text) & 0xFFFFFFFF) if crc is None else crc, len(text) if isize is None else isize)
