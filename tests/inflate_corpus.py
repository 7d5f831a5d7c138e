"""TEST INFRASTRUCTURE: hand-built DEFLATE streams for every branch of the wave decoder (biolib_amd/csrc/bl_inflate_core.hpp),
made with tests/deflate_writer.py from fixed seeds.  Every class is DESIGNED sound or unsound; zlib (raw inflate, wbits = -15)
is the judge, and judge() must agree with the design for every stream (tests/test_inflate_streams.py asserts it), so that no
class can silently turn into something else than it says.

A record: the class, a name, the raw deflate data, the text size the member states (ISIZE), the design verdict, the expected
text (model_text: plain byte copying) for a sound stream, and the decoder's status code where the cause has one of its own."""
import collections
import random
import struct
import zlib

import numpy as np

import deflate_writer as W

Rec = collections.namedtuple("Rec", "cls name data isize sound text status")

CLASSES = ["match_literal", "match_dependent", "match_block_end", "match_member_end", "flush", "codes", "unsound"]
DISTANCES = list(range(1, 131)) + list(range(255, 260)) + [4096, 16383, 16384, 16385, 32767, 32768]
LENGTHS = list(range(3, 259))
MAX_TEXT = 65536
# bl_inflate::Status
ERR_BLOCK_TYPE, ERR_STORED, ERR_HEADER, ERR_CODE_SET, ERR_SYMBOL, ERR_DISTANCE, ERR_OVERRUN, ERR_INPUT, ERR_SIZE, STATUS_CRC = range(1, 11)


def judge(data, isize):
    """zlib's verdict: (sound, text).  Sound = the end of the final block is reached on the last byte of the data, with
    exactly `isize` bytes of text"""
    z = zlib.decompressobj(wbits=-15)
    try:
        text = z.decompress(bytes(data))
    except zlib.error:
        return False, None
    if not z.eof or z.unused_data or len(text) != isize:
        return False, None
    return True, text


class Member:
    """one deflate stream in the making: blocks of any kind one after the other, and the text they stand for"""

    def __init__(self, seed):
        self.w = W.DeflateWriter()
        self.text = bytearray()
        self.syms = []
        self.rng = np.random.default_rng(seed)

    def noise(self, n):
        return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    _pending = 0  # bytes of text that self.syms (the block in the making) stand for

    def size(self):
        return len(self.text) + self._pending

    def add(self, *symbols):
        for s in symbols:
            self.syms.append(s)
            self._pending += 1 if isinstance(s, int) else s[0]

    def literals(self, n, below=256):
        self.add(*[b % below for b in self.noise(n)])

    def _apply(self):
        apply_symbols(self.text, self.syms)
        self.syms = []
        self._pending = 0

    def end_fixed(self, final=False):
        self.w.fixed(self.syms, final)
        self._apply()

    def end_dynamic(self, ll_lens, d_lens, final=False, **header):
        self.w.dynamic(self.syms, ll_lens, d_lens, final, **header)
        self._apply()

    def stored(self, data, final=False):
        assert not self.syms
        for a in range(0, max(len(data), 1), 65535):
            self.w.stored(data[a:a + 65535], final and a + 65535 >= len(data))
        self.text += data

    def fill_to(self, position):
        """stored noise up to text position `position`"""
        assert not self.syms and position >= len(self.text), (position, len(self.text))
        if position > len(self.text):
            self.stored(self.noise(position - len(self.text)))

    def rec(self, cls, name, sound=True, isize=None, status=0):
        assert not self.syms
        text = bytes(self.text)
        return Rec(cls, name, self.w.getvalue(), len(text) if isize is None else isize, sound, text if sound else None, status)


def apply_symbols(t, symbols):
    """model_text on a bytearray in place (and by slices: tests/test_inflate_streams.py holds it against model_text's byte loop)"""
    for s in symbols:
        if isinstance(s, int):
            if s != W.END:
                t.append(s)
        else:
            length, dist = s
            assert dist <= len(t), (dist, len(t))
            a = len(t) - dist
            if dist >= length:
                t += t[a:a + length]
            else:  # the match runs into itself: its `dist` last bytes, over and over
                t += (bytes(t[a:]) * (length // dist + 1))[:length]


# ---- match copies -------------------------------------------------------------------------------------------------------

def _fresh(m, dist):
    """literals in front of a match so that its source is noise, never a run or a period left by the matches before it"""
    m.literals(min(dist, 24))


def match_records():
    rnd = random.Random(20260)
    for follower in ("literal", "dependent", "block_end"):
        cls, m, n_members = "match_" + follower, None, 0

        def close():
            nonlocal m, n_members
            if m is not None:
                m.end_fixed(final=True)
                n_members += 1
                r = m.rec(cls, f"{cls}#{n_members}")
                m = None
                return r
            return None

        for dist in DISTANCES:
            for length in LENGTHS:
                need = 24 + length + 260
                if m is not None and m.size() + need > MAX_TEXT:
                    yield close()
                if m is None:
                    m = Member(1000 * len(cls) + n_members)
                if m.size() < dist:  # the text so far does not reach back that far: noise in front
                    if dist > 300:
                        if m.syms:
                            m.end_fixed()
                        m.fill_to(dist)
                        if m.size() + need > MAX_TEXT:
                            yield close()
                            m = Member(1000 * len(cls) + n_members)
                            m.fill_to(dist)
                    else:
                        m.literals(dist - m.size())
                _fresh(m, dist)
                m.add((length, dist))
                if follower == "literal":
                    m.literals(1)
                else:
                    # a match whose source lies inside the bytes the first one has just produced
                    if follower == "block_end":
                        m.end_fixed()
                    d2 = rnd.randint(1, length)
                    m.add((rnd.randint(3, 40) if rnd.random() < 0.8 else rnd.randint(3, 258), d2))
        yield close()
    # the match is the member's last symbol: one member per pair
    n = 0
    for dist in DISTANCES:
        for length in LENGTHS:
            m = Member(7_000_000 + n)
            n += 1
            if dist > 300:
                m.fill_to(dist - 8)
                m.literals(8)
            else:
                m.literals(dist)
            m.add((length, dist))
            m.end_fixed(final=True)
            yield m.rec("match_member_end", f"match_member_end D={dist} L={length}")


# ---- flush boundaries ---------------------------------------------------------------------------------------------------

# (length, distance) of each copy path of inflate_member and by how many bytes the match reaches over the boundary
FLUSH_MATCHES = ([("pending", 64, 64, k) for k in (1, 63)] + [("pending", 64, 32768, k) for k in (1, 63)] +
                 [("rounds", 258, 300, k) for k in (1, 63, 64, 65, 257)] + [("rounds", 258, 100, k) for k in (64, 257)] +
                 [("rounds", 65, 32768, k) for k in (1, 64)] +
                 [("run", 258, 1, k) for k in (1, 63, 64, 65, 257)] +
                 [("period", 258, 7, k) for k in (1, 63, 64, 65, 257)] + [("period", 258, 63, k) for k in (1, 65)] + [("period", 258, 2, 64), ("period", 130, 33, 63)])


def _flush_item(m, kind, p, last=False):
    """put `kind` on text position p (a flush boundary seen from the ring, or the text's end when `last`)"""
    what = kind[0]
    if what == "literal":
        m.fill_to(p - 1)
        m.literals(1)
    elif what == "stored":
        m.fill_to(p - 100)
        m.stored(m.noise(100 if last else 200), final=last)
        if last:
            return
    else:
        _, length, dist, over = kind
        if last:
            over = 0
        m.fill_to(p - (length - over) - 16)
        m.literals(16)
        m.add((length, dist))
    if not last:
        m.literals(1)
        m.add((10, 5), (20, 10 + min(kind[3], 200) if len(kind) > 3 else 12))  # reads back over the boundary
    m.end_fixed(final=last)


def flush_records():
    kinds = [("literal",), ("stored",), ("pending_exact", 40, 50, 0), ("pending_straddle", 40, 50, 20)] + FLUSH_MATCHES
    n = 0
    for align in range(16):
        for kind in kinds:
            # one member per kind and alignment: the kind at 16384, 32768 and 49152 (in ring positions: text position + the
            # destination's low four bits), and as the last thing of a text that ends on 65536
            m = Member(8_000_000 + n)
            n += 1
            for boundary in (16384, 32768, 49152):
                if len(kind) > 2 and kind[2] > boundary - 600:
                    continue  # (a distance of 32768 needs that much text first)
                _flush_item(m, kind, boundary - align)
            _flush_item(m, kind, 65536 - align, last=True)
            yield m.rec("flush", f"flush align={align} {kind}")
        # text that ends exactly on a boundary, its last symbol a literal, a match, a stored byte
        for boundary in (16384, 32768, 49152):
            for kind in (("literal",), ("stored",), ("pending", 40, 50, 0), ("rounds", 258, 300, 0), ("period", 258, 7, 0)):
                m = Member(8_500_000 + n)
                n += 1
                _flush_item(m, kind, boundary - align, last=True)
                yield m.rec("flush", f"flush text ends on {boundary} align={align} {kind}")
    for isize in (65536, 65535, 49153, 16385, 16384, 16383, 17, 16, 15, 1, 0):
        for how in range(3):
            m = Member(8_900_000 + 3 * isize + how)
            if how == 0:  # stored, then fixed
                m.stored(m.noise(isize // 2))
                m.literals(min(isize - isize // 2, 40))
                while m.size() < isize:
                    m.add((min(258, isize - m.size()), 1 + (m.size() * 7) % min(m.size(), 32768))) if isize - m.size() >= 3 else m.literals(1)
                m.end_fixed(final=True)
            elif how == 1:  # fixed, then stored
                m.literals(min(isize // 3, 50))
                while isize // 3 - m.size() >= 3:
                    m.add((min(258, isize // 3 - m.size()), 1 + (m.size() * 5 + 3) % m.size()))
                m.end_fixed()
                m.stored(m.noise(isize - m.size()), final=True)
            else:  # one stored block (two for 65536: LEN has 16 bits)
                m.stored(m.noise(isize), final=True)
            yield m.rec("flush", f"flush isize={isize} how={how}")


# ---- code sets ----------------------------------------------------------------------------------------------------------

def _complete(n_symbols, short):
    """code lengths of a complete code over n symbols that uses two lengths: `short` and short + 1"""
    x = (1 << (short + 1)) - n_symbols  # x + y = n, 2 x + y = 2^(short + 1)
    assert 0 <= x <= n_symbols
    return [short] * x + [short + 1] * (n_symbols - x)


def code_records():
    cls = "codes"
    staircase = list(range(1, 16)) + [15]  # 1, 2, ..., 14, 15, 15: complete, the longest there is
    ll_used = [65, 66, 67, 68, 69, 70, 71, 72, 256, 257, 260, 265, 270, 277, 284, 285]
    d_used = [0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 26, 29]
    for rot in range(16):
        m = Member(9_000_000 + rot)
        m.fill_to(32768)
        ll_lens, d_lens = [0] * 286, [0] * 30
        for i, s in enumerate(ll_used):
            ll_lens[s] = staircase[(i + rot) % 16]
        for i, s in enumerate(d_used):
            d_lens[s] = staircase[(i + 2 * rot + 3) % 16]
        for rep in range(3):
            for i in range(16):
                s, ds = ll_used[(i + rep) % 16], d_used[(5 * i + rep) % 16]
                if s < 256:
                    m.add(s)
                elif s > 256:
                    c = s - 257
                    for x in (0, (1 << W.LEN_EXTRA[c]) - 1):
                        for dx in (0, (1 << W.DIST_EXTRA[ds]) - 1):
                            m.add((W.LEN_BASE[c] + x, W.DIST_BASE[ds] + dx))
            for ds in d_used:  # every distance code, long ones included
                m.add((3, W.DIST_BASE[ds]), 65 + ds % 8)
        m.end_dynamic(ll_lens, d_lens, final=True)
        yield m.rec(cls, f"codes staircase rot={rot}")
    # all 286 / 30 symbols coded; every length base and every extra-bits value at its minimum and maximum
    for variant in range(4):
        m = Member(9_100_000 + variant)
        m.fill_to(32768)
        rnd = random.Random(variant)
        ll_lens, d_lens = _complete(286, 8), _complete(30, 4)
        if variant:
            rnd.shuffle(ll_lens)
            rnd.shuffle(d_lens)
        m.add(*range(256))
        for c in range(29):
            for x in (0, (1 << W.LEN_EXTRA[c]) - 1):
                ds = (c + variant) % 30
                m.add((W.LEN_BASE[c] + x, W.DIST_BASE[ds] + x % (1 << W.DIST_EXTRA[ds])), rnd.randrange(256))
        for ds in range(30):
            for x in (0, (1 << W.DIST_EXTRA[ds]) - 1):
                m.add((3 + (ds + x) % 9, W.DIST_BASE[ds] + x), rnd.randrange(256))
        m.end_dynamic(ll_lens, d_lens, final=True)
        yield m.rec(cls, f"codes all symbols variant={variant}")
    # HLIT = 0: literals and the end-of-block code only; no distance code at all (one length of 0, and thirty)
    for n_d in (1, 30):
        m = Member(9_200_000 + n_d)
        m.literals(3000)
        ll_lens = _complete(257, 8)
        m.end_dynamic(ll_lens, [0] * n_d, final=True, hlit=0, hdist=n_d - 1)
        yield m.rec(cls, f"codes HLIT=0, no distance code, HDIST={n_d - 1}")
    # one distance code of one bit, as symbol 0 and as symbol 29
    for ds in (0, 29):
        m = Member(9_300_000 + ds)
        m.fill_to(32768)
        ll_lens = _complete(286, 8)
        for x in (0, (1 << W.DIST_EXTRA[ds]) - 1, 1 if ds else 0):
            m.literals(5)
            m.add((3, W.DIST_BASE[ds] + x), (258, W.DIST_BASE[ds] + x), (64, W.DIST_BASE[ds] + x))
        m.end_dynamic(ll_lens, [0] * ds + [1], final=True)
        yield m.rec(cls, f"codes lone distance code, symbol {ds}")
    # a literal/length code that holds the end-of-block code alone, one bit long: an empty block (after text, and on its own)
    for with_text in (0, 1):
        m = Member(9_400_000 + with_text)
        if with_text:
            m.literals(100)
            m.end_fixed()
        m.end_dynamic([0] * 256 + [1], [0], final=True)
        yield m.rec(cls, f"codes lone end-of-block code, text={with_text}")
    # code-length repeats that run from the literal/length lengths into the distance lengths
    ll_base = [8] * 252 + [0] * 4 + [8] * 4  # 256 codes of 8 bits; lengths 3..5 coded (symbols 257..259)
    n = 0
    for sym in (16, 17, 18):
        if sym == 16:
            n_ll, d_lens = 260, [8, 8, 8, 8, 1, 2, 3, 4, 5, 6]
            spans = [(j, k) for k in range(3, 7) for j in range(1, 4) if 1 <= k - j <= 4]
        elif sym == 17:
            n_ll, d_lens = 265, [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 8, 8, 8, 8]
            spans = [(j, k) for k in range(3, 11) for j in range(1, 6) if 1 <= k - j <= 4]
        else:
            n_ll, d_lens = 286, [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 8, 8, 8, 8]
            spans = [(j, k) for k in range(11, 31) for j in range(7, 27) if 1 <= k - j <= 4]
        ll_lens = (ll_base + [0] * 26)[:n_ll]
        for j, k in spans:  # j lengths of the repeat are literal/length lengths, k - j are distance lengths
            both = ll_lens + d_lens
            a = n_ll - j
            assert len(set(both[a - (sym == 16):a + k])) == 1
            stream = W.rle_cl_stream(both[:a]) + [(sym, k)] + W.plain_cl_stream(both[a + k:])
            assert W.cl_stream_length(stream) == len(both)
            m = Member(9_500_000 + n)
            n += 1
            m.literals(300, below=252)
            for ds, dl in enumerate(d_lens):  # every distance code is used: a length put in the wrong slot changes the text
                if dl:
                    m.add((3 + ds % 3, W.DIST_BASE[ds]), 7 * ds)
            m.end_dynamic(ll_lens, d_lens, final=True, hlit=n_ll - 257, hdist=len(d_lens) - 1, cl_stream=stream)
            yield m.rec(cls, f"codes repeat {sym} over the boundary: {j} + {k - j}")
    # HCLEN: all 19 lengths of the code-length code sent, and the fewest that can describe a code (8: lengths 0, 6..9;
    # with 4 only the repeats and 0 have codes, every length is 0 and there is no end-of-block code: see the unsound class)
    m = Member(9_600_000)
    m.literals(500)
    m.add((100, 7), (258, 400))
    cl19 = [4] * 19
    for s in (1, 15, 14):
        cl19[s] = 5
    cl19[2] = cl19[13] = 5
    cl19[3] = 5  # 13 of 4 bits, 6 of 5
    assert W.kraft(cl19) == 32768 and cl19[15]
    m.end_dynamic(_complete(286, 8), _complete(30, 4), final=True, cl_lens=cl19, hclen=15)
    yield m.rec(cls, "codes HCLEN: 19 lengths")
    m = Member(9_600_001)
    m.literals(600, below=252)
    cl8 = [0] * 19
    for s in (16, 17, 18, 0, 8, 7, 9, 6):
        cl8[s] = 3
    m.end_dynamic(ll_base, [0], final=True, cl_lens=cl8, hclen=4)
    yield m.rec(cls, "codes HCLEN field 4: 8 lengths")
    # many tiny blocks: stored, fixed and dynamic in turn, an empty stored block between them (what a sync flush leaves), and
    # an empty final block behind a text that is already complete
    for final_kind in range(3):
        m = Member(9_700_000 + final_kind)
        ll_lens, d_lens = _complete(286, 8), _complete(30, 4)
        for i in range(120):
            kind = i % 3
            if kind == 0:
                m.stored(m.noise(1 + i % 5))
            else:
                m.literals(1 + i % 4)
                if m.size() > 10:
                    m.add((3 + i % 70, 1 + i % 9))
                m.end_fixed() if kind == 1 else m.end_dynamic(ll_lens, d_lens)
            m.stored(b"")
        if final_kind == 0:
            m.stored(b"", final=True)
        elif final_kind == 1:
            m.end_fixed(final=True)
        else:
            m.end_dynamic([0] * 256 + [1], [0], final=True)
        yield m.rec(cls, f"codes 120 tiny blocks, empty final block of type {final_kind}")


# ---- unsound by construction --------------------------------------------------------------------------------------------

def unsound_records():
    cls = "unsound"
    flat_ll, flat_d = _complete(286, 8), _complete(30, 4)

    def bad(name, data, isize, status=0):
        return Rec(cls, name, bytes(data), isize, False, None, status)

    def some_text(m, n=40):
        m.literals(n)
        m.add((9, 3), (70, 33))

    # reserved block type, first and after a sound block
    w = W.DeflateWriter()
    w.header(True, 3)
    w.w.bits(0x5A5A, 16)
    yield bad("block type 3", w.getvalue(), 0, ERR_BLOCK_TYPE)
    m = Member(1)
    some_text(m)
    m.end_fixed()
    m.w.header(True, 3)
    m.w.w.bits(0, 13)
    yield bad("block type 3 after a fixed block", m.w.getvalue(), len(m.text), ERR_BLOCK_TYPE)
    # stored: NLEN is not ~LEN; LEN beyond the stated size
    for nlen in (0, 10, 0xFFF4):
        w = W.DeflateWriter()
        w.stored(b"0123456789", True, nlen=nlen)
        yield bad(f"stored NLEN={nlen:#x}", w.getvalue(), 10, ERR_STORED)
    for isize in (9, 0):
        w = W.DeflateWriter()
        w.stored(b"0123456789", True)
        yield bad(f"stored LEN 10, ISIZE {isize}", w.getvalue(), isize, ERR_OVERRUN)
    # HLIT / HDIST beyond 286 / 30 codes
    for hlit, hdist in ((29, 29), (30, 29), (31, 29), (29, 30), (29, 31), (31, 31)):
        m = Member(2)
        m.literals(40)
        m.add((9, 3), (70, 2))
        ll_lens, d_lens = (flat_ll + [0, 0])[:hlit + 257], (flat_d + [0, 0])[:hdist + 1]
        m.end_dynamic(ll_lens, d_lens, final=True, hlit=hlit, hdist=hdist)
        if (hlit, hdist) == (29, 29):
            yield m.rec("codes", "codes HLIT=29 HDIST=29 (the most there may be)")
        else:
            yield bad(f"HLIT={hlit} HDIST={hdist}", m.w.getvalue(), len(m.text))
    # the code-length stream: a repeat of the previous length with nothing before it, repeats that overrun, no end-of-block code
    both = flat_ll + flat_d
    streams = {"repeat 16 comes first": [(16, 3)] + both[3:], "repeat 16 overruns": both[:-2] + [(16, 3)], "repeat 17 overruns": both[:-1] + [(17, 3)],
               "repeat 18 overruns": both[:-10] + [(18, 11)], "repeat 18 overruns by 128": both[:-10] + [(18, 138)], "a length too many": both + [5]}
    for name, stream in streams.items():
        m = Member(3)
        some_text(m)
        m.end_dynamic(flat_ll, flat_d, final=True, cl_stream=stream)
        yield bad(name, m.w.getvalue(), len(m.text))
    ll = list(flat_ll)
    ll[256] = 0
    ll[285] = 0  # (two 9-bit codes fewer would be incomplete as well; the missing end-of-block code is looked at first)
    m = Member(4)
    m.literals(40)
    m.w.dynamic(m.syms, ll, flat_d, True, end=False)
    yield bad("no end-of-block code", m.w.getvalue(), 40)
    ll = [0] * 286
    for s in range(128):
        ll[s] = 7  # complete without symbol 256
    m = Member(4)
    m.literals(40, below=128)
    m.w.dynamic(m.syms, ll, flat_d, True, end=False)
    yield bad("complete code, no end-of-block code", m.w.getvalue(), 40)
    m = Member(4)
    m.w.dynamic([], [0] * 257, [0], True, end=False, cl_lens=[2 if s in (16, 17, 18, 0) else 0 for s in range(19)], hclen=0)
    yield bad("HCLEN field 0: every length is 0", m.w.getvalue(), 0)
    # over-subscribed and incomplete sets, each of the three codes on its own
    cl_over, cl_under, cl_lone = [3] * 19, list(W.CL_ALL), [0] * 19
    cl_under[18] = 0
    cl_lone[8] = 1
    sets = [("code-length code over-subscribed", flat_ll, flat_d, dict(cl_lens=cl_over)),
            ("code-length code incomplete", flat_ll, [4] * 16, dict(cl_lens=cl_under, cl_stream=flat_ll + [4] * 16)),
            ("code-length code of one 1-bit code", [8] * 256 + [8], [8], dict(cl_lens=cl_lone, cl_stream=[8] * 258)),
            ("literal/length code over-subscribed", [8] * 257, flat_d, {}),
            ("literal/length code over-subscribed by a short code", [1, 1] + [0] * 254 + [1], flat_d, {}),
            ("literal/length code incomplete", [8] * 252 + [0] * 4 + [8] * 3, flat_d, {}),
            ("literal/length code: lone end-of-block code of 2 bits", [0] * 256 + [2], flat_d, {}),
            ("literal/length code: two codes of 2 bits", [2] + [0] * 255 + [2], flat_d, {}),
            ("distance code over-subscribed", flat_ll, [1, 1, 1], {}),
            ("distance code over-subscribed, long", flat_ll, [4] * 17, {}),
            ("distance code incomplete", flat_ll, [2, 2, 2], {}),
            ("distance code incomplete: lone code of 2 bits", flat_ll, [2], {}),
            ("distance code incomplete: lone code of 15 bits", flat_ll, [0] * 29 + [15], {}),
            ("distance code incomplete: 1 and 2 bits", flat_ll, [1, 0, 0, 2], {}),
            ("distance code incomplete: 29 of 5 bits", flat_ll, [5] * 29, {})]
    for name, ll_lens, d_lens, header in sets:
        m = Member(5)
        m.w.dynamic([ll_lens.index(max(ll_lens))] * 3, ll_lens, d_lens, True, **header)
        yield bad(name, m.w.getvalue(), 3)
    # reserved symbols of the fixed codes
    for name, syms in (("literal/length symbol 286", [("ll", 286)]), ("literal/length symbol 287", [("ll", 287)]),
                       ("distance symbol 30", [("ll", 257), ("d", 30)]), ("distance symbol 31", [("ll", 285), ("d", 31)])):
        m = Member(6)
        m.literals(50)
        m.w.fixed(m.syms + syms + [65, 66], True)
        yield bad(name + " in a fixed block", m.w.getvalue(), 55)
    # a match where there is no distance code (its length is sent, its distance cannot be); the unused half of a lone 1-bit code
    m = Member(7)
    m.literals(50)
    m.w.dynamic(m.syms + [(5, 1), 65, 66, 67], flat_ll, [0], True, force=True)
    yield bad("match with no distance code", m.w.getvalue(), 58)
    m = Member(7)
    m.literals(50)
    m.w.header(True, 2)
    m.w.dynamic_header(flat_ll, [1])
    m.w.symbols(m.syms + [("ll", 257)], flat_ll, [1])
    m.w.w.bits(1, 1)  # the other codeword of one bit: no symbol
    m.w.symbols([65, W.END], flat_ll, [1])
    yield bad("lone distance code: the codeword that is not in use", m.w.getvalue(), 54)
    # a distance one beyond the text so far (at 32768 bytes of text every distance there is reaches text: 32767 is the last
    # position at which one can be beyond)
    for pos, dist in ((0, 1), (1, 2), (1, 32768), (100, 101), (32767, 32768), (300, 16385)):
        m = Member(8)
        if pos > 300:
            m.fill_to(pos)
        else:
            m.literals(pos)
            m.end_fixed()
        m.w.fixed([(3, dist), 65], True)
        yield bad(f"distance {dist} at text position {pos}", m.w.getvalue(), pos + 4, ERR_DISTANCE)
    # text one byte longer / shorter than the stated size, ended by a literal, by a match, by a stored block; wrong ISIZE
    for last in ("literal", "pending match", "long match", "run", "stored"):
        tail = {"literal": 2, "pending match": 4, "long match": 200, "run": 70, "stored": 5}[last]
        for base in (60, 16384 - 7, 65537 - tail):  # (the last: one byte more than a member may hold)
            m = Member(9)
            m.fill_to(base - 59)
            m.literals(59)
            if last == "literal":
                m.literals(2)
                m.end_fixed(final=True)
            elif last == "stored":
                m.end_fixed()
                m.stored(m.noise(5), final=True)
            else:
                m.add({"pending match": (4, 9), "long match": (200, 40), "run": (70, 1)}[last])
                m.end_fixed(final=True)
            n = len(m.text)
            if n + 1 <= MAX_TEXT:
                yield bad(f"text of {n} bytes ended by a {last}, ISIZE one more", m.w.getvalue(), n + 1, ERR_SIZE)
            yield bad(f"text of {n} bytes ended by a {last}, ISIZE one less", m.w.getvalue(), n - 1, ERR_OVERRUN)
            if base == 60:
                yield bad(f"text of {n} bytes ended by a {last}, ISIZE 0", m.w.getvalue(), 0, ERR_OVERRUN)
                yield bad(f"text of {n} bytes ended by a {last}, ISIZE 65536", m.w.getvalue(), 65536, ERR_SIZE)
    # data cut inside a symbol, inside extra bits, inside a stored block, inside a dynamic header; src_len one byte short
    m = Member(10)
    m.literals(20)
    m.add((258, 5), (162, 17), (3, 280))  # extra bits: none, 5 for the length, 7 for the distance
    m.end_fixed(final=True)
    whole = m.w.getvalue()
    for cut in range(1, len(whole)):
        yield bad(f"fixed block cut to {cut} of {len(whole)} bytes", whole[:cut], len(m.text))
    w = W.DeflateWriter()
    w.stored(b"x" * 4200)
    w.fixed([65] * 30 + [(193, 4097)], True)  # 5 + 11 extra bits
    whole = w.getvalue()
    for cut in (len(whole) - 1, len(whole) - 2, len(whole) - 3, 4205 + 30, 4205, 4204, 2000, 5, 4, 3, 2, 1):
        yield bad(f"stored + fixed cut to {cut} of {len(whole)} bytes", whole[:cut], 4200 + 30 + 193)
    m = Member(12)
    some_text(m, 300)
    m.end_dynamic(flat_ll, flat_d, final=True)
    whole = m.w.getvalue()
    for cut in list(range(1, 80, 3)) + [len(whole) - 1, len(whole) - 2]:
        yield bad(f"dynamic block cut to {cut} of {len(whole)} bytes", whole[:cut], len(m.text))
    w = W.DeflateWriter()
    w.stored(b"abcdefgh", True)
    yield bad("stored block one byte short", w.getvalue()[:-1], 8)
    # a dynamic code whose all-zero codeword is a literal, on data that ends early: the zeros behind the data are literals
    # without end, and the decoder has to stop on the text bound or on the input bound
    ll = [0] * 286
    ll[65], ll[66], ll[256] = 1, 2, 2
    for isize in (50, 4000, 65536):
        for n_lit in (10, 2000):
            m = Member(13)
            m.w.dynamic([65, 66] * (n_lit // 2), ll, [0], True, end=False)
            yield bad(f"all-zero codeword is a literal, data ends after {n_lit} literals, ISIZE {isize}", m.w.getvalue(), isize)


def corpus():
    """every record, class by class"""
    for gen in (match_records, flush_records, code_records, unsound_records):
        for r in gen():
            if r is not None:
                yield r


def write_corpus_file(records, path):
    records = list(records)
    assert all(r.isize <= MAX_TEXT and (not r.sound or len(r.text) == r.isize) for r in records)
    """the file tests/emu/emu_inflate.cpp --corpus reads: per record six little-endian dwords (bytes of data, stated size, 1 =
    sound, expected status or 0, bytes of text, index of the class), the data, the text"""
    with open(path, "wb") as f:
        f.write(b"BLINFLC1")
        for r in records:
            text = r.text if r.sound else b""
            f.write(struct.pack("<6I", len(r.data), r.isize, 1 if r.sound else 0, r.status, len(text), CLASSES.index(r.cls)))
            f.write(r.data)
            f.write(text)
