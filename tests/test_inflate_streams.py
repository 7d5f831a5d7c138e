"""The inflate kernel on streams whose symbols the TEST chose (tests/deflate_writer.py, tests/inflate_corpus.py): every match-copy
path at every (distance, length) with every kind of follower, every flush boundary at every destination alignment, code sets
at the limits of the format, and streams that are unsound by construction.  zlib is the judge of every stream.

CPU: the writer against zlib, the design of every stream against zlib's verdict, and the whole corpus through the host build of
the decoder under the sanitizers, at the destination misalignments 0..15 (tests/emu/emu_inflate.cpp --corpus).
GPU: the same streams through bl_bgzf_inflate with a member table of the test's own: data at every src_off & 3, texts at every
dst_off & 15 between guard bytes, the last member's data on the last byte of the packed buffer, sound and unsound members side
by side in one launch; and the CRC-32 kernel on stored members of every small size."""
import ctypes as C
import functools
import gzip
import os
import random
import subprocess
import time
import zlib

import numpy as np
import pytest

import deflate_writer as W
import inflate_corpus as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 48


@functools.lru_cache(maxsize=1)
def corpus():
    return tuple(IC.corpus())


def class_table(records):
    """per class: streams, accepted by zlib, refused by zlib"""
    table = {c: [0, 0, 0] for c in IC.CLASSES}
    for r in records:
        ok = IC.judge(r.data, r.isize)[0]
        table[r.cls][0] += 1
        table[r.cls][1 if ok else 2] += 1
    return table


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_writer_vs_zlib():
    """the writer's own parts: bit order, the fixed and dynamic codes, stored blocks, the code-length stream, the refusal of a
    symbol without a code, the BGZF wrapper — each against zlib or against the RFC's own example"""
    # RFC 1951 §3.2.2: lengths (3, 3, 3, 3, 3, 2, 4, 4) give the codes 010 011 100 101 110 00 1110 1111
    assert W.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    w = W.BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)      # final fixed block
    w.code(0x30 + 0x41, 8)  # literal 'A': 8-bit codes of literals 0..143 start at 00110000
    w.code(0, 7)      # end of block
    assert zlib.decompress(w.getvalue(), -15) == b"A"
    assert [W.length_symbol(n) for n in (3, 10, 11, 12, 257, 258)] == [(257, 0, 0), (264, 0, 0), (265, 1, 0), (265, 1, 1), (284, 5, 30), (285, 0, 0)]
    assert [W.distance_symbol(d) for d in (1, 4, 5, 6, 24577, 32768)] == [(0, 0, 0), (3, 0, 0), (4, 1, 0), (4, 1, 1), (29, 13, 0), (29, 13, 8191)]
    assert W.kraft(W.FIXED_LL) == 32768 and W.kraft(W.FIXED_D) == 32768 and W.kraft(W.CL_ALL) == 32768
    rnd = random.Random(5)
    for case in range(300):
        symbols, size = [], 0
        for _ in range(rnd.randint(0, 200)):
            if size and rnd.random() < 0.5:
                s = (rnd.choice((3, 4, 10, 11, 64, 65, 257, 258, rnd.randint(3, 258))), rnd.choice((1, min(2, size), size, rnd.randint(1, size))))
                if s[1] > 32768:
                    continue
                size += s[0]
            else:
                s = rnd.randrange(256)
                size += 1
            symbols.append(s)
        text = W.model_text(symbols)
        t = bytearray()
        IC.apply_symbols(t, symbols)
        assert bytes(t) == text and len(text) == size
        w = W.DeflateWriter()
        if case % 3 == 0:
            w.fixed(symbols, True)
        elif case % 3 == 1:  # a dynamic block over all symbols, then the same symbols again after a stored block
            w.dynamic(symbols, IC._complete(286, 8), IC._complete(30, 4), False)
            w.stored(b"between")
            w.fixed(symbols, True)
            text = W.model_text(symbols, W.model_text(symbols) + b"between")
        else:  # any complete code is a code: the two lengths of each dealt out at random, sent one by one
            ll, d = IC._complete(286, 8), IC._complete(30, 4)
            rnd.shuffle(ll)
            rnd.shuffle(d)
            w.dynamic(symbols, ll, d, True, cl_stream=W.plain_cl_stream(ll + d))
        sound, got = IC.judge(w.getvalue(), len(text))
        assert sound and got == text, case
    # the code-length stream: repeats stand for what they say
    for lens in ([0] * 300, [8] * 7 + [0] * 2 + [5] * 3 + [0] * 139 + [7], [1, 2, 3] * 50):
        stream = W.rle_cl_stream(lens)
        flat = []
        for s in stream:
            if isinstance(s, int):
                flat.append(s)
            else:
                assert (s[0] == 16 and 3 <= s[1] <= 6 and flat) or (s[0] == 17 and 3 <= s[1] <= 10) or (s[0] == 18 and 11 <= s[1] <= 138)
                flat += [flat[-1] if s[0] == 16 else 0] * s[1]
        assert flat == lens and W.cl_stream_length(stream) == len(lens)
    # a symbol without a code is refused; forced, it leaves a stream zlib refuses
    for symbols, ll, d in (([65], [0] * 66 + [1] + [0] * 189 + [1], [1]), ([(3, 1)], W.FIXED_LL, [0]), ([(3, 5)], W.FIXED_LL, [1, 1]), ([300], W.FIXED_LL, W.FIXED_D)):
        with pytest.raises((W.NoCode, ValueError)):
            W.DeflateWriter().symbols(symbols, ll, d)
    with pytest.raises(W.NoCode):
        flat = IC._complete(286, 8)
        W.DeflateWriter().dynamic([65], flat, [1], cl_lens=[0] * 8 + [1, 1] + [0] * 9, cl_stream=flat + [1])  # lengths 8 and 9 have codes, 1 has none
    w = W.DeflateWriter()
    w.dynamic([65, (5, 1), 66], IC._complete(286, 8), [0], True, force=True)
    assert not IC.judge(w.getvalue(), 7)[0]
    # stored blocks; wrong NLEN; the BGZF wrapper
    w = W.DeflateWriter()
    w.fixed([65], False)
    w.stored(b"hello")
    w.stored(b"", True)
    assert IC.judge(w.getvalue(), 6) == (True, b"Ahello")
    w = W.DeflateWriter()
    w.stored(b"hello", True, nlen=0)
    assert not IC.judge(w.getvalue(), 5)[0]
    member = W.bgzf_member(w.getvalue(), b"hello")
    assert member[12:14] == b"BC" and int.from_bytes(member[16:18], "little") == len(member) - 1
    w = W.DeflateWriter()
    w.stored(b"hello", True)
    assert gzip.decompress(W.bgzf_member(w.getvalue(), b"hello")) == b"hello"
    with pytest.raises((OSError, EOFError, zlib.error)):
        gzip.decompress(W.bgzf_member(w.getvalue(), b"hello", crc=zlib.crc32(b"hello") ^ 1))


def test_corpus_design_is_zlibs_verdict():
    """every stream is what its class says: zlib accepts the sound ones, with the model's text, and refuses the others"""
    t0 = time.perf_counter()
    records = corpus()
    for r in records:
        sound, text = IC.judge(r.data, r.isize)
        assert sound == r.sound, (r.cls, r.name, "zlib:", sound)
        assert r.isize <= 65536 and len(r.data) >= 1
        if sound:
            assert text == r.text, (r.cls, r.name)
        elif r.status:
            assert 1 <= r.status <= 9
    table = class_table(records)
    print("\nclass: streams, accepted by zlib, refused by zlib")
    for c in IC.CLASSES:
        print(f"  {c}: {table[c][0]}, {table[c][1]}, {table[c][2]}")
    print(f"  corpus built and judged in {time.perf_counter() - t0:.1f} s")
    assert all(table[c][0] for c in IC.CLASSES)
    # every (distance, length) with each of the four followers
    assert len(IC.DISTANCES) == 141 and len(IC.LENGTHS) == 256
    assert table["match_member_end"][0] == 141 * 256 and table["unsound"][1] == 0
    assert sum(table[c][2] for c in IC.CLASSES if c != "unsound") == 0


def test_corpus_through_host_decoder(tmp_path):
    """the host build of the decoder, address + undefined-behaviour sanitizers on: every stream at the destination
    misalignments 0..15 — status (the cause's own code where it has one), text, and nothing written around the text"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
    exe = os.path.join(ROOT, "tests", "emu", "_build", "emu_inflate")
    path = str(tmp_path / "corpus.bin")
    records = corpus()
    IC.write_corpus_file(records, path)
    t0 = time.perf_counter()
    shards = max(1, min(8, len(os.sched_getaffinity(0))))
    procs = [subprocess.Popen([exe, "--corpus", path, str(i), str(shards)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for i in range(shards)]
    outs = [p.communicate(timeout=3000)[0] for p in procs]
    print(f"\n{len(records)} streams x 16 misalignments through the host decoder in {time.perf_counter() - t0:.1f} s")
    done = 0
    for p, out in zip(procs, outs):
        assert p.returncode == 0 and "emu_inflate: OK" in out, out[-3000:]
        done += int(out.split("corpus records ")[1].split()[0])
    assert done == len(records)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

class Entry:
    __slots__ = ("data", "isize", "crc", "text", "status", "name")

    def __init__(self, data, isize, crc, text, status, name):
        self.data, self.isize, self.crc, self.text, self.status, self.name = data, isize, crc, text, status, name


def device_entries():
    """the corpus as members (sound: status 0 and the text; unsound: any status but 0, or the cause's own), and some of its
    sound streams with one bit of the CRC-32 wrong (status 10)"""
    out = []
    for i, r in enumerate(corpus()):
        if r.sound:
            out.append(Entry(r.data, r.isize, zlib.crc32(r.text), r.text, 0, r.name))
            if i % 97 == 0 or r.cls in ("codes",):
                out.append(Entry(r.data, r.isize, zlib.crc32(r.text) ^ (1 << (i % 32)), None, IC.STATUS_CRC, r.name + ", CRC-32 wrong in one bit"))
        else:
            out.append(Entry(r.data, r.isize, 0x12345678, None, r.status or -1, r.name))
    return out


def crc_entries():
    """the CRC-32 kernel alone: stored members of random bytes of every small size, around 4096 and at the limit, each with the
    right CRC-32 and with a wrong one"""
    rng = np.random.default_rng(31)
    out = []
    for n in list(range(0, 131)) + [4095, 4096, 4097, 65535, 65536]:
        text = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        m = IC.Member(0)
        m.stored(text, final=True)
        crc = zlib.crc32(text)
        out.append(Entry(m.w.getvalue(), n, crc, text, 0, f"stored {n} bytes"))
        out.append(Entry(m.w.getvalue(), n, crc ^ (1 << (n % 32)), None, IC.STATUS_CRC, f"stored {n} bytes, CRC-32 wrong in one bit"))
        out.append(Entry(m.w.getvalue(), n, (crc + 0x01010101) & 0xFFFFFFFF, None, IC.STATUS_CRC, f"stored {n} bytes, CRC-32 wrong"))
    return out


def run_on_device(ctx, entries, turn, align_of=None, long_members=True):
    """one launch over `entries` in an order of the turn's own: member i's data starts at src_off & 3 = (i + turn) & 3 behind
    noise, its text at dst_off & 15 = (what align_of says, or i) + 5 * turn, GUARD bytes of 0xA5 on either side; packed_bytes is
    turn mod 4 (mod 4) and the last member's data ends on its last byte.  Checks every status, every sound text, every byte that
    belongs to no member's text."""
    lib, h = ctx._lib, ctx._h
    order = list(range(len(entries)))
    random.Random(turn).shuffle(order)
    # the last member: sound, with all of its data needed (a stored block at its end) — the longest such
    last = max((i for i in order if entries[i].status == 0), key=lambda i: len(entries[i].data) if entries[i].name.startswith("flush isize=65536 how=2") else 0)
    order.remove(last)
    order.append(last)
    n = len(order)
    noise = np.random.default_rng(turn).integers(0, 256, 8, dtype=np.uint8).tobytes()
    members = np.zeros((n, 4), np.uint64)
    packed, text_at = bytearray(), 0
    dst_offs = []
    for j, i in enumerate(order):
        e = entries[i]
        lead = (j + turn) & 3
        if j == n - 1:  # the total comes out as turn mod 4
            lead = (turn - len(e.data)) & 3
        packed += noise[:(lead - len(packed)) & 3]
        align = ((align_of[i] if align_of and align_of[i] is not None else j) + 5 * turn) & 15
        text_at += GUARD
        text_at += (align - text_at) & 15
        members[j] = (len(packed), text_at, len(e.data) | (e.isize << 32), e.crc & 0xFFFFFFFF)
        dst_offs.append(text_at)
        packed += e.data
        text_at += e.isize
    text_bytes = text_at + GUARD
    packed_bytes = len(packed)
    assert packed_bytes & 3 == turn & 3 and int(members[-1, 0]) + len(entries[order[-1]].data) == packed_bytes
    src_offs = members[:, 0].astype(np.int64)
    sizes = np.array([len(entries[i].data) for i in order])
    sound = np.array([entries[i].status == 0 for i in order])
    for lead in range(4 if long_members else 0):  # a sound member beyond one 64-dword chunk (and its prefetch) at every lead
        assert ((src_offs & 3 == lead) & sound & (sizes > 1024)).any()
    assert len(set(np.array(dst_offs)[sound] & 15)) == 16
    assert (sound[1:] != sound[:-1]).sum() >= min(100, (~sound).sum())  # sound and unsound members are neighbours
    alloc = (packed_bytes + 3) & ~3  # whole dwords, and not a byte more
    ptrs = []
    try:
        for size in (alloc, 32 * n, text_bytes, 4 * n):
            p = C.c_void_p()
            assert lib.bl_device_alloc(h, size, C.byref(p)) == 0
            ptrs.append(p)
        d_packed, d_members, d_text, d_status = ptrs
        assert d_text.value % 256 == 0 and d_packed.value % 4 == 0
        host_text = np.full(text_bytes, 0xA5, np.uint8)
        assert lib.bl_copy_to_device(h, d_packed, bytes(packed) + b"\0" * (alloc - packed_bytes), alloc) == 0
        assert lib.bl_copy_to_device(h, d_members, members.ctypes.data, 32 * n) == 0
        assert lib.bl_copy_to_device(h, d_text, host_text.ctypes.data, text_bytes) == 0
        status = np.full(n, 0xFFFFFFFF, np.uint32)
        assert lib.bl_copy_to_device(h, d_status, status.ctypes.data, 4 * n) == 0
        ctx.sync()
        t0 = time.perf_counter()
        assert lib.bl_bgzf_inflate(h, d_packed, packed_bytes, d_members, n, d_text, text_bytes, d_status) == 0
        ctx.sync()
        kernel_s = time.perf_counter() - t0
        assert lib.bl_copy_to_host(h, status.ctypes.data, d_status, 4 * n) == 0
        assert lib.bl_copy_to_host(h, host_text.ctypes.data, d_text, text_bytes) == 0
    finally:
        for p in ptrs:
            lib.bl_device_free(h, p)
    inside = np.zeros(text_bytes, bool)
    wrong = []
    for j, i in enumerate(order):
        e, a = entries[i], dst_offs[j]
        inside[a:a + e.isize] = True
        st = int(status[j])
        if e.status == 0:
            if st != 0:
                wrong.append((e.name, "sound, status", st))
            elif host_text[a:a + e.isize].tobytes() != e.text:
                wrong.append((e.name, "text differs, dst_off & 15 =", a & 15, "src_off & 3 =", int(src_offs[j]) & 3))
        elif st == 0 or (e.status > 0 and st != e.status):
            wrong.append((e.name, "unsound, status", st, "expected", e.status))
    assert not wrong, (len(wrong), wrong[:10])
    outside = host_text[~inside]
    assert len(outside) >= GUARD * (n + 1) and (outside == 0xA5).all(), f"{int((outside != 0xA5).sum())} bytes written outside the members' texts"
    return kernel_s, n, packed_bytes, int(inside.sum())


@pytest.mark.gpu
def test_device_inflate_hand_built_streams():
    """the whole corpus in one launch, four times over: each turn another order, another src_off & 3 and dst_off & 15 for every
    member (the flush class starts at the alignment its boundaries were laid out for), another packed_bytes mod 4"""
    import biolib_amd

    t0 = time.perf_counter()
    entries = device_entries()
    # the flush streams put their symbols on ring positions that hold for ONE alignment of the destination: turn 0 gives them that one
    design = [int(e.name.split("align=")[1].split()[0]) if e.name.startswith("flush") and "align=" in e.name else None for e in entries]
    built = time.perf_counter() - t0
    ctx = biolib_amd.Context(0)
    t0 = time.perf_counter()
    for turn in range(4):
        kernel_s, n, packed_bytes, text_bytes = run_on_device(ctx, entries, turn, design)
        print(f"\nturn {turn}: {n} members, {packed_bytes / 1e6:.1f} MB packed, {text_bytes / 1e6:.1f} MB of text, both kernels {kernel_s * 1e3:.1f} ms")
    print(f"corpus built in {built:.1f} s; device part (layout, copies, 4 launches, checks) {time.perf_counter() - t0:.1f} s")
    ctx.close()


@pytest.mark.gpu
def test_device_crc_of_stored_members():
    import biolib_amd

    ctx = biolib_amd.Context(0)
    entries = crc_entries()
    for turn in range(4):
        run_on_device(ctx, entries, turn, long_members=False)
    ctx.close()
