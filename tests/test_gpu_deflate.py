"""GPU: BGZF written on the device (bl_bgzf_bound, bl_bgzf_deflate, bl_text_write_bgzf; biolib_amd/csrc/bl_deflate.hip) against the Python
specification (deflate_cases.py) byte for byte — guard bytes behind the output, the member table, every alignment of the text, reruns,
the capacity refusal and every other refusal, member counts up to one past the group — the round trips through gzip, bl_bgzf_inflate and
bl_bgzf_walk, and the chain's exit end to end: simulated FASTQ in, trimmed, written compressed, read back."""
import ctypes as C
import gzip

import numpy as np
import pytest

import deflate_cases as DC

pytestmark = pytest.mark.gpu
GUARD = 64
CASES = DC.cases()


@pytest.fixture(scope="module")
def ctx():
    import biolib_amd

    c = biolib_amd.Context(0)
    yield c
    c.close()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def on_device(text, offset=0):
    """the text inside a device allocation, its first byte `offset` bytes behind the allocation's first"""
    import torch

    t = torch.zeros(len(text) + offset + 1, dtype=torch.uint8, device="cuda")
    if text:
        t[offset:offset + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    return t


def deflate(ctx, text, eof=True, offset=0, capacity=None, members=True):
    """(the bytes written, the whole output buffer with its guard, the member rows, rc) of one raw call"""
    import torch

    from biolib_amd import capi

    flags = 0 if eof else capi.BGZF_NO_EOF
    bound = int(ctx._lib.bl_bgzf_bound(len(text), flags))
    assert bound == DC.bound(len(text), eof)
    src = on_device(text, offset)
    out = torch.full((bound + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    n_rows = max((len(text) + DC.MEMBER - 1) // DC.MEMBER, 1)
    table = torch.full((n_rows + 1, 4), -1, dtype=torch.int64, device="cuda") if members else None
    nb, nm = C.c_uint64(7), C.c_uint64(7)
    torch.cuda.synchronize()
    rc = ctx._lib.bl_bgzf_deflate(ctx._h, C.c_void_p(src.data_ptr() + offset) if text else None, len(text), flags, ptr(out), bound if capacity is None else capacity,
                                  C.byref(nb), ptr(table), C.byref(nm))
    return int(nb.value), out, table, int(nm.value), rc


def rows_of(table, n):
    a = table[:n].cpu().numpy().view(np.uint64)
    return [(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF, int(r[2]) >> 32, int(r[3]) & 0xFFFFFFFF) for r in a], a


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(ctx, name):
    text, eof = CASES[name]
    want, _, want_table = DC.bgzf_model(text, eof)
    n_out, out, table, n_members, rc = deflate(ctx, text, eof)
    assert rc == 0 and n_out == len(want) and n_members == len(want_table)
    host = out.cpu().numpy()
    assert host[:n_out].tobytes() == want, (name, next((i for i in range(n_out) if host[i] != want[i]), None))
    assert (host[n_out:] == 0xA5).all(), "nothing at or behind d_out[n_out_bytes], the guard behind the bound included"
    rows, raw = rows_of(table, n_members)
    assert rows == want_table and not (raw[:, 3] >> 32).any(), "the member table; reserved is 0"
    assert (table[n_members:].cpu().numpy() == -1).all(), "no row behind the last member"
    # rerun: bit-equal
    again = deflate(ctx, text, eof)
    assert again[0] == n_out and bool((again[1] == out).all()) and bool((again[2] == table).all())
    assert (gzip.decompress(want) if want else b"") == text


@pytest.mark.parametrize("name", ["bytes_1", "bytes_4", "twenty_bytes", "no_match", "far_32768", "member_plus_1", "ends_at_bit_3"])
def test_every_alignment_of_the_text(ctx, name):
    text, eof = CASES[name]
    want = DC.bgzf_model(text, eof)[0]
    for offset in range(16):
        n_out, out, _, _, rc = deflate(ctx, text, eof, offset=offset, members=False)
        assert rc == 0 and out[:n_out].cpu().numpy().tobytes() == want, (name, offset)


def test_capacity_refusal_leaves_the_output_untouched(ctx):
    from biolib_amd import capi

    for name in ("bytes_1", "member_plus_1", "empty"):
        text, eof = CASES[name]
        bound = DC.bound(len(text), eof)
        for capacity in (bound - 1, 0):
            n_out, out, table, _, rc = deflate(ctx, text, eof, capacity=capacity)
            assert rc == capi.BL_ERR_CAPACITY and n_out == bound, "the bound is reported"
            assert bool((out == 0xA5).all()) and bool((table == -1).all()), "nothing was launched"
        assert deflate(ctx, text, eof, capacity=bound)[4] == 0


def test_refusals(ctx):
    import torch

    from biolib_amd import capi

    lib, INV = ctx._lib, capi.BL_ERR_INVALID
    text = on_device(b"ACGT" * 10)
    out = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    nb = C.c_uint64()
    torch.cuda.synchronize()
    good = (ctx._h, ptr(text), 40, 0, ptr(out), 256, C.byref(nb), None, None)

    def call(**change):
        names = ("ctx", "d_text", "n_bytes", "flags", "d_out", "capacity", "n_out_bytes", "d_members", "n_members")
        return lib.bl_bgzf_deflate(*[change.get(k, v) for k, v in zip(names, good)])

    assert call(ctx=None) == INV
    assert call(d_text=None) == INV
    assert call(d_out=None) == INV
    assert call(n_out_bytes=None) == INV
    assert call(flags=2) == INV and call(flags=1 << 31) == INV
    assert call(d_out=C.c_void_p(out.data_ptr() + 8)) == INV and call(d_out=C.c_void_p(out.data_ptr() + 1)) == INV
    assert b"16-byte" in lib.bl_last_error()
    assert bool((out == 0xA5).all()), "nothing was launched"
    assert call() == 0 and nb.value == len(DC.bgzf_model(b"ACGT" * 10)[0])
    assert call(d_text=None, n_bytes=0) == 0 and nb.value == 28, "no text: the EOF marker alone"
    assert lib.bl_text_write_bgzf(None, ptr(text), 40, b"/dev/null", 0, 0) == INV
    assert lib.bl_text_write_bgzf(ctx._h, None, 40, b"/dev/null", 0, 0) == INV
    assert lib.bl_text_write_bgzf(ctx._h, ptr(text), 40, None, 0, 0) == INV
    assert lib.bl_text_write_bgzf(ctx._h, ptr(text), 40, b"/dev/null", 0, 2) == INV
    assert lib.bl_text_write_bgzf(ctx._h, ptr(text), 40, b"/no_such_directory/x.gz", 0, 0) == capi.BL_ERR_IO


@pytest.mark.parametrize("n_members", [1, 2, 5, DC.GROUP_MEMBERS + 1])
def test_member_counts_and_round_trips(ctx, n_members):
    """whole members of one text and a short last one; the output through gzip, through bl_bgzf_inflate with the returned table, and
    through bl_bgzf_walk"""
    import torch

    block = DC.simulated_fastq(210, seed=6)[:DC.MEMBER]
    text = block * (n_members - 1) + DC.dna_lines(777, 5)
    want, _, want_table = DC.bgzf_model(text)
    packed, table = ctx.bgzf_deflate(text, members=True)
    data = packed.cpu().numpy().tobytes()
    assert data == want and table.shape == (n_members, 4)
    assert gzip.decompress(data) == text
    rows, raw = rows_of(table, n_members)
    assert rows == want_table
    # the device round trip needs no walk
    back = torch.full((len(text) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((n_members,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert ctx._lib.bl_bgzf_inflate(ctx._h, ptr(packed), packed.numel(), ptr(table), n_members, ptr(back), len(text), ptr(status)) == 0
    ctx.sync()
    assert not status.any() and back[:len(text)].cpu().numpy().tobytes() == text and bool((back[len(text):] == 0xA5).all())
    # and the walk over the bytes gives that same table
    walked = np.zeros((n_members + 2, 4), np.uint64)
    n, used, n_text = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert ctx._lib.bl_bgzf_walk(data, len(data), 0, 0, walked.ctypes.data, n_members + 2, C.byref(n), C.byref(used), C.byref(n_text)) == 0
    assert (n.value, used.value, n_text.value) == (n_members + 1, len(data), len(text)), "the EOF marker is a member to the walk"
    assert np.array_equal(walked[:n_members], raw)


def test_write_of_three_chunks(ctx, tmp_path):
    """bl_text_write_bgzf takes the text in chunks of DC.GROUP_MEMBERS members: two whole chunks and a short third one through its
    pipeline (compression, the size in a pinned word, the copy, the write), then appended to"""
    block = DC.simulated_fastq(210, seed=6)[:DC.MEMBER]
    text = block * (2 * DC.GROUP_MEMBERS + 3) + DC.dna_lines(777, 5)
    want = DC.bgzf_model(text)[0]
    d_text = on_device(text)[:len(text)]
    path = tmp_path / "three_chunks.gz"
    assert ctx._write_text(d_text, path, False, True, False) == len(want) - 28
    assert path.read_bytes() == want[:-28]
    assert ctx._write_text(d_text[:777], path, True, True, True) == len(DC.bgzf_model(text[:777])[0])
    data = path.read_bytes()
    assert data == want[:-28] + DC.bgzf_model(text[:777])[0] and gzip.decompress(data) == text + text[:777]


def test_python_entry_points(ctx):
    text = CASES["simulated_fastq"][0]
    want = DC.bgzf_model(text)[0]
    assert ctx.bgzf_deflate(text).cpu().numpy().tobytes() == want
    assert ctx.bgzf_deflate(on_device(text)[:len(text)], eof=False).cpu().numpy().tobytes() == want[:-28]
    assert ctx.bgzf_deflate(b"").cpu().numpy().tobytes() == DC.EOF_MARKER and ctx.bgzf_deflate(b"", eof=False).numel() == 0
    text, status = ctx.bgzf_inflate(want)
    assert text.tobytes() == CASES["simulated_fastq"][0] and not status.any()


def test_end_to_end_trim_write_compressed_read_back(ctx, tmp_path):
    """the chain's exit: simulated FASTQ in, trimmed, write(compress=True); gzip gives format()'s text; the Reader gives the same reads;
    the append loop with eof=False gives one valid file"""
    import torch

    import biolib_amd

    k = 21
    text = DC.simulated_fastq(3000, seed=9)  # about 1 MB: 15 members
    b, ix = ctx.from_text_indexed(text)
    scan = b.kmers(k, canonical=True)
    counted = ctx.count_table(torch.from_numpy(np.ascontiguousarray(scan["values"][scan["valid"] != 0]).view(np.int64)).cuda(), key_bits=2 * k)
    rc, _ = b.read_counts(counted, k, 2, canonical=True)
    spans = b.read_spans(rc, k, "prefix")
    kept, source_index = b.select(spans)
    how = dict(index=ix, source_index=source_index, spans=spans)
    want = kept.format(**how).cpu().numpy().tobytes()
    assert 0 < kept.n_seqs and len(want) > 10 * DC.MEMBER
    path = tmp_path / "out.fq.gz"
    n_written = kept.write(path, compress=True, **how)
    data = path.read_bytes()
    assert n_written == len(data) and data == DC.bgzf_model(want)[0]
    with gzip.open(path) as f:
        assert f.read() == want
    assert kept.write(tmp_path / "plain.fq", **how) == len(want) and (tmp_path / "plain.fq").read_bytes() == want, "compress=False: as before"
    # the file read back through the device reader: the same reads
    r = biolib_amd.Reader(path)
    assert r.kind == "bgzf"
    bases, n_seqs = [], 0
    loop = tmp_path / "loop.fq.gz"
    for i, (batch, index) in enumerate(r.device_batches(ctx, len(want) // 4, indexed=True)):
        bases.append(bytes(batch.download()))
        n_seqs += batch.n_seqs
        batch.write(loop, append=i > 0, compress=True, eof=False, index=index)
        index.close()
        batch.close()
    r.close()
    assert i >= 2 and n_seqs == kept.n_seqs and b"".join(bases) == bytes(kept.download())
    # the loop's file lacks its EOF marker; a last call with an empty text writes it
    assert loop.read_bytes()[-28:] != DC.EOF_MARKER
    empty = ctx.upload(b"")
    assert empty.write(loop, append=True, compress=True) == 28
    empty.close()
    data = loop.read_bytes()
    assert gzip.decompress(data) == want and data[-28:] == DC.EOF_MARKER and data.count(DC.EOF_MARKER) == 1
    DC.check_members(data, want, True, full_members=False)
    for x in (kept, counted, ix, b):
        x.close()


def test_unitigs_write_compressed(ctx, tmp_path):
    import links_cases as LK
    from test_gpu_links import build

    k, table, m = LK.dense_model("dense_300_of_512")
    t = build(ctx, table, 1, 2 * k)
    u = t.unitigs(k, links=True)
    text = u.format_gfa("utg", 5).cpu().numpy().tobytes()
    n = u.write_gfa(tmp_path / "g.gfa.gz", prefix="utg", first_number=5, compress=True)
    data = (tmp_path / "g.gfa.gz").read_bytes()
    assert n == len(data) and data == DC.bgzf_model(text)[0] and gzip.decompress(data) == text
    assert u.write_gfa(tmp_path / "g.gfa", prefix="utg", first_number=5) == len(text) and (tmp_path / "g.gfa").read_bytes() == text
    n = u.write_fasta(tmp_path / "u.fa.gz", line_width=60, compress=True)
    u.write_fasta(tmp_path / "u.fa", line_width=60)
    data = (tmp_path / "u.fa.gz").read_bytes()
    assert n == len(data) and gzip.decompress(data) == (tmp_path / "u.fa").read_bytes() and data[-28:] == DC.EOF_MARKER
    t.close()
