"""The specification of the text index and the FASTA / FASTQ writer (bl_text_index_build, bl_batch_format; biolib_amd/csrc/bl_format_core.hpp)
as Python, and the named cases.  TEST INFRASTRUCTURE shared by test_format_model.py (CPU: the model against a plain restatement),
test_emu_format.py (the bodies under the sanitizers) and test_gpu_format.py (the kernels).  Nothing here runs code under test.

index_model    the 16-byte records and the offsets of a regular text, by position (what the index kernel writes)
format_model   the writer by position: the widths of a record's segments, then every byte from its place in the record — the arithmetic
               the kernel does, on the arrays the kernel gets
parse_plain / format_plain   the plain restatement: split the text into lines, join strings per record
cases()        name -> case: text (or None), bases, offsets, source_index, spans, tags, rule; each the smallest that reaches its branch"""
import numpy as np

U64 = 2**64 - 1
WAVE_BYTES = 4096
RECORD_DTYPE = np.dtype([("name_begin", "<u8"), ("name_len", "<u4"), ("qual_delta", "<u4")])


def rule(fmt="fastq", line_width=0, quality_fill=b"I", prefix=b"", first_number=0, label=b"", skip_empty=False, tag_length=False):
    return dict(fmt=fmt, line_width=line_width, quality_fill=quality_fill[0] if isinstance(quality_fill, bytes) else int(quality_fill), prefix=bytes(prefix),
                first_number=int(first_number), label=bytes(label), skip_empty=bool(skip_empty), tag_length=bool(tag_length))


# ----------------------------------------------------------------------------- the index

def _lines(text):
    """(start, end) of every line without its terminator ('\\n' or '\\r\\n'); the last line may lack one"""
    out, at = [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        end = len(text) if nl < 0 else nl
        stop = end - 1 if end > at and text[end - 1:end] == b"\r" else end
        out.append((at, stop))
        at = end + 1
    return out


def index_model(text):
    """records (RECORD_DTYPE), offsets (uint64, n + 1), is_fastq of a text the device parser accepts"""
    if not text:
        return np.zeros(0, RECORD_DTYPE), np.zeros(1, np.uint64), False
    fastq = text[:1] == b"@"
    if not fastq and text.endswith(b">") and (len(text) == 1 or text[-2:-1] == b"\n"):
        text = text[:-1]  # a lone marker at the very end opens no record
    lines = _lines(text)
    recs, offs, total = [], [], 0
    if fastq:
        lines = lines[:len(lines) - len(lines) % 4]
        for r in range(0, len(lines), 4):
            (hs, he), (ss, se), _, (qs, _) = lines[r:r + 4]
            recs.append((hs + 1, he - hs - 1, qs - (hs + 1)))
            offs.append(total)
            total += se - ss
    else:
        for s, e in lines:
            if text[s:s + 1] == b">":
                recs.append((s + 1, e - s - 1, 0))
                offs.append(total)
            else:
                total += e - s
    return np.array(recs, RECORD_DTYPE).reshape(-1), np.array(offs + [total], np.uint64), fastq


def parse_plain(text):
    """the restatement's view of a regular text: (names, sequences, qualities or None), names being whole header lines"""
    fastq = text[:1] == b"@"
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in text.split(b"\n")]
    if lines and lines[-1] == b"":
        lines.pop()
    if fastq:
        while len(lines) % 4:
            lines.pop()
        return [ln[1:] for ln in lines[0::4]], lines[1::4], lines[3::4]
    names, seqs = [], []
    for ln in lines:
        if ln[:1] == b">":
            names.append(ln[1:])
            seqs.append(b"")
        else:
            seqs[-1] += ln
    if text.endswith(b">") and (len(text) == 1 or text[-2:-1] == b"\n"):
        names.pop(), seqs.pop()
    return names, seqs, None


# ----------------------------------------------------------------------------- the writer, by position

def _digits(v):
    d, p = 1, 10
    for _ in range(19):
        d += v >= p
        p *= 10
    return d


def _digit(v, nd, idx):
    return 48 + v // 10 ** (nd - 1 - idx) % 10


def _extent(offsets, n_bases, i):
    first, end = min(int(offsets[i]), n_bases), min(int(offsets[i + 1]), n_bases)
    return first, max(end - first, 0)


def format_model(c):
    """(text bytes, records written) of case c"""
    r = c["rule"]
    bases, offsets = c["bases"], c["offsets"]
    n_seqs = len(offsets) - 1
    text = c["text"] or b""
    records, ioffs, ifastq = index_model(text)
    fastq = r["fmt"] == "fastq"
    W = 0 if fastq else r["line_width"]
    out, written = bytearray(), 0
    for i in range(n_seqs):
        first, L = _extent(offsets, len(bases), i)
        if L == 0 and r["skip_empty"]:
            continue
        written += 1
        s = int(c["source_index"][i]) if c["source_index"] is not None else i
        indexed = len(records) > 0 and s < len(records)
        number = (r["first_number"] + s) & U64
        q_src = qn = name_src = 0
        if indexed:
            name_src = min(int(records[s]["name_begin"]), len(text))
            name_w = min(int(records[s]["name_len"]), len(text) - name_src)
            if ifastq and fastq:
                Ls = max(int(ioffs[s + 1]) - int(ioffs[s]), 0)
                b = int(c["spans"][s][0]) if c["spans"] is not None else 0
                q = int(records[s]["name_begin"]) + int(records[s]["qual_delta"])
                qn = min(max(Ls - b, 0), L)
                qn = 0 if q + b >= len(text) else min(qn, len(text) - q - b)
                q_src = q + b
        else:
            name_w = len(r["prefix"]) + _digits(number)
        ln_w = 6 + _digits(L) if r["tag_length"] else 0
        tag = int(c["tags"][i]) if c["tags"] is not None else 0
        tag_w = 1 + len(r["label"]) + _digits(tag) if c["tags"] is not None else 0
        head = 2 + name_w + ln_w + tag_w
        body = L + ((L + W - 1) // W if W and L else 1)
        total = head + body + (L + 3 if fastq else 0)
        for at in range(total):
            a = at - 1
            if at == 0:
                byte = 64 if fastq else 62
            elif a < name_w:
                if indexed:
                    byte = text[name_src + a]
                else:
                    byte = r["prefix"][a] if a < len(r["prefix"]) else _digit(number, _digits(number), a - len(r["prefix"]))
            elif a - name_w < ln_w:
                a -= name_w
                byte = b" LN:i:"[a] if a < 6 else _digit(L, _digits(L), a - 6)
            elif a - name_w - ln_w < tag_w:
                a -= name_w + ln_w
                byte = 32 if a == 0 else (r["label"][a - 1] if a - 1 < len(r["label"]) else _digit(tag, _digits(tag), a - 1 - len(r["label"])))
            elif at < head:
                byte = 10
            elif at - head < body:
                a = k = at - head
                if W:
                    col = a % (W + 1)
                    k = None if col == W else a // (W + 1) * W + col
                byte = 10 if k is None or k >= L else int(bases[first + k])
            else:
                a = at - head - body
                byte = 43 if a == 0 else 10 if a == 1 or a - 2 >= L else (text[q_src + a - 2] if a - 2 < qn else r["quality_fill"])
            out.append(byte)
    return bytes(out), written


# ----------------------------------------------------------------------------- the writer, restated plainly

def format_plain(c):
    r = c["rule"]
    bases, offsets = bytes(c["bases"]), c["offsets"]
    names, seqs, quals = parse_plain(c["text"]) if c["text"] else ([], [], None)
    out, written = [], 0
    for i in range(len(offsets) - 1):
        lo, hi = min(int(offsets[i]), len(bases)), min(int(offsets[i + 1]), len(bases))
        seq = bases[lo:max(lo, hi)]
        if not seq and r["skip_empty"]:
            continue
        written += 1
        s = int(c["source_index"][i]) if c["source_index"] is not None else i
        name = names[s] if s < len(names) else r["prefix"] + str((r["first_number"] + s) % 2**64).encode()
        if r["tag_length"]:
            name += b" LN:i:%d" % len(seq)
        if c["tags"] is not None:
            name += b" " + r["label"] + str(int(c["tags"][i])).encode()
        if r["fmt"] == "fasta":
            W = r["line_width"]
            lines = [seq[j:j + W] for j in range(0, len(seq), W)] if W and seq else [seq]
            out.append(b">" + name + b"\n" + b"".join(ln + b"\n" for ln in lines))
        else:
            fill = bytes([r["quality_fill"]])
            qual = fill * len(seq)
            if quals is not None and s < len(quals):
                b = int(c["spans"][s][0]) if c["spans"] is not None else 0
                qual = (quals[s][b:b + len(seq)] + qual)[:len(seq)]
            out.append(b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out), written


# ----------------------------------------------------------------------------- builders and cases

def dna(n, seed=1):
    return np.random.default_rng(7000 + seed).choice(np.frombuffer(b"ACGTN", np.uint8), int(n)).tobytes()


def quality(n, seed=1):
    return np.random.default_rng(9000 + seed).integers(33, 127, int(n)).astype(np.uint8).tobytes()


def name(n, seed=1):
    if n == 0:
        return b""
    body = np.random.default_rng(11000 + seed).choice(np.frombuffer(b"abcdefgh0123456789/:_ ", np.uint8), int(n)).tobytes()
    return (b"r" + body[1:]).replace(b"  ", b" x")


def fastq_text(names, seqs, nl=b"\n", quals=None):
    quals = quals or [quality(len(s), i) for i, s in enumerate(seqs)]
    return b"".join(b"@" + nm + nl + s + nl + b"+" + nl + q + nl for nm, s, q in zip(names, seqs, quals))


def fasta_text(names, seqs, nl=b"\n", width=0):
    out = []
    for nm, s in zip(names, seqs):
        lines = [s[j:j + width] for j in range(0, len(s), width)] if width and s else [s]
        out.append(b">" + nm + nl + b"".join(ln + nl for ln in lines))
    return b"".join(out)


def case(text=None, bases=None, offsets=None, source_index=None, spans=None, tags=None, **rule_args):
    """a case from a text (the batch is the text's own unless bases / offsets say otherwise)"""
    if bases is None:
        _, seqs, _ = parse_plain(text) if text else ([], [], None)
        bases = b"".join(seqs)
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]) if seqs else np.zeros(1)
    u = lambda a, shape=(-1,): None if a is None else np.ascontiguousarray(np.array(a, dtype=np.uint64).reshape(shape))
    return dict(text=text, bases=np.frombuffer(bytes(bases), np.uint8), offsets=u(offsets), source_index=u(source_index), spans=u(spans, (-1, 2)), tags=u(tags),
                rule=rule(**rule_args))


LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 10000)
NAME_LENGTHS = (0, 1, 15, 16, 17)
LINE_WIDTHS = (1, 15, 16, 17, 60)


def selected(text, spans, keep_empty=True):
    """the batch bl_batch_select makes of the text's reads and these spans: (bases, offsets, source_index)"""
    _, seqs, _ = parse_plain(text)
    parts, src = [], []
    for i, (s, (b, e)) in enumerate(zip(seqs, spans)):
        b, e = min(b, len(s)), min(e, len(s))
        piece = s[b:e] if e > b else b""
        if piece or keep_empty:
            parts.append(piece)
            src.append(i)
    return b"".join(parts), np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64), np.array(src, np.uint64)


def _cases():
    C = {}
    C["zero_records"] = case(text=None, bases=b"", offsets=[0])
    C["zero_records_fasta"] = case(text=None, bases=b"", offsets=[0], fmt="fasta", line_width=60)
    C["one_base"] = case(fastq_text([b"a"], [b"A"]))
    C["minimal_fastq"] = case(b"@\n\n+\n\n")
    seqs20 = [dna(20, i) for i in range(len(NAME_LENGTHS))]
    C["name_lengths"] = case(fastq_text([name(n, n) for n in NAME_LENGTHS], seqs20))
    C["name_lengths_fasta"] = case(fasta_text([name(n, n) for n in NAME_LENGTHS], seqs20), fmt="fasta")
    long_seqs = [dna(L, L) for L in LENGTHS]
    C["lengths"] = case(fastq_text([name(3 + i % 5, i) for i in range(len(LENGTHS))], long_seqs))
    C["lengths_reversed"] = case(fastq_text([name(9, i) for i in range(len(LENGTHS))], long_seqs[::-1]))
    C["lengths_generated"] = case(None, b"".join(long_seqs), np.concatenate([[0], np.cumsum(LENGTHS)]), fmt="fasta", prefix=b"u", tag_length=True)
    C["lengths_generated_fastq"] = case(None, b"".join(long_seqs), np.concatenate([[0], np.cumsum(LENGTHS)]), prefix=b"read/", quality_fill=b"#")
    few = [dna(L, 50 + L) for L in (5, 0, 33, 16, 1)]
    nm5 = [name(4 + i, 70 + i) for i in range(5)]
    full = [dna(L, 60 + L) for L in (5, 2, 33, 16, 1)]  # (the parser refuses a CRLF text with an empty sequence: a lone '\r' is a base to the reference reader)
    C["crlf"] = case(fastq_text(nm5, full, nl=b"\r\n"))
    C["crlf_fasta"] = case(fasta_text(nm5, full, nl=b"\r\n", width=7), fmt="fasta", line_width=7)
    C["unterminated"] = case(fastq_text(nm5, few)[:-1])
    C["unterminated_fasta"] = case(fasta_text(nm5[:4], few[:4])[:-1], fmt="fasta")
    C["trailing_blank_lines"] = case(fastq_text(nm5, few) + b"\n\r\n\n")
    C["wrapped_fasta_source"] = case(fasta_text(nm5, [dna(L, L) for L in (61, 120, 1, 60, 179)], width=60), fmt="fasta", line_width=60)
    C["wrapped_fasta_unwrapped"] = case(fasta_text(nm5, [dna(L, L) for L in (61, 120, 1, 60, 179)], width=60), fmt="fasta")
    three = b"ACGTA" * 3
    for nm, first in (("9_to_10", 8), ("99_to_100", 98), ("2_pow_32", 2**32 - 2), ("2_pow_64_wraps", 2**64 - 2)):
        C["numbers_" + nm] = case(None, three, [0, 5, 10, 15], prefix=b"n", first_number=first, tags=[9, 10, U64], label=b"KC:i:")
    C["numbers_long_prefix"] = case(None, three, [0, 5, 10, 15], fmt="fasta", prefix=b"fifteen_bytes__", first_number=2**63, tags=[0, 99, 100], label=b"fifteen_bytes__")
    for W in LINE_WIDTHS:
        Ls = (W, 2 * W, 3 * W + 1, W - 1 if W > 1 else 0, 1, 4 * W, 0, 5 * W + W // 2, 300)
        C["line_width_%d" % W] = case(None, dna(sum(Ls), W), np.concatenate([[0], np.cumsum(Ls)]), fmt="fasta", line_width=W, prefix=b"s", tag_length=True)
    src_seqs = [dna(L, 200 + L) for L in (40, 40, 40, 40, 7, 100, 40)]
    src = fastq_text([name(6 + i, 300 + i) for i in range(7)], src_seqs)
    spans = [(0, 40), (13, 35), (40, 40), (41, 50), (3, 7), (17, 100), (0, 16)]  # begin 0, inside, = L, > L
    for keep in (True, False):
        b, o, si = selected(src, spans, keep)
        C["spans_keep_empty" if keep else "spans_compacted"] = case(src, b, o, si, spans)
        C["spans_keep_empty_skip" if keep else "spans_compacted_skip"] = case(src, b, o, si, spans, skip_empty=True)
    b, o, si = selected(src, spans, True)
    C["spans_null_source_index"] = case(src, b, o, None, spans)
    C["spans_overrun_gets_fill"] = case(src, src_seqs[0] * 2, [0, 30, 80], [0, 4], [(20, 40)] * 7, quality_fill=b"!")  # quality lines end before the sequences
    whole = b"".join(src_seqs)
    whole_offs = np.concatenate([[0], np.cumsum([len(s) for s in src_seqs])])
    pick = [6, 0, 3, 3, 5, 1, 2]
    C["source_index_permutes_and_repeats"] = case(src, whole, whole_offs, pick)
    C["source_index_past_the_index"] = case(src, whole, whole_offs, [0, 7, 6, U64, 8, 2**32, 1], prefix=b"lost", first_number=5, quality_fill=b"~")
    C["tags_on_index_names"] = case(src, whole, whole_offs, tags=[0, 9, 10, 99, 100, 2**32, U64], label=b"KC:i:", tag_length=True)
    C["fastq_to_fasta"] = case(src, fmt="fasta")
    C["fastq_to_fasta_wrapped"] = case(src, fmt="fasta", line_width=16)
    C["fasta_to_fastq"] = case(fasta_text(nm5, few, width=10), quality_fill=b"5")
    C["many_tiny"] = case(b"@\n\n+\n\n" * 700 + b"@x\nA\n+\n!\n" * 3)  # 682 records begin inside the first wave's bytes
    C["many_tiny_generated"] = case(None, b"", np.zeros(2001), fmt="fasta")
    # every alignment mod 4 of name start, sequence start, quality start and output offset
    al_names = [name(a, 400 + a + 4 * k) for k in range(8) for a in range(4)]
    al_seqs = [dna(33 + (a + k) % 4 + 16 * (k % 3), 500 + a + 4 * k) for k in range(8) for a in range(4)]
    al = fastq_text(al_names, al_seqs)
    C["alignments"] = case(al)
    b, o, si = selected(al, [(i % 5, 30 + i) for i in range(32)], False)
    C["alignments_trimmed"] = case(al, b, o, si, [(i % 5, 30 + i) for i in range(32)])
    return C


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def wave_paths(rec_off):
    """(register waves, memory waves) of the write: a wave looks its records up in memory where 64 or more records begin behind its first
    one at or in front of its last byte"""
    total, reg, mem = int(rec_off[-1]), 0, 0
    for first in range(0, total, WAVE_BYTES):
        last = min(first + WAVE_BYTES, total) - 1
        lo = int(np.searchsorted(rec_off[:-1], first, side="right")) - 1
        inside = int(np.searchsorted(rec_off[lo + 1:lo + 65], last, side="right"))
        if inside < 64:
            reg += 1
        else:
            mem += 1
    return reg, mem


def record_offsets(c):
    """the first output byte of every sequence's record (dropped ones have length 0), the total last"""
    lens = []
    for i in range(len(c["offsets"]) - 1):
        one = dict(c, offsets=c["offsets"][i:i + 2], source_index=None if c["source_index"] is None else c["source_index"][i:i + 1],
                   tags=None if c["tags"] is None else c["tags"][i:i + 1])
        if c["source_index"] is None:  # (the source read is the sequence's own number)
            one["source_index"] = np.array([i], np.uint64)
        lens.append(len(format_model(one)[0]))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
