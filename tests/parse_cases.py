"""Hand-built FASTA / FASTQ texts for every rule and edge of the device-side parser (biolib_amd/csrc/bl_parse.hip), a plain model of the
reference reader and the parser's stated domain.  TEST INFRASTRUCTURE shared by test_parse_cases.py (CPU: model, host reader, recorded
reference verdicts, the host emulation tests/emu/emu_parse.cpp) and test_gpu_parse_cases.py (the kernels).  Nothing here runs code under test.

kseq_model    a byte-by-byte reader with the reference reader's semantics, written from the rules at the head of bl_ingest.cpp
is_regular    the layouts the device parser promises to ACCEPT (head of bl_parse.hip); whatever it accepts besides must still match
CASES         name -> text, built by code, no text over 40 KB.  The kernel constants the geometry cases aim at: 16 bytes per thread,
              1,024 per wave, 4,096 per block of the newline kernels; 256 lines / records / 16-byte output groups per block elsewhere
ORDER         the names with large and small texts alternating (the parser's scratch only grows: no result may depend on the text before)
FIXED_UNIFORM / FIXED_RAGGED   reads of one length, and the same total and count with one pair of reads made L - 1 and L + 1
BGZF_NAMES    the cases that also go through the compressed path"""
import hashlib

import numpy as np

MAX_TEXT = 40 * 1024
_BLANK = b" \t\n\v\f\r"


# ----------------------------------------------------------------------------- the reference reader, modelled

def kseq_model(text):
    """the sequences the reference reader returns for `text`, or None where it reports an error"""
    n, i, out, pending = len(text), 0, [], False
    while True:
        if not pending:  # a record starts at the next '>' or '@', wherever it stands
            while i < n and text[i] not in b">@":
                i += 1
            if i >= n:
                return out
            i += 1
        pending = False
        if i >= n:  # the marker was the last byte: end of input, no record
            return out
        while i < n and text[i] not in _BLANK:  # the name ends at the first whitespace byte
            i += 1
        if i < n:
            stop = text[i]
            i += 1
            if stop != 10:  # the rest of the header line is the comment
                while i < n and text[i] != 10:
                    i += 1
                i += 1
        seq, plus = bytearray(), False
        while True:  # sequence lines are joined until a line opens with '>', '@' or '+'
            if i >= n:
                out.append(bytes(seq))
                return out
            c = text[i]
            i += 1
            if c in b">@":
                pending = True
                break
            if c == 43:
                plus = True
                break
            if c == 10:
                continue
            seq.append(c)
            while i < n and text[i] != 10:
                seq.append(text[i])
                i += 1
            i += 1
            if len(seq) > 1 and seq[-1] == 13:  # a trailing '\r' goes only if more than that one byte has been gathered
                seq.pop()
        if not plus:
            out.append(bytes(seq))
            continue
        while True:  # the rest of the separator line carries nothing
            if i >= n:
                return None  # no quality at all
            c = text[i]
            i += 1
            if c == 10:
                break
        qual = bytearray()
        while i < n:  # quality lines are gathered until they are as long as the sequence
            while i < n and text[i] != 10:
                qual.append(text[i])
                i += 1
            i += 1
            if len(qual) > 1 and qual[-1] == 13:
                qual.pop()
            if len(qual) >= len(seq):
                break
        if len(qual) != len(seq):
            return None
        out.append(bytes(seq))


def verdict(seqs):
    """a reader's result as tests/golden/ref_verdicts.json keeps it under "parser_cases": None for an error; the lengths and a digest of the
    bases (test_ingest.reads_verdict), and past 64 records the count and a digest of the lengths in place of the list"""
    if seqs is None:
        return None
    return compact({"lens": [len(x) for x in seqs], "sha": hashlib.sha256(b"".join(seqs)).hexdigest()[:32]})


def compact(v):
    if v is None or len(v["lens"]) <= 64:
        return v
    return {"n": len(v["lens"]), "lens_sha": hashlib.sha256(",".join(map(str, v["lens"])).encode()).hexdigest()[:32], "sha": v["sha"]}


def text_sha(text):
    return hashlib.sha256(text).hexdigest()[:16]


# ----------------------------------------------------------------------------- the parser's stated domain

def _strip_cr(line):
    return line[:-1] if line.endswith(b"\r") else line


def is_regular(text):
    """True for the layouts the device parser must accept: first byte '@' or '>'; FASTQ of exactly four lines per record ('@' header,
    '+' separator, a quality line as long as its sequence) with at most three blank lines behind the last record, FASTA with any
    wrapping; LF or CRLF; no sequence line that opens with '>', '@' or '+'; no line that is a lone '\\r'"""
    if not text or text[:1] not in (b"@", b">"):
        return False
    lines = text.split(b"\n")
    terminated = lines[-1] == b""
    if terminated:
        lines.pop()
    if text[:1] == b">":
        for ln in lines:
            if ln == b"\r" or (ln[:1] in (b"@", b"+")):
                return False
        return True
    excess = len(lines) % 4  # the blank lines behind the last record, "\n" or "\r\n" (an empty record's own lines are no excess)
    if excess and not (terminated and all(ln in (b"", b"\r") for ln in lines[-excess:])):
        return False
    lines = lines[:len(lines) - excess]
    if not lines or any(ln == b"\r" for ln in lines):
        return False
    for r in range(0, len(lines), 4):
        head, seq, sep, qual = (_strip_cr(x) for x in lines[r:r + 4])
        if head[:1] != b"@" or sep[:1] != b"+" or seq[:1] in (b">", b"@", b"+") or len(seq) != len(qual):
            return False
    return True


# ----------------------------------------------------------------------------- builders

def dna(n, seed=1):
    """n bases, upper case, no line structure"""
    return np.random.default_rng(1000 + seed).choice(np.frombuffer(b"ACGT", np.uint8), int(n)).tobytes()


def fasta(records, nl=b"\n", width=0):
    """records: sequences (bytes) or lists of lines"""
    out = []
    for i, r in enumerate(records):
        lines = r if isinstance(r, list) else ([r[j:j + width] for j in range(0, len(r), width)] if width and r else ([r] if r else []))
        out.append(b">s%d" % i + nl + b"".join(ln + nl for ln in lines))
    return b"".join(out)


def fastq(seqs, nl=b"\n", sep=b"+", qual=None):
    return b"".join(b"@r%d" % i + nl + s + nl + sep + nl + (qual(i, s) if qual else b"I" * len(s)) + nl for i, s in enumerate(seqs))


CASES = {}
FIXED_UNIFORM, FIXED_RAGGED, BGZF_NAMES = [], [], []


def _add(name, text, bgzf=False):
    assert name not in CASES and len(text) <= MAX_TEXT, (name, len(text))
    CASES[name] = bytes(text)
    if bgzf:
        BGZF_NAMES.append(name)


def _newline_geometry():
    places = (15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)
    for p in places:
        # a sequence line whose '\n' sits at byte p; with CRLF its '\r' at p - 1: the last byte of a chunk, wave or block where p is a multiple
        for tag, nl in (("lf", b"\n"), ("crlf", b"\r\n")):
            head = b">h" + nl
            L = p - (len(nl) - 1) - len(head)
            t = head + dna(L, p) + nl + b"ACGT" + nl + b">t" + nl + b"GG" + nl
            assert t[p] == 10 and (nl == b"\n" or t[p - 1] == 13)
            _add("nl_fa_%s_%d" % (tag, p), t)
            head = b"@h" + nl
            L = p - (len(nl) - 1) - len(head)
            s = dna(L, p + 1)
            t = head + s + nl + b"+" + nl + b"J" * L + nl + b"@t" + nl + b"GG" + nl + b"+" + nl + b"JJ" + nl
            assert t[p] == 10
            _add("nl_fq_%s_%d" % (tag, p), t)
    # text length n: n mod 16 of 0, 1, 15 (the last chunk goes byte by byte unless n mod 16 == 0), and one block -1, +0, +1
    for n in (32, 33, 47, 4095, 4096, 4097):
        body = n - 4  # ">h\n" ... "\n"
        s = dna(body - body // 61, n)
        t = b">h\n" + b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) + b"\n"
        t = t[:n - 1].rstrip(b"\n") + b"A" * (n - 1 - len(t[:n - 1].rstrip(b"\n"))) + b"\n"
        assert len(t) == n
        _add("len_fa_%d" % n, t)
        for open_end in (False, True):  # the same lengths with the last line left open
            sep = b"+" if (n - 7 - (0 if open_end else 1) + 1) % 2 == 0 else b"+x"
            L = (n - len(b"@h\n\n\n") - len(sep) - (0 if open_end else 1)) // 2
            t = b"@h\n" + dna(L, n) + b"\n" + sep + b"\n" + b"K" * L + (b"" if open_end else b"\n")
            if len(t) == n:
                _add("len_fq_%d%s" % (n, "_open" if open_end else ""), t)
    # under 16 bytes: the byte-wise tail only
    for name, t in (("tiny_gt", b">"), ("tiny_gt_nl", b">\n"), ("tiny_fa_open", b">a\nA"), ("tiny_at", b"@"), ("tiny_fq_empty", b"@\n\n+\n\n"),
                    ("tiny_fq", b"@a\nAC\n+\nII\n"), ("tiny_fa", b">a\nAC\n")):
        _add(name, t)
    # a chunk of 16 newlines (bytes 16..31), and a whole block of them (blank lines inside a FASTA record)
    _add("chunk_of_newlines", b">h\nACGTACGTACGT\n" + b"\n" * 16 + b"GG\n>t\nTT\n")
    pre = b">h\n" + b"\n".join(dna(4092 - 4092 // 64, 7)[j:j + 63] for j in range(0, 4028, 63))
    pre = pre[:4095] + b"\n"
    assert len(pre) == 4096
    _add("block_of_newlines", pre + b"\n" * 4096 + b"ACGT\n>x\nTT\n", bgzf=True)
    # a line longer than 8,192 bytes: two blocks without a newline
    _add("long_line_fa", b">h\n" + dna(5000, 3) + b"\n" + dna(9000, 4) + b"\n" + dna(17, 5) + b"\n>t\nAC\n", bgzf=True)
    s = dna(9001, 6)
    _add("long_line_fq", b"@h\n" + s + b"\n+\n" + b"5" * len(s) + b"\n@t\nAC\n+\nII\n", bgzf=True)
    # every byte value but '\n' in mid-line: 0x0b, 0x1a, 0x2a, 0x8a are the SWAR test's near misses; '\r', '>', '@', '+' not in first place
    every = b"A" + bytes(b for b in range(1, 256) if b != 10) + b"C"
    _add("every_byte_fa", b">h\n" + every + b"\n" + every[::-1] + b"\n>t\nAC\n")
    _add("every_byte_fq", b"@h\n" + every + b"\n+\n" + every[::-1] + b"\n@t\n" + every[::-1] + b"\n+\n" + every + b"\n")


def _gather_geometry():
    one = dna(40, 11)
    _add("one_base_lines", b">h\n" + b"".join(one[i:i + 1] + b"\n" for i in range(40)) + b">t\nAC\n")
    _add("one_base_lines_crlf", b">h\r\n" + b"".join(one[i:i + 1] + b"\r\n" for i in range(40)))
    lens = (15, 16, 17, 31, 32, 33)
    recs = []
    for i, L in enumerate(lens):
        s = dna(L + 16, 20 + i)
        recs += [[s[:L], b"", s[L:]], []]  # a blank line inside, a header-only record behind
    _add("line_lengths", fasta(recs))
    _add("line_lengths_crlf", fasta(recs, nl=b"\r\n"))
    _add("line_lengths_fq", fastq([dna(L, 30 + L) for L in lens]))
    for total in (32, 33, 47, 5, 15, 16, 17):
        s = dna(total, 40 + total)
        _add("total_%d" % total, fasta([[s[:3], s[3:4], b"", s[4:20]], [s[20:]]]))
    _add("total_0", b">a\n>b\n\n>c\n")
    _add("total_0_fq", b"@a\n\n+\n\n@b\n\n+\n\n")
    _add("empty_first", fasta([b"", dna(20, 1), dna(5, 2)]))
    _add("empty_middle", fasta([dna(20, 1), b"", dna(5, 2)]))
    _add("empty_last", fasta([dna(20, 1), dna(5, 2), b""]))
    _add("empty_first_fq", fastq([b"", dna(20, 1), dna(5, 2)]))
    _add("empty_middle_fq", fastq([dna(20, 1), b"", dna(5, 2)]))
    _add("empty_last_fq", fastq([dna(20, 1), dna(5, 2), b""]))


def _counts():
    for n in (1, 2, 255, 256, 257):  # the launch arithmetic of the per-record kernels
        seqs = [dna((7 * i) % 23, i) for i in range(n)]
        _add("records_fa_%d" % n, fasta(seqs))
        _add("records_fq_%d" % n, fastq(seqs), bgzf=n == 257)
    for n in (255, 256, 257, 1023, 1024, 1025):  # ... and of the per-line kernels: one record of n lines
        s = dna(5 * n, n)
        _add("lines_%d" % n, b">h\n" + b"".join(s[5 * i:5 * i + 1 + i % 5] + b"\n" for i in range(n - 1)))


def fixed_reads():
    """(seq, offsets): the reads kernel_cases.reads(MODE_MINIMIZER, 100, 21, 5, 1) uses"""
    import kernel_cases as K
    import tie_plant as P

    seq, offs, L, g = K.reads(P.MODE_MINIMIZER, 100, 21, 5, 1)
    assert L == 100 and g is not None
    return seq.tobytes(), [int(x) for x in offs]


def _fixed_length():
    L = 100
    seq, offs = fixed_reads()
    n = len(offs) - 1

    def cut(flat, count, short):  # reads of L bases; read `short` gets L - 1 and the next one L + 1
        at, out = 0, []
        for i in range(count):
            k = L - 1 if i == short else L + 1 if i == short + 1 else L
            out.append(flat[at:at + k])
            at += k
        assert at == len(flat)
        return out

    _add("fixed_uniform", fastq(cut(seq, n, -5)), bgzf=True)
    FIXED_UNIFORM.append("fixed_uniform")
    for tag, short in (("first", 0), ("last", n - 2)):
        _add("fixed_ragged_" + tag, fastq(cut(seq, n, short)))
        FIXED_RAGGED.append("fixed_ragged_" + tag)
    # the offsets' second block (records 256 ...) takes more reads than those: 300 of the same length, as two-line FASTA
    many = dna(300 * L, 77)
    _add("fixed_uniform_300", fasta(cut(many, 300, -5)))
    FIXED_UNIFORM.append("fixed_uniform_300")
    _add("fixed_ragged_255_256", fasta(cut(many, 300, 255)))
    FIXED_RAGGED.append("fixed_ragged_255_256")
    _add("fixed_one_record", fastq([seq[:L]]))
    _add("fixed_all_empty", fastq([b""] * 40))
    _add("fixed_all_empty_fa", fasta([b""] * 300))


def _text_ends():
    two = fastq([dna(21, 1), dna(9, 2)])
    two_crlf = fastq([dna(21, 1), dna(9, 2)], nl=b"\r\n")
    for k in (1, 2, 3, 4, 5):
        _add("end_lf_%d" % k, two + b"\n" * k, bgzf=k in (1, 3))
        _add("end_crlf_%d" % k, two_crlf + b"\r\n" * k, bgzf=k == 3)
    _add("end_mixed_2", two + b"\r\n\n")
    _add("end_mixed_3", two_crlf + b"\n\r\n\n", bgzf=True)
    _add("end_mixed_3b", two + b"\r\n\r\n\n")
    for target in (60, 64, 65):  # the host looks at the last 64 bytes only
        for tag, tail in (("lf1", b"\n"), ("lf2", b"\n\n"), ("lf3", b"\n\n\n"), ("crlf1", b"\r\n"), ("crlf3", b"\r\n\r\n\r\n"), ("mixed3", b"\n\r\n\n"),
                          ("lf4", b"\n" * 4)):
            room = target - len(tail) - len(b"@r\n\n\n\n")
            sep = b"+" if (room - 1) % 2 == 0 else b"+x"
            L = (room - len(sep)) // 2
            t = b"@r\n" + dna(L, target) + b"\n" + sep + b"\n" + b"I" * L + b"\n" + tail
            assert len(t) == target
            _add("end_%d_%s" % (target, tag), t)
    _add("end_64_newlines_fa", fasta([dna(30, 1), dna(7, 2)]) + b"\n" * 64)
    _add("end_64_newlines_fq", two + b"\n" * 64)
    _add("end_63_newlines_fq", two + b"\n" * 63)
    # an unterminated last line, also with '\r' as the last byte
    for tag, cr in (("", b""), ("_cr", b"\r")):
        _add("open_qual" + tag, two[:-1] + cr, bgzf=not cr)
        _add("open_fa_seq" + tag, fasta([dna(30, 1), dna(7, 2)], width=20)[:-1] + cr, bgzf=bool(cr))
        _add("open_fa_header" + tag, fasta([dna(30, 1)]) + b">last one" + cr, bgzf=not cr)
    _add("open_qual_crlf", two_crlf[:-2])
    _add("trailing_gt", fasta([dna(30, 1)]) + b">")
    _add("trailing_gt_crlf", fasta([dna(30, 1)], nl=b"\r\n") + b">")
    _add("trailing_gt_nl", fasta([dna(30, 1)]) + b">\n")
    _add("trailing_gt_cr", fasta([dna(30, 1)]) + b">\r")
    _add("trailing_gt_open", fasta([dna(30, 1)])[:-1] + b">")  # no line of its own: a base


def _rules():
    seqs = [dna(n, n) for n in (5, 1, 12, 30, 2)]
    first = (b"@", b"+", b">", b"I", b"@")
    _add("qual_opens_with_marker", fastq(seqs, qual=lambda i, s: (first[i] + b"@" * len(s))[:len(s)]))
    _add("qual_opens_with_marker_crlf", fastq(seqs, nl=b"\r\n", qual=lambda i, s: (first[i] + b"+" * len(s))[:len(s)]))
    _add("plus_name", fastq(seqs, sep=b"+r name"))
    _add("markers_in_headers", b">a>b @c +d\nACGT\n>@x\nGG\n>+\nTT\n")
    _add("markers_in_headers_fq", b"@a@b >c +d\nACGT\n+\nIIII\n@>x\nGG\n+\nII\n")
    _add("lower_case_and_n", fasta([b"acgtnNACGTnnnnacgt", b"NNNNNNNNNNNNNNNNNNNNNNNN", b"n"]))
    _add("lower_case_and_n_fq", fastq([b"acgtnNACGTnnnnacgt", b"NNNNNNNNNNNNNNNNNNNNNNNN", b"n"]))
    _add("blanks_in_lines", b">h x\nAC GT\n A\nC \n\tG\n>t\n  \n")
    _add("blanks_in_lines_fq", b"@h x\nAC GT\tA\n+\nIIIIIII\n@t\n  \n+\n  \n")
    _add("double_cr", b">h\nAC\r\r\nGT\r\n")
    _add("double_cr_fq", b"@h\nAC\r\r\n+\nIII\r\n")
    # the reference reader drops a trailing '\r' only from more than one gathered byte
    _add("lone_cr_first_crlf", b">h\r\n\r\nACGT\r\n")
    _add("lone_cr_only", b">h\n\r")
    _add("lone_cr_only_nl", b">h\n\r\n")
    _add("lone_cr_first_second_record", b">a\r\nAC\r\n>h\r\n\r\nACGT\r\n")
    _add("lone_cr_after_blank", b">h\n\n\r\nAC\n")
    _add("lone_cr_after_bases", b">h\r\nAC\r\n\r\nGT\r\n")
    _add("lone_cr_after_one_base", b">h\nA\n\r\nC\n")
    _add("lone_cr_last_after_bases", b">a\nAC\n\r\n>b\nGT\n\r\n")
    _add("lone_cr_fq", b"@a\r\n\r\n+\r\n\r\n@b\r\nAC\r\n+\r\nII\r\n")
    _add("lone_cr_fq_seq", b"@a\nA\n+\nI\n@b\n\r\n+\nI\n")
    _add("lone_cr_fq_qual", b"@a\nA\n+\n\r\n@b\nAC\n+\nII\n")
    for tag, c in (("at", b"@"), ("plus", b"+"), ("gt", b">")):  # ends the sequence in the reference reader
        _add("fq_seq_opens_with_" + tag, b"@a\n" + c + b"CGT\n+\nIIII\n@b\nAC\n+\nII\n", bgzf=c == b"@")
        _add("fq_seq_is_" + tag, b"@a\nAC\n+\nII\n@b\n" + c + b"\n+\nI\n")
    _add("fa_seq_opens_with_at", b">a\nAC\n@CGT\nGG\n")
    _add("fa_seq_opens_with_plus", b">a\nAC\n+CGT\nGG\n")
    # irregular texts: refused, or the reference's sequences
    s = dna(50, 9)
    _add("multi_line_fq", b"@a\n" + s[:25] + b"\n" + s[25:] + b"\n+\n" + b"I" * 25 + b"\n" + b"I" * 25 + b"\n")
    _add("multi_line_fq_8", b"@a\nAC\nGT\n+\nII\nII\n@b\nAC\n+\nII\n")
    _add("junk_before_header", b"junk\n>a\nACGT\n")
    _add("junk_before_header_fq", b"junk\n@a\nACGT\n+\nIIII\n")
    _add("at_line_in_fasta", b">a\nACGT\n@b\nAC\n+\nII\n")
    _add("qual_short", b"@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", bgzf=True)
    _add("qual_long", b"@a\nACGT\n+\nIIIII\n@b\nAC\n+\nII\n")
    _add("qual_missing", b"@a\nACGT\n+\n")
    _add("three_line_fq", b"@a\nACGT\n+\n@b\nAC\n+\nII\n")
    _add("fasta_in_fastq", b"@a\nACGT\n+\nIIII\n>b\nAC\n")


_newline_geometry()
_gather_geometry()
_counts()
_fixed_length()
_text_ends()
_rules()


def _alternate():
    by_size = sorted(CASES, key=lambda k: (len(CASES[k]), k))
    small, large = by_size[:len(by_size) // 2], by_size[len(by_size) // 2:][::-1]
    out = []
    for a, b in zip(large, small):
        out += [a, b]
    return out + large[len(small):]


# irregular by the letter of is_regular (a lone '\r' line) but accepted before the lone-'\r' refusals and still: the line stands behind bases
STILL_ACCEPTED = ("lone_cr_after_bases", "lone_cr_after_one_base", "lone_cr_last_after_bases", "line_lengths_crlf")


def expected_fixed_len(seqs):
    """the read length a batch of these sequences records: more than one record, all of one length (0: not fixed)"""
    return len(seqs[0]) if len(seqs) > 1 and len({len(x) for x in seqs}) == 1 else 0


def recorded():
    """name -> {"text": digest, "ref": verdict}: what the reference reader returned (tests/golden/make_ref_golden.py)"""
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_verdicts.json")) as f:
        return json.load(f)["parser_cases"]


ORDER = _alternate()
assert sorted(ORDER) == sorted(CASES)
