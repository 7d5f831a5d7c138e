"""CPU-only: the Python specification of bl_bgzf_deflate (deflate_cases.py) judged by zlib — every named case inflates to its text, every
member's header, BSIZE, CRC-32 and ISIZE are right, no member is larger than its text + 31 bytes and no output larger than
bl_bgzf_bound — the counters over the case set (all three block forms, the length limiter, match lengths 3 and 258, distances 1 and
32,768), and the ratio caps, which zlib level 1 on the same 65,280-byte blocks must meet as well."""
import gzip

import pytest

import deflate_cases as DC

CASES = DC.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_valid_bgzf(name):
    text, eof = CASES[name]
    out, counters, table = DC.bgzf_model(text, eof)
    assert (gzip.decompress(out) if out else b"") == text
    assert DC.check_members(out, text, eof) == len(table) == (len(text) + DC.MEMBER - 1) // DC.MEMBER
    assert len(out) <= DC.bound(len(text), eof)
    for src_off, dst_off, src_len, isize, crc in table:
        assert out[src_off - 18:src_off - 14] == b"\x1f\x8b\x08\x04" and text[dst_off:dst_off + isize] == DC.zlib.decompress(out[src_off:src_off + src_len], -15)


def test_empty_text():
    assert DC.bgzf_model(b"", True)[0] == DC.EOF_MARKER and DC.bgzf_model(b"", False)[0] == b""
    assert DC.bound(0, True) == 28 and DC.bound(0, False) == 0 and DC.bound(65281, True) == 65281 + 62 + 28


def test_what_each_case_is_there_for():
    c = {name: DC.bgzf_model(*CASES[name])[1] for name in CASES}
    assert c["member_plus_1"]["forms"] == [0, 1, 1], "the second member holds one byte: fixed codes"
    assert c["four_kinds"]["forms"][0] >= 1 and c["four_kinds"]["forms"][2] >= 1
    r = c["one_byte_repeated"]
    assert (r["max_len"], r["max_dist"], r["min_dist"], r["forms"]) == (258, 1, 1, [0, 0, 1]), "distance 1 only: a single distance symbol"
    assert c["no_match"]["max_len"] == 0 and c["no_match"]["forms"] == [0, 0, 1], "no distance symbol used: the padding rule, in a dynamic block"
    assert c["twenty_bytes"]["forms"] == [0, 1, 0] and c["random_bytes"]["forms"] == [1, 0, 0]
    assert c["fibonacci"]["limited"] == 1 and c["fibonacci"]["max_len"] == 0 and c["fibonacci"]["forms"] == [0, 0, 1]
    assert c["far_32768"]["max_dist"] == 32768, "the furthest distance the matcher reaches by design"
    assert c["far_32769"]["max_dist"] < 32768 and c["far_32769"]["max_len"] < 100, "one byte further: not matched"
    for r in range(8):
        text = CASES["ends_at_bit_%d" % r][0]
        assert DC.member_model(text)[1]["data_bits"] % 8 == r and DC.member_model(text)[1]["form"] == 2


def test_counters_over_the_case_set():
    forms, limited, lens, dists = [0, 0, 0], 0, set(), set()
    for name in CASES:
        c = DC.bgzf_model(*CASES[name])[1]
        forms = [a + b for a, b in zip(forms, c["forms"])]
        limited += c["limited"]
        lens |= {c["max_len"], c["min_len"]}
        dists |= {c["max_dist"], c["min_dist"]}
    assert all(forms) and limited and {3, 258} <= lens and {1, 32768} <= dists, (forms, limited, lens, dists)


@pytest.mark.parametrize("name", sorted(DC.ratio_texts()))
def test_ratio_caps(name):
    """conditions, not measurements: zlib level 1 stays inside them, and so must the model"""
    text, cap = DC.ratio_texts()[name]
    out = DC.bgzf_model(text)[0]
    assert gzip.decompress(out) == text
    z1, ours = DC.zlib_bgzf_size(text, 1) / len(text), (len(out) - 28) / len(text)
    print(name, "model", round(ours, 4), "zlib 1", round(z1, 4), "zlib 6", round(DC.zlib_bgzf_size(text, 6) / len(text), 4))
    assert z1 <= cap, "the reference fails the cap"
    assert ours <= cap
