"""What the chain's entry points refuse, word for word: the status code and the exact bl_last_error() text of every refusal that a small
batch reaches, and which of two bad arguments is reported.  The units of the chain (count table, lookup, per-read counts, quantiles,
select, correct, graph, links, clean, steps, text, BGZF) share their argument checks; this file pins what a caller sees of them.

The expected codes and texts are literals, recorded from the library as it stood before the checks were shared.  Every case is refused
before anything is launched; all the same every pointer that is not NULL is a real device buffer large enough for the call, and a
misaligned one lies eight bytes into such a buffer.  (The 2^31 cap of a range needs a batch of that size: the edge tests have it.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXPECTED = {
    'kmers/foreign_batch': (-1, 'ctx/batch is NULL or the batch belongs to another context'),
    'kmers/first_beyond': (-1, 'range starts beyond the batch'),
    'kmers/k_then_range': (-1, 'k must be in [1, 32] (KmerType = uint64_t)'),
    'kmers/batch_then_k': (-1, 'ctx/batch is NULL or the batch belongs to another context'),
    'kmers128/foreign_batch': (-1, 'ctx/batch is NULL or the batch belongs to another context'),
    'kmers128/first_beyond': (-1, 'range starts beyond the batch'),
    'kmers128/k_then_range': (-1, 'k must be in [1, 64] (KmerType = __uint128_t)'),
    'kmers128/batch_then_k': (-1, 'ctx/batch is NULL or the batch belongs to another context'),
    'kmers128/misaligned_values': (-1, 'd_values must be 16-byte aligned (one __uint128_t per record)'),
    'kmers128/misaligned_then_range': (-1, 'd_values must be 16-byte aligned (one __uint128_t per record)'),
    'kmer_counts/foreign_batch': (-1, 'ctx/batch is NULL or the batch belongs to another context'),
    'kmer_counts/foreign_table': (-1, 'the table belongs to another context'),
    'kmer_counts/first_beyond': (-1, 'range starts beyond the batch'),
    'kmer_counts/one_word_k33': (-1, 'a table of one-word keys takes k <= 32'),
    'kmer_counts/2k_above_key_bits': (-1, "2k = 12 exceeds the table's key_bits = 10"),
    'kmer_counts/two_words_k34': (-1, "2k = 68 exceeds the table's key_bits = 66"),
    'kmer_counts/table_then_k': (-1, 'the table belongs to another context'),
    'kmer_counts/k_then_batch': (-1, "2k = 12 exceeds the table's key_bits = 10"),
    'kmer_counts/k33_then_range': (-1, 'range starts beyond the batch'),
    'kmer_counts/no_context': (-1, 'ctx/batch is NULL or the batch belongs to another context'),
    'kmer_counts/no_context_k6': (-1, "2k = 12 exceeds the table's key_bits = 10"),
    'read_counts/foreign_batch': (-1, 'ctx/batch is NULL or the batch belongs to another context'),
    'read_counts/foreign_table': (-1, 'the table belongs to another context'),
    'read_counts/first_beyond': (-1, 'range starts beyond the batch'),
    'read_counts/no_offsets': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'read_counts/one_word_k33': (-1, 'a table of one-word keys takes k <= 32'),
    'read_counts/2k_above_key_bits': (-1, "2k = 12 exceeds the table's key_bits = 10"),
    'read_counts/misaligned_records': (-1, 'd_records must be 16-byte aligned'),
    'read_counts/misaligned_then_offsets': (-1, 'd_records must be 16-byte aligned'),
    'read_counts/offsets_then_batch': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'read_counts/k_then_min_count': (-1, "2k = 12 exceeds the table's key_bits = 10"),
    'read_counts/offsets_then_range': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'read_counts/no_context': (-1, 'ctx/batch is NULL or the batch belongs to another context'),
    'read_edits/foreign_batch': (-1, 'the batch belongs to another context'),
    'read_edits/foreign_table': (-1, 'the table belongs to another context'),
    'read_edits/first_beyond': (-1, 'range starts beyond the batch'),
    'read_edits/one_word_k33': (-1, 'a table of one-word keys takes k <= 32'),
    'read_edits/2k_above_key_bits': (-1, "2k = 12 exceeds the table's key_bits = 10"),
    'read_edits/misaligned_edits': (-1, 'd_edits must be 16-byte aligned'),
    'read_edits/batch_then_table': (-1, 'the batch belongs to another context'),
    'read_edits/table_then_misaligned': (-1, 'the table belongs to another context'),
    'read_edits/misaligned_then_k': (-1, 'd_edits must be 16-byte aligned'),
    'read_edits/k_then_range': (-1, "2k = 12 exceeds the table's key_bits = 10"),
    'read_edits/flags_then_range': (-1, 'flags: BL_FLAG_CANONICAL only (BL_FLAG_SYNC is accepted)'),
    'apply_edits/foreign_batch': (-1, 'the batch belongs to another context'),
    'apply_edits/misaligned_edits': (-1, 'd_edits must be 16-byte aligned'),
    'apply_edits/batch_then_misaligned': (-1, 'the batch belongs to another context'),
    'read_steps/foreign_batch': (-1, 'the batch belongs to another context'),
    'read_steps/foreign_table': (-1, 'the table belongs to another context'),
    'read_steps/first_beyond': (-1, 'range starts beyond the batch'),
    'read_steps/no_offsets': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'read_steps/one_word_k33': (-1, "2k = 66 exceeds the table's key_bits = 10"),
    'read_steps/2k_above_key_bits': (-1, "2k = 14 exceeds the table's key_bits = 10"),
    'read_steps/misaligned_steps': (-1, 'd_steps must be 16-byte aligned'),
    'read_steps/batch_then_table': (-1, 'the batch belongs to another context'),
    'read_steps/table_then_k': (-1, 'the table belongs to another context'),
    'read_steps/offsets_then_misaligned': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'read_steps/misaligned_then_range': (-1, 'd_steps must be 16-byte aligned'),
    'link_support/misaligned_steps': (-1, 'd_steps must be 16-byte aligned'),
    'format_gaf/foreign_batch': (-1, 'the batch belongs to another context'),
    'format_gaf/no_offsets': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'format_gaf/misaligned_out': (-1, 'd_out must be 16-byte aligned'),
    'format_gaf/misaligned_steps': (-1, 'd_steps must be 16-byte aligned'),
    'format_gaf/batch_then_offsets': (-1, 'the batch belongs to another context'),
    'format_gaf/offsets_then_misaligned': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'select_read_counts/foreign_batch': (-1, 'the batch belongs to another context'),
    'select_read_counts/first_beyond': (-1, 'range starts beyond the batch'),
    'select_read_counts/no_offsets': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'select_read_counts/batch_then_n_q': (-1, 'the batch belongs to another context'),
    'select_read_counts/n_q_then_range': (-1, 'n_q must be 1 .. 4'),
    'select_read_counts/range_then_offsets': (-1, 'range starts beyond the batch'),
    'batch_select/foreign_batch': (-1, 'the batch belongs to another context'),
    'batch_select/no_offsets': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'batch_select/misaligned_spans': (-1, 'd_spans must be 16-byte aligned'),
    'batch_select/misaligned_then_batch': (-1, 'd_spans must be 16-byte aligned'),
    'batch_select/batch_then_offsets': (-1, 'the batch belongs to another context'),
    'read_spans/foreign_batch': (-1, 'the batch belongs to another context'),
    'read_spans/no_offsets': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'read_spans/misaligned_spans': (-1, 'd_records and d_spans must be 16-byte aligned'),
    'read_spans/misaligned_then_batch': (-1, 'd_records and d_spans must be 16-byte aligned'),
    'read_spans/batch_then_offsets': (-1, 'the batch belongs to another context'),
    'batch_format/foreign_batch': (-1, 'the batch belongs to another context'),
    'batch_format/no_offsets': (-1, 'd_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets'),
    'batch_format/misaligned_out': (-1, 'd_out must be 16-byte aligned'),
    'batch_format/misaligned_spans': (-1, 'd_spans must be 16-byte aligned'),
    'batch_format/misaligned_then_batch': (-1, 'd_out must be 16-byte aligned'),
    'batch_format/batch_then_offsets': (-1, 'the batch belongs to another context'),
    'format_gfa/foreign_batch': (-1, 'the batch belongs to another context'),
    'format_gfa/misaligned_out': (-1, 'd_out must be 16-byte aligned'),
    'format_gfa/misaligned_then_batch': (-1, 'd_out must be 16-byte aligned'),
    'unitig_links/foreign_table': (-1, 'the table belongs to another context'),
    'table_adjacency/foreign_table': (-1, 'the table belongs to another context'),
    'table_unitigs/foreign_table': (-1, 'the table belongs to another context'),
    'remove_unitigs/foreign_table': (-1, 'the table belongs to another context'),
    'table_lookup/foreign_table': (-1, 'the table belongs to another context'),
    'table_lookup128/misaligned_queries': (-1, 'arrays of 16-byte keys must be 16-byte aligned'),
    'table_lookup128/table_then_misaligned': (-1, 'the table belongs to another context'),
    'table_build128/misaligned_keys': (-1, 'arrays of 16-byte keys must be 16-byte aligned'),
    'table_histogram/foreign_table': (-1, 'the table belongs to another context'),
    'table_combine/foreign_left': (-1, 'the table belongs to another context'),
    'table_combine/foreign_right': (-1, 'the table belongs to another context'),
    'bgzf_deflate/misaligned_out': (-1, 'bl_bgzf_deflate: d_out must be 16-byte aligned'),
}


class Env:
    """Two contexts; in the first a ragged batch of two 40-base reads, a one-word table of four 5-mers (key_bits 10) and a two-word
    table of 33-mers (key_bits 66); in the second a batch and a table of the same kind."""

    def __init__(self):
        import torch

        import biolib_amd
        from biolib_amd import capi

        self.capi = capi
        self.a = biolib_amd.Context(0)
        self.b = biolib_amd.Context(0)
        self.lib = self.a._lib
        dev = self.a.torch_device
        reads = np.frombuffer(b"ACGTTGCAAC" * 8, dtype=np.uint8)
        self.bases = torch.zeros(256, dtype=torch.uint8, device=dev)  # 80 bases and zeros behind them
        self.bases[:80] = torch.from_numpy(reads.copy()).to(dev)
        self.offsets = torch.tensor([0, 40, 80], dtype=torch.int64, device=dev)
        self.ragged = self._batch(self.a)
        self.foreign = self._batch(self.b)
        five = torch.tensor([0x1B, 0x6C, 0x1B1, 0x2C6], dtype=torch.int64, device=dev)  # four 5-mers: 10 bits each
        wide = torch.tensor([[5, 1], [9, 2]], dtype=torch.int64, device=dev)  # two 33-mers: 66 bits each
        self.t10 = self.a.count_table(five, key_bits=10)
        self.t66 = self.a.count_table(wide, key_bits=66)
        self.t10_foreign = self.b.count_table(five, key_bits=10)
        # what the calls would write or read had they gone on: zeros, 64 KiB each
        self.out = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        self.aux = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        self.more = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def _batch(self, ctx):
        h = C.c_void_p()
        offs = np.array([0, 40, 80], dtype=np.uint64)
        self.capi.check(ctx._lib.bl_batch_from_device(ctx._h, C.c_void_p(self.bases.data_ptr()), 80, offs.ctypes.data_as(C.c_void_p), 2, 0, C.byref(h)))
        assert ctx._lib.bl_batch_n_seqs(h) == 2
        return h

    def close(self):
        for ctx, h in ((self.a, self.ragged), (self.b, self.foreign)):
            ctx._lib.bl_batch_destroy(h)
        for t in (self.t10, self.t66, self.t10_foreign):
            t.close()
        self.b.close()
        self.a.close()


def p(t, shift=0):
    return C.c_void_p(t.data_ptr() + shift)


def cases(e):
    """id -> the call, as a function that returns the status code"""
    capi, L = e.capi, e.lib
    A, B = e.a._h, e.b._h
    ragged, foreign = e.ragged, e.foreign
    t10, t66, t10f = e.t10._h, e.t66._h, e.t10_foreign._h
    offs, out, aux, more = p(e.offsets), p(e.out), p(e.aux), p(e.more)
    odd = p(e.out, 8)  # misaligned
    SYNC = capi.FLAG_SYNC
    past = 81  # n_bases + 1
    c = {}

    def kmers(fn, ctx=A, batch=ragged, first=0, k=5, values=out):
        return lambda: fn(ctx, batch, first, 0, k, 0, SYNC, values, aux, more, C.byref(capi.Result()))

    for name, fn in (("kmers", L.bl_scan_kmers), ("kmers128", L.bl_scan_kmers128)):
        c[name + "/foreign_batch"] = kmers(fn, batch=foreign)
        c[name + "/first_beyond"] = kmers(fn, first=past)
        c[name + "/k_then_range"] = kmers(fn, k=99, first=past)
        c[name + "/batch_then_k"] = kmers(fn, batch=foreign, k=99)
    c["kmers128/misaligned_values"] = kmers(L.bl_scan_kmers128, values=odd)
    c["kmers128/misaligned_then_range"] = kmers(L.bl_scan_kmers128, values=odd, first=past)

    def kmer_counts(ctx=A, batch=ragged, first=0, k=5, table=t10):
        return lambda: L.bl_scan_kmer_counts(ctx, batch, first, 0, k, SYNC, table, out, aux, C.byref(capi.Result()))

    c["kmer_counts/foreign_batch"] = kmer_counts(batch=foreign)
    c["kmer_counts/foreign_table"] = kmer_counts(table=t10f)
    c["kmer_counts/first_beyond"] = kmer_counts(first=past)
    c["kmer_counts/one_word_k33"] = kmer_counts(k=33)
    c["kmer_counts/2k_above_key_bits"] = kmer_counts(k=6)
    c["kmer_counts/two_words_k34"] = kmer_counts(table=t66, k=34)
    c["kmer_counts/table_then_k"] = kmer_counts(table=t10f, k=33)
    c["kmer_counts/k_then_batch"] = kmer_counts(batch=foreign, k=6)
    c["kmer_counts/k33_then_range"] = kmer_counts(table=t66, k=33, first=past)
    c["kmer_counts/no_context"] = kmer_counts(ctx=None)
    c["kmer_counts/no_context_k6"] = kmer_counts(ctx=None, k=6)

    def read_counts(ctx=A, batch=ragged, first=0, k=5, table=t10, min_count=1, offsets=offs, records=out):
        return lambda: L.bl_scan_read_counts(ctx, batch, first, 0, k, SYNC, table, min_count, offsets, capi.READ_COUNTS_INIT, records, C.byref(capi.Result()))

    c["read_counts/foreign_batch"] = read_counts(batch=foreign)
    c["read_counts/foreign_table"] = read_counts(table=t10f)
    c["read_counts/first_beyond"] = read_counts(first=past)
    c["read_counts/no_offsets"] = read_counts(offsets=None)
    c["read_counts/one_word_k33"] = read_counts(k=33)
    c["read_counts/2k_above_key_bits"] = read_counts(k=6)
    c["read_counts/misaligned_records"] = read_counts(records=odd)
    c["read_counts/misaligned_then_offsets"] = read_counts(records=odd, offsets=None)
    c["read_counts/offsets_then_batch"] = read_counts(offsets=None, batch=foreign)
    c["read_counts/k_then_min_count"] = read_counts(k=6, min_count=0)
    c["read_counts/offsets_then_range"] = read_counts(offsets=None, first=past)
    c["read_counts/no_context"] = read_counts(ctx=None)

    def read_edits(batch=ragged, first=0, k=5, flags=0, table=t10, edits=out):
        return lambda: L.bl_scan_read_edits(A, batch, first, 0, k, flags, table, 1, 1, edits, 16, C.byref(capi.EditStats()))

    c["read_edits/foreign_batch"] = read_edits(batch=foreign)
    c["read_edits/foreign_table"] = read_edits(table=t10f)
    c["read_edits/first_beyond"] = read_edits(first=past)
    c["read_edits/one_word_k33"] = read_edits(k=33)
    c["read_edits/2k_above_key_bits"] = read_edits(k=6)
    c["read_edits/misaligned_edits"] = read_edits(edits=odd)
    c["read_edits/batch_then_table"] = read_edits(batch=foreign, table=t10f)
    c["read_edits/table_then_misaligned"] = read_edits(table=t10f, edits=odd)
    c["read_edits/misaligned_then_k"] = read_edits(edits=odd, k=33)
    c["read_edits/k_then_range"] = read_edits(k=6, first=past)
    c["read_edits/flags_then_range"] = read_edits(flags=capi.FLAG_DROP_LAST, first=past)

    def apply_edits(batch=ragged, edits=out):
        return lambda: L.bl_batch_apply_edits(A, batch, edits, 1, C.byref(C.c_void_p()))

    c["apply_edits/foreign_batch"] = apply_edits(batch=foreign)
    c["apply_edits/misaligned_edits"] = apply_edits(edits=odd)
    c["apply_edits/batch_then_misaligned"] = apply_edits(batch=foreign, edits=odd)

    def read_steps(batch=ragged, first=0, k=5, table=t10, offsets=offs, steps=out):
        return lambda: L.bl_scan_read_steps(A, batch, first, 0, k, 0, table, aux, more, 1, offsets, steps, 4, C.byref(capi.StepStats()))

    c["read_steps/foreign_batch"] = read_steps(batch=foreign)
    c["read_steps/foreign_table"] = read_steps(table=t10f)
    c["read_steps/first_beyond"] = read_steps(first=past)
    c["read_steps/no_offsets"] = read_steps(offsets=None)
    c["read_steps/one_word_k33"] = read_steps(k=33)
    c["read_steps/2k_above_key_bits"] = read_steps(k=7)
    c["read_steps/misaligned_steps"] = read_steps(steps=odd)
    c["read_steps/batch_then_table"] = read_steps(batch=foreign, table=t10f)
    c["read_steps/table_then_k"] = read_steps(table=t10f, k=7)
    c["read_steps/offsets_then_misaligned"] = read_steps(offsets=None, steps=odd)
    c["read_steps/misaligned_then_range"] = read_steps(steps=odd, first=past)

    c["link_support/misaligned_steps"] = lambda: L.bl_link_support(A, odd, 1, aux, more, 0, 1, None, C.byref(capi.SupportStats()))

    def gaf(batch=ragged, offsets=offs, steps=aux, text=out):
        rule = capi.GafRule()
        rule.k, rule.read_prefix, rule.segment_prefix = 5, b"r", b"s"
        return lambda: L.bl_steps_format_gaf(A, batch, offsets, steps, 0, more, 0, C.byref(rule), text, 1 << 15, C.byref(C.c_uint64()))

    c["format_gaf/foreign_batch"] = gaf(batch=foreign)
    c["format_gaf/no_offsets"] = gaf(offsets=None)
    c["format_gaf/misaligned_out"] = gaf(text=odd)
    c["format_gaf/misaligned_steps"] = gaf(steps=p(e.aux, 8))
    c["format_gaf/batch_then_offsets"] = gaf(batch=foreign, offsets=None)
    c["format_gaf/offsets_then_misaligned"] = gaf(offsets=None, text=odd)

    q_num, q_den = (C.c_uint32 * 1)(1), (C.c_uint32 * 1)(2)

    def quantiles(batch=ragged, first=0, offsets=offs, n_q=1):
        return lambda: L.bl_select_read_counts(A, batch, first, 0, aux, more, offsets, q_num, q_den, n_q, out, None)

    c["select_read_counts/foreign_batch"] = quantiles(batch=foreign)
    c["select_read_counts/first_beyond"] = quantiles(first=past)
    c["select_read_counts/no_offsets"] = quantiles(offsets=None)
    c["select_read_counts/batch_then_n_q"] = quantiles(batch=foreign, n_q=0)
    c["select_read_counts/n_q_then_range"] = quantiles(n_q=0, first=past)
    c["select_read_counts/range_then_offsets"] = quantiles(first=past, offsets=None)

    def select(batch=ragged, offsets=offs, spans=aux):
        return lambda: L.bl_batch_select(A, batch, offsets, spans, 0, C.byref(C.c_void_p()), None, None, C.byref(C.c_uint64()), C.byref(C.c_uint64()))

    c["batch_select/foreign_batch"] = select(batch=foreign)
    c["batch_select/no_offsets"] = select(offsets=None)
    c["batch_select/misaligned_spans"] = select(spans=odd)
    c["batch_select/misaligned_then_batch"] = select(spans=odd, batch=foreign)
    c["batch_select/batch_then_offsets"] = select(batch=foreign, offsets=None)

    def read_spans(batch=ragged, offsets=offs, spans=out):
        rule = capi.SpanRule()
        rule.k, rule.solid_min_den, rule.solid_max_num, rule.solid_max_den = 5, 1, 1, 1
        return lambda: L.bl_read_spans(A, batch, offsets, aux, None, C.byref(rule), spans)

    c["read_spans/foreign_batch"] = read_spans(batch=foreign)
    c["read_spans/no_offsets"] = read_spans(offsets=None)
    c["read_spans/misaligned_spans"] = read_spans(spans=odd)
    c["read_spans/misaligned_then_batch"] = read_spans(spans=odd, batch=foreign)
    c["read_spans/batch_then_offsets"] = read_spans(batch=foreign, offsets=None)

    def fmt(batch=ragged, offsets=offs, spans=None, text=out):
        rule = capi.FormatRule()
        rule.format, rule.quality_fill = capi.FORMAT_FASTA, 73
        return lambda: L.bl_batch_format(A, batch, offsets, None, None, spans, None, C.byref(rule), text, 1 << 15, C.byref(C.c_uint64()), C.byref(C.c_uint64()))

    c["batch_format/foreign_batch"] = fmt(batch=foreign)
    c["batch_format/no_offsets"] = fmt(offsets=None)
    c["batch_format/misaligned_out"] = fmt(text=odd)
    c["batch_format/misaligned_spans"] = fmt(spans=p(e.aux, 8))
    c["batch_format/misaligned_then_batch"] = fmt(text=odd, batch=foreign)
    c["batch_format/batch_then_offsets"] = fmt(batch=foreign, offsets=None)

    def gfa(batch=ragged, text=out):
        rule = capi.GfaRule()
        rule.k = 5
        return lambda: L.bl_unitigs_format_gfa(A, batch, aux, 0, None, None, 0, C.byref(rule), text, 1 << 15, C.byref(C.c_uint64()))

    c["format_gfa/foreign_batch"] = gfa(batch=foreign)
    c["format_gfa/misaligned_out"] = gfa(text=odd)
    c["format_gfa/misaligned_then_batch"] = gfa(text=odd, batch=foreign)

    # the table's owner, in the calls that take no batch
    c["unitig_links/foreign_table"] = lambda: L.bl_unitig_links(A, t10f, 5, aux, more, 1, 0, None, None, 0, C.byref(C.c_uint64()), C.byref(capi.LinkStats()))
    c["table_adjacency/foreign_table"] = lambda: L.bl_table_adjacency(A, t10f, 5, out, None, C.byref(capi.GraphStats()))
    c["table_unitigs/foreign_table"] = lambda: L.bl_table_unitigs(A, t10f, 5, None, None, None, None, C.byref(C.c_uint64()), C.byref(C.c_uint64()), C.byref(capi.GraphStats()))
    c["remove_unitigs/foreign_table"] = lambda: L.bl_table_remove_unitigs(A, t10f, aux, more, 1, C.byref(C.c_void_p()), C.byref(C.c_uint64()))
    c["table_lookup/foreign_table"] = lambda: L.bl_table_lookup_u64(A, t10f, aux, 1, out)
    c["table_lookup128/misaligned_queries"] = lambda: L.bl_table_lookup_u128(A, t66, odd, 1, aux)
    c["table_lookup128/table_then_misaligned"] = lambda: L.bl_table_lookup_u128(A, t10f, odd, 1, aux)
    c["table_build128/misaligned_keys"] = lambda: L.bl_table_build_u128(A, odd, None, 1, 66, C.byref(C.c_void_p()))
    hist = (C.c_uint64 * 4)()
    c["table_histogram/foreign_table"] = lambda: L.bl_table_histogram(A, t10f, hist, 4)
    c["table_combine/foreign_left"] = lambda: L.bl_table_combine(A, t10f, t10, capi.TABLE_UNION, capi.COUNT_SUM, 0, 2**32 - 1, C.byref(C.c_void_p()), None)
    c["table_combine/foreign_right"] = lambda: L.bl_table_combine(A, t10, t10f, capi.TABLE_UNION, capi.COUNT_SUM, 0, 2**32 - 1, C.byref(C.c_void_p()), None)
    c["bgzf_deflate/misaligned_out"] = lambda: L.bl_bgzf_deflate(A, aux, 16, 0, odd, 1 << 15, C.byref(C.c_uint64()), None, C.byref(C.c_uint64()))
    return c


def observe(e, call):
    """(status code, bl_last_error() text) of one call; a call that is not refused has no text"""
    rc = call()
    return rc, (e.lib.bl_last_error().decode() if rc != 0 else "")


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.calls = cases(e)
    yield e
    e.close()


def test_every_case_has_its_record(env):
    assert sorted(env.calls) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_refusal(env, case):
    got = observe(env, env.calls[case])
    print(case, got)
    assert got == EXPECTED[case]
