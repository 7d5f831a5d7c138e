"""Host-side binding of the scan entry points (thin; all work happens in the HIP library).

Device memory for outputs comes from torch (plumbing only): int64 CUDA tensors whose storage the
kernels fill with uint64 records; `.view(np.uint64)` on the host copy restores the type.
"""
import ctypes as C
import math
import weakref

import numpy as np

from . import capi
from .capi import FLAG_CANONICAL, FLAG_DROP_LAST, FLAG_SYNC, READ_COUNTS_ACCUMULATE, READ_COUNTS_INIT, BiolibError, Result, check


def hash64(value, seed=0):
    """hash::hash64::hash<uint64_t>(value, seed) (include/hash.hpp:55-59), bit-exact, on the host."""
    return int(capi.lib().bl_hash64_u64(int(value) & (2**64 - 1), int(seed) & (2**64 - 1)))


def hash64_u128(lo, hi, seed=0):
    """hash::hash64::hash<__uint128_t>(hi << 64 | lo, seed): the hash of the 128-bit k-mer scans (16 key bytes), bit-exact, on the host."""
    m = 2**64 - 1
    return int(capi.lib().bl_hash64_u128(int(lo) & m, int(hi) & m, int(seed) & m))


def _flags(canonical=False, drop_last=False, sync=False):
    return (FLAG_CANONICAL if canonical else 0) | (FLAG_DROP_LAST if drop_last else 0) | (FLAG_SYNC if sync else 0)


def _names(call):
    need = C.c_uint64()
    call(None, 0, C.byref(need))  # BL_ERR_CAPACITY: how many bytes
    buf = C.create_string_buffer(int(need.value))
    check(call(buf, len(buf), C.byref(need)))
    return buf.value.decode().split()


class Context:
    """One context per (process, GPU): owns the stream-ordered workspace of the scans."""

    def __init__(self, device=0, torch_stream=True, lanes=1):
        import torch

        if not torch.cuda.is_available():
            raise BiolibError(capi.BL_ERR_NO_DEVICE, "no GPU visible: biolib_amd has no CPU fallback")
        self._lib = capi.lib()
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        h = C.c_void_p()
        check(self._lib.bl_ctx_create(self.device, C.byref(h)))
        self._h = h
        self._batches = weakref.WeakSet()
        self._tables = weakref.WeakSet()
        self._pending = []  # Result structs of asynchronous scans: the library fills them at the next sync
        self._borrowed = bool(torch_stream)
        if torch_stream:
            self.use_torch_stream()
        elif lanes != 1:
            # own streams only: consecutive asynchronous scans overlap (they must not share output arrays)
            check(self._lib.bl_ctx_set_lanes(self._h, int(lanes)))

    def use_torch_stream(self):
        """Run on torch's CURRENT stream (call again after switching torch streams): scans, set operations, torch kernels
        and RCCL collectives are then ordered with each other.  torch's default stream is the legacy stream, handle 0,
        which bl_ctx_set_stream honours as a stream (it does not mean "unset")."""
        import torch

        with torch.cuda.device(self.device):
            s = torch.cuda.current_stream(self.device).cuda_stream
        check(self._lib.bl_ctx_set_stream(self._h, C.c_void_p(s)))
        self._borrowed = True

    def _inputs_ready(self):
        """A context on its own streams is not ordered with torch: tensors produced by pending torch work (kernels,
        all-to-all payloads) must be complete before the library reads them."""
        if not self._borrowed:
            import torch

            torch.cuda.current_stream(self.device).synchronize()

    def close(self):
        if getattr(self, "_h", None):
            for b in list(self._batches):
                b.close()
            for t in list(self._tables):
                t.close()
            self._lib.bl_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._lib.bl_ctx_sync(self._h))
        self._pending.clear()

    def last_scan_ms(self):
        ms = C.c_float()
        check(self._lib.bl_ctx_last_scan_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def set_exact_windows(self, on=True):
        """Later scans decide their windows on the 64-bit hashes themselves (bl_ctx_set_exact_windows): same records, for checks and A/B runs.
        Result.redone counts the tiles a default scan had to decide a second time."""
        check(self._lib.bl_ctx_set_exact_windows(self._h, 1 if on else 0))

    def set_option(self, name, value):
        """tuning / test switches by name (bl_ctx_set_option: "exact_windows", "lanes", "position_tiled", "packed_codes", "direct_codes", "emit_lds_bytes",
        "count128_tables", "jaccard128_path", "table_prefix_bits")"""
        check(self._lib.bl_ctx_set_option(self._h, name.encode(), int(value)))

    def last_scan_kernels(self):
        """names of the kernels the most recent window scan on this context launched, in launch order (bl_ctx_last_scan_kernels)"""
        return _names(lambda buf, cap, need: self._lib.bl_ctx_last_scan_kernels(self._h, buf, cap, need))

    @staticmethod
    def scan_kernel_names():
        """every name a scan's launch can record (bl_scan_kernel_names)"""
        return _names(capi.lib().bl_scan_kernel_names)

    def kernel_timing(self, enable=True):
        check(self._lib.bl_ctx_kernel_timing(self._h, 1 if enable else 0))

    def _hold(self, result, flags):
        """an asynchronous scan fills `result` at a later sync: keep it alive until then (bounded)"""
        if flags & FLAG_SYNC:
            return
        if len(self._pending) >= 4096:
            self.sync()
        self._pending.append(result)

    def kernel_time(self):
        """(total ms, launches) of the scan kernels alone since kernel_timing(True)."""
        ms, n = C.c_double(), C.c_uint64()
        check(self._lib.bl_ctx_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def mark(self):
        """a marker on the device's timeline behind everything issued so far (bl_ctx_mark): does not stop the device"""
        check(self._lib.bl_ctx_mark(self._h))

    def mark_times(self):
        """synchronises; milliseconds after the first marker at which the work in front of each marker had finished; forgets the markers"""
        n = C.c_uint32()
        check(self._lib.bl_ctx_mark_times(self._h, None, 0, C.byref(n)))  # capacity 0: how many there are (they stay)
        k = int(n.value)
        buf = (C.c_double * max(k, 1))()
        check(self._lib.bl_ctx_mark_times(self._h, buf, k, C.byref(n)))
        return [float(buf[i]) for i in range(k)]

    # ---- batches
    def upload(self, bases, offsets=None, read_len=0):
        """host bases -> device batch; sequences by `offsets`, or reads of one length `read_len` laid end to end (bl_batch_upload_reads)"""
        if isinstance(bases, str):
            bases = bases.encode()
        arr = np.frombuffer(bytes(bases), dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, dtype=np.uint8)
        if read_len:
            h = C.c_void_p()
            check(self._lib.bl_batch_upload_reads(self._h, arr.ctypes.data_as(C.c_void_p) if arr.size else None, arr.size, int(read_len), C.byref(h)))
            return Batch(self, h, read_len=int(read_len))
        offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        check(self._lib.bl_batch_upload(self._h, arr.ctypes.data_as(C.c_void_p) if arr.size else None, arr.size,
                                        None if offs is None else offs.ctypes.data_as(C.c_void_p), 0 if offs is None else len(offs) - 1, C.byref(h)))
        return Batch(self, h, offsets=offs)

    def synth(self, seed, n_bases, read_len=0):
        h = C.c_void_p()
        check(self._lib.bl_batch_synth(self._h, int(seed), int(n_bases), int(read_len), C.byref(h)))
        return Batch(self, h, read_len=int(read_len))

    def from_text(self, text):
        """Parse raw FASTA / 4-line FASTQ text on the device (bl_batch_from_text).  text: bytes or a uint8 numpy array."""
        arr = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        h, ns, nb = C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(self._lib.bl_batch_from_text(self._h, arr.ctypes.data_as(C.c_void_p) if arr.size else None, arr.size, C.byref(h), C.byref(ns), C.byref(nb)))
        return Batch(self, h)

    def from_text_indexed(self, text):
        """from_text that keeps the names and qualities on the device (bl_text_index_build): (Batch, TextIndex).  The batch is
        from_text's, byte for byte, and carries its offsets on the device like the result of select; the index holds a device copy
        of the text (about 2.3 times the bases for FASTQ) until it is closed, and is what Batch.format / Batch.write take as `index`."""
        arr = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        h, ix, ns, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(self._lib.bl_text_index_build(self._h, arr.ctypes.data_as(C.c_void_p) if arr.size else None, arr.size, C.byref(h), C.byref(ix), C.byref(ns),
                                            C.byref(nb)))
        return _indexed_batch(self, h, ix)

    def from_tensor(self, t, offsets=None, read_len=0):
        """Wrap a uint8 CUDA tensor of ASCII bases (not copied; must stay alive)."""
        self._inputs_ready()
        assert t.is_cuda and t.dtype.itemsize == 1 and t.is_contiguous()
        offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        check(self._lib.bl_batch_from_device(self._h, C.c_void_p(t.data_ptr()), t.numel(),
                                             None if offs is None else offs.ctypes.data_as(C.c_void_p), 0 if offs is None else len(offs) - 1,
                                             int(read_len), C.byref(h)))
        b = Batch(self, h, offsets=offs, read_len=0 if offs is not None else int(read_len))
        b._keep = t
        return b

    # ---- set operations on device k-mer lists, run files and super-k-mer records: one implementation per operation, keyed by the 8-byte
    # words of an element.  Keys: 1 word (int64[n] CUDA tensors holding uint64 keys) or 2 (int64[n, 2]: low, high, as kmers128 /
    # expand_super_kmers128 return).  Records: 2 words (16 bytes, whose k-mers are one-word keys) or 4 (32 bytes: two-word keys).
    def _keys128(self, keys, n):
        if keys.dim() != 2 or keys.shape[1] != 2 or keys.element_size() != 8 or not keys.is_contiguous():
            raise ValueError("128-bit keys are a contiguous int64[n, 2] tensor (low, high)")
        n = keys.shape[0] if n is None else int(n)
        if n > keys.shape[0]:
            raise ValueError("n exceeds the tensor")
        self._inputs_ready()
        return n

    def _n_keys(self, words, keys, n):
        if words == 2:
            return self._keys128(keys, n)
        n = keys.numel() if n is None else int(n)
        self._inputs_ready()
        return n

    def _n_records(self, records, n):
        n = records.shape[0] if n is None else int(n)
        self._inputs_ready()
        return n

    def _key_call(self, name, words):
        return getattr(self._lib, f"bl_{name}_u{64 * words}")

    def _record_call(self, name, words):
        return getattr(self._lib, f"bl_{name}{'128' if words == 4 else ''}")

    def _empty_words(self, n, words):
        import torch

        n = max(int(n), 1)
        return torch.empty(n if words == 1 else (n, words), dtype=torch.int64, device=self.torch_device)

    def _sort_unique(self, words, keys, n, *key_bits):
        n = self._n_keys(words, keys, n)
        out = C.c_uint64()
        check(self._key_call("sort_unique", words)(self._h, C.c_void_p(keys.data_ptr()), n, *key_bits, C.byref(out)))
        return int(out.value)

    def _jaccard(self, words, a, na, b, nb):
        na, nb = self._n_keys(words, a, na), self._n_keys(words, b, nb)
        i, u = C.c_uint64(), C.c_uint64()
        check(self._key_call("jaccard_sorted", words)(self._h, C.c_void_p(a.data_ptr()), na, C.c_void_p(b.data_ptr()), nb, C.byref(i), C.byref(u)))
        return int(i.value), int(u.value)

    def _partition(self, words, keys, parts, seed, n):
        n = self._n_keys(words, keys, n)
        out = self._empty_words(n, words)
        counts = (C.c_uint64 * max(int(parts), 1))()
        check(self._key_call("partition", words)(self._h, C.c_void_p(keys.data_ptr()), n, int(parts), int(seed), C.c_void_p(out.data_ptr()), counts))
        return out[:n], [int(c) for c in counts]

    def _sort_count(self, words, keys, n, *key_bits):
        import torch

        n = self._n_keys(words, keys, n)
        check(self._key_call("sort", words)(self._h, C.c_void_p(keys.data_ptr()), n, *key_bits))
        uniq = self._empty_words(n, words)
        mult = torch.empty(max(n, 1), dtype=torch.int32, device=self.torch_device)
        runs = C.c_uint64()
        check(self._key_call("count_sorted", words)(self._h, C.c_void_p(keys.data_ptr()), n, C.c_void_p(uniq.data_ptr()), C.c_void_p(mult.data_ptr()), C.byref(runs)))
        return uniq[: runs.value], mult[: runs.value]

    def _read_file(self, words, path, with_count):
        n = C.c_uint64()
        check(self._key_call("file_count", words)(str(path).encode(), 1 if with_count else 0, C.byref(n)))
        out = self._empty_words(n.value, words)
        check(self._key_call("read_file", words)(self._h, str(path).encode(), 1 if with_count else 0, C.c_void_p(out.data_ptr()), n.value, C.byref(n)))
        return out[: n.value]

    def _merge_runs(self, words, paths):
        merge = self._key_call("merge_runs", words)
        arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
        total = C.c_uint64()
        rc = merge(self._h, arr, len(paths), None, 0, C.byref(total))
        if rc not in (0, capi.BL_ERR_CAPACITY):
            check(rc)
        out = self._empty_words(total.value, words)
        if total.value:
            check(merge(self._h, arr, len(paths), C.c_void_p(out.data_ptr()), total.value, C.byref(total)))
        return out[: total.value]

    def _partition_records(self, words, hashes, records, parts, n):
        n = self._n_records(records, n)
        out = self._empty_words(n, words)
        counts = (C.c_uint64 * int(parts))()
        check(self._record_call("partition_records", words)(self._h, C.c_void_p(hashes.data_ptr()), C.c_void_p(records.data_ptr()), n, int(parts),
                                                            C.c_void_p(out.data_ptr()), counts))
        return out[:n], [int(c) for c in counts]

    def _expand_super_kmers(self, words, records, k, canonical, n):
        expand = self._record_call("expand_super_kmers", words)
        n = self._n_records(records, n)
        need = C.c_uint64()
        flags = FLAG_CANONICAL if canonical else 0
        rc = expand(self._h, C.c_void_p(records.data_ptr()), n, int(k), flags, None, 0, C.byref(need))
        if rc not in (0, capi.BL_ERR_CAPACITY):
            check(rc)
        out = self._empty_words(need.value, words // 2)
        if need.value:
            check(expand(self._h, C.c_void_p(records.data_ptr()), n, int(k), flags, C.c_void_p(out.data_ptr()), need.value, C.byref(need)))
        return out[: need.value]

    def _count_super_kmers(self, words, records, k, m, seed, canonical, n, out=None):
        import torch

        n = self._n_records(records, n)
        flags = FLAG_CANONICAL if canonical else 0
        need = C.c_uint64()
        cap = int(n * (k - m + 1) * 0.62) + 4096  # groups average ~ (w+1)/2 k-mers; retried with the exact need if short
        while True:
            if out is not None:  # caller-owned (keys int64, counts int32) tensors: no allocation on this path
                keys, cnts = out
                cap = min(keys.shape[0], cnts.numel())
                out = None
            else:
                keys = self._empty_words(cap, words // 2)
                cnts = torch.empty(max(cap, 1), dtype=torch.int32, device=self.torch_device)
            rc = self._record_call("count_super_kmers", words)(self._h, C.c_void_p(records.data_ptr()), n, int(k), int(m), int(seed), flags,
                                                               C.c_void_p(keys.data_ptr()), C.c_void_p(cnts.data_ptr()), cap, C.byref(need))
            if rc == capi.BL_ERR_CAPACITY:
                cap = int(need.value) + 64
                continue
            check(rc)
            return keys[: need.value], cnts[: need.value]

    def sort_unique(self, keys, n=None):
        """in-place sort + unique of keys[:n]; returns the number of distinct keys now at the front"""
        return self._sort_unique(1, keys, n)

    def jaccard(self, a, na, b, nb):
        """(|A n B|, |A u B|) of two sorted duplicate-free key arrays"""
        return self._jaccard(1, a, na, b, nb)

    def partition(self, keys, parts, seed=0, n=None):
        """(bucketed copy of keys[:n], sizes[parts]): bucket b = keys with hash64(key, seed) % parts == b, contiguous, in bucket order"""
        return self._partition(1, keys, parts, seed, n)

    def sort_count(self, keys, n=None):
        """(distinct keys ascending, multiplicities) of keys[:n]; keys is sorted in place"""
        return self._sort_count(1, keys, n)

    def partition_records(self, hashes, records, parts, n=None):
        """(bucketed copy of the 16-byte records[:n], sizes[parts]): bucket b = records with hashes[i] % parts == b"""
        return self._partition_records(2, hashes, records, parts, n)

    def expand_super_kmers(self, records, k, canonical=True, n=None):
        """the k-mers (device tensor) the packed super-k-mer records stand for, group after group"""
        return self._expand_super_kmers(2, records, k, canonical, n)

    def count_super_kmers(self, records, k, m, seed=0, canonical=True, n=None, out=None):
        """(distinct k-mers, multiplicities) of the packed super-k-mer records, in no particular order: buckets by minimizer
        hash counted in LDS hash tables (bl_count_super_kmers), no global sort"""
        return self._count_super_kmers(2, records, k, m, seed, canonical, n, out)

    def read_file_u64(self, path, with_count=False):
        """a run file (raw sorted u64) or, with_count, an io::basic_store'd vector<uint64_t> of biolib -> device tensor"""
        return self._read_file(1, path, with_count)

    def merge_runs(self, paths):
        """the sorted union (duplicates kept) of biolib run files, on the device: what iterating the reference's
        external_memory_vector yields"""
        return self._merge_runs(1, paths)

    # ---- the same on 16-byte keys and 32-byte records
    def sort128(self, keys, key_bits=128, n=None):
        """in-place ascending sort of keys[:n] as 128-bit integers; key_bits = number of low bits that can be non-zero (2k for k-mers)"""
        n = self._keys128(keys, n)
        check(self._lib.bl_sort_u128(self._h, C.c_void_p(keys.data_ptr()), n, int(key_bits)))

    def sort_unique128(self, keys, key_bits=128, n=None):
        """in-place sort + unique of keys[:n]; returns the number of distinct keys now at the front"""
        return self._sort_unique(2, keys, n, int(key_bits))

    def jaccard128(self, a, na, b, nb):
        """(|A n B|, |A u B|) of two sorted duplicate-free arrays of 128-bit keys"""
        return self._jaccard(2, a, na, b, nb)

    def partition128(self, keys, parts, seed=0, n=None):
        """(bucketed copy of keys[:n], sizes[parts]): bucket b = keys with hash64_u128(lo, hi, seed) % parts == b, contiguous, in bucket order"""
        return self._partition(2, keys, parts, seed, n)

    def sort_count128(self, keys, key_bits=128, n=None):
        """(distinct keys ascending int64[d, 2], multiplicities int32[d]) of keys[:n]; keys is sorted in place"""
        return self._sort_count(2, keys, n, int(key_bits))

    def partition_records128(self, hashes, records, parts, n=None):
        """(bucketed copy of the 32-byte records[:n] — int64[n, 4] —, sizes[parts]): bucket b = records with hashes[i] % parts == b"""
        return self._partition_records(4, hashes, records, parts, n)

    def expand_super_kmers128(self, records, k, canonical=True, n=None):
        """the 128-bit k-mers (device tensor int64[n_kmers, 2]: low, high) the 32-byte super-k-mer records stand for, group after group"""
        return self._expand_super_kmers(4, records, k, canonical, n)

    def count_super_kmers128(self, records, k, m, seed=0, canonical=True, n=None):
        """(distinct 128-bit k-mers int64[d, 2] — low, high —, multiplicities int32[d]) of the 32-byte super-k-mer records, in no particular
        order (bl_count_super_kmers128)"""
        return self._count_super_kmers(4, records, k, m, seed, canonical, n)

    def read_file_u128(self, path, with_count=False):
        """a run file (raw sorted 16-byte keys) or, with_count, an io::basic_store'd vector<__uint128_t> of biolib -> int64[n, 2] device tensor"""
        return self._read_file(2, path, with_count)

    def merge_runs128(self, paths):
        """the sorted union (duplicates kept) of run files of 16-byte keys, on the device: what iterating the reference's
        external_memory_vector<__uint128_t> yields"""
        return self._merge_runs(2, paths)

    # ---- the count table: what takes the (keys, counts) pairs of the counters on
    def count_table(self, keys, counts=None, key_bits=None, n=None):
        """A CountTable of keys[:n] with counts[:n] (None: every entry counts 1).  An int64[n] tensor gives one-word keys, an int64[n, 2]
        tensor two-word keys (low, high), as sort128 takes them.  Any order, duplicates allowed: equal keys are merged, their counts added
        (saturating at 2^32 - 1).  key_bits: the number of low bits that can be non-zero (2k for k-mers; default: the full width).
        The inputs are not modified."""
        if keys.dim() == 2:
            n = self._keys128(keys, n)
            key_words = 2
        else:
            if keys.dim() != 1 or keys.element_size() != 8 or not keys.is_contiguous():
                raise ValueError("keys are a contiguous int64[n] or int64[n, 2] tensor")
            n = keys.numel() if n is None else int(n)
            if n > keys.numel():
                raise ValueError("n exceeds the tensor")
            self._inputs_ready()
            key_words = 1
        if counts is not None and (counts.element_size() != 4 or not counts.is_contiguous() or counts.numel() < n):
            raise ValueError("counts are a contiguous int32 tensor of at least n entries")
        key_bits = 64 * key_words if key_bits is None else int(key_bits)
        h = C.c_void_p()
        build = self._lib.bl_table_build_u128 if key_words == 2 else self._lib.bl_table_build_u64
        check(build(self._h, C.c_void_p(keys.data_ptr()), _ptr(counts), n, key_bits, C.byref(h)))
        return CountTable(self, h)

    def probe_hbm(self, n_bytes=8 << 30, iters=5):
        """(read GB/s, copy GB/s) sustained by this device: read-only stream kernel and DtoD copy"""
        r, c = C.c_double(), C.c_double()
        check(self._lib.bl_probe_hbm(self._h, int(n_bytes), int(iters), C.byref(r), C.byref(c)))
        return r.value, c.value

    def bgzf_inflate(self, data):
        """inflate a buffer of whole BGZF members on the device (bl_bgzf_walk + bl_bgzf_inflate): (text as a numpy uint8 array,
        per-member status codes — 0 = sound)"""
        data = bytes(data)
        cap = len(data) // 26 + 1
        members = np.zeros(cap * 4, np.uint64)  # 32 bytes per member
        n, used, text = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(self._lib.bl_bgzf_walk(data, len(data), 0, 0, members.ctypes.data, cap, C.byref(n), C.byref(used), C.byref(text)))
        if used.value != len(data):
            raise BiolibError(capi.BL_ERR_INVALID, "the buffer ends inside a BGZF member")
        n, text = n.value, text.value
        ptrs = []
        try:
            for size in (len(data) + 8, 32 * max(n, 1), text + 16, 4 * max(n, 1)):
                p = C.c_void_p()
                check(self._lib.bl_device_alloc(self._h, size, C.byref(p)))
                ptrs.append(p)
            d_packed, d_members, d_text, d_status = ptrs
            check(self._lib.bl_copy_to_device(self._h, d_packed, data, len(data)))
            if n:
                check(self._lib.bl_copy_to_device(self._h, d_members, members.ctypes.data, 32 * n))
            check(self._lib.bl_bgzf_inflate(self._h, d_packed, len(data), d_members, n, d_text, text, d_status))
            self.sync()
            out = np.zeros(text, np.uint8)
            st = np.zeros(max(n, 1), np.uint32)
            if text:
                check(self._lib.bl_copy_to_host(self._h, out.ctypes.data, d_text, text))
            if n:
                check(self._lib.bl_copy_to_host(self._h, st.ctypes.data, d_status, 4 * n))
            return out, st[:n]
        finally:
            for p in ptrs:
                self._lib.bl_device_free(self._h, p)

    def bgzf_deflate_raw(self, text_ptr, n_bytes, flags, out, capacity, members=None):
        """bl_bgzf_deflate: `text_ptr` a device address (or None), `out` a uint8 device tensor (or None) of `capacity` bytes, `members` an
        int64 device tensor of 4 words per member (or None).  Returns (n_out_bytes, n_members); the library checks every argument."""
        nb, nm = C.c_uint64(), C.c_uint64()
        check(self._lib.bl_bgzf_deflate(self._h, text_ptr, int(n_bytes), int(flags), _ptr(out), int(capacity), C.byref(nb), _ptr(members), C.byref(nm)))
        return int(nb.value), int(nm.value)

    def bgzf_deflate(self, text, eof=True, members=False):
        """`text` (bytes or a uint8 device tensor) as BGZF made on the device (bl_bgzf_deflate): a uint8 device tensor holding members of at
        most 65,280 bytes of text each, one deflate block a member, and the EOF marker unless eof=False.  members=True: also the member
        table, an int64 device tensor [n_members, 4] (the 32-byte rows of bl_bgzf_member: what bl_bgzf_inflate takes)."""
        import torch

        if not isinstance(text, torch.Tensor):
            data = bytes(text)
            text = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(self.torch_device) if data else torch.empty(0, dtype=torch.uint8, device=self.torch_device)
        if not (text.is_cuda and text.dtype == torch.uint8 and text.is_contiguous()):
            raise ValueError("text: bytes or a contiguous uint8 device tensor")
        n, flags = int(text.numel()), 0 if eof else capi.BGZF_NO_EOF
        bound = int(self._lib.bl_bgzf_bound(n, flags))
        out = torch.empty(max(bound, 16), dtype=torch.uint8, device=self.torch_device)
        table = torch.zeros((max((n + 65279) // 65280, 1), 4), dtype=torch.int64, device=self.torch_device) if members else None
        self._inputs_ready()
        n_out, n_members = self.bgzf_deflate_raw(_ptr(text) if n else None, n, flags, out, bound, table)
        return (out[:n_out], table[:n_members]) if members else out[:n_out]

    def _write_text(self, text, path, append, compress, eof):
        """a uint8 device tensor to a file: bl_text_write, or bl_text_write_bgzf.  Returns the bytes written: the text's, or with compress
        the bytes the file grew by (the C call reports no count) — 0 for a target that is no regular file, such as /dev/null."""
        import os

        path = str(path)
        p, n = (_ptr(text) if text.numel() else None), int(text.numel())
        if not compress:
            check(self._lib.bl_text_write(self._h, p, n, path.encode(), 1 if append else 0))
            return n
        before = os.path.getsize(path) if append and os.path.exists(path) else 0
        check(self._lib.bl_text_write_bgzf(self._h, p, n, path.encode(), 1 if append else 0, 0 if eof else capi.BGZF_NO_EOF))
        return os.path.getsize(path) - before

    def clock_probe_start(self, duration_ms):
        """start measuring the shader clock the chip holds over the next duration_ms (beside whatever else runs)"""
        h = C.c_void_p()
        check(self._lib.bl_clock_probe_start(self._h, int(duration_ms), C.byref(h)))
        return h

    def clock_probe_finish(self, probe):
        ghz = C.c_double()
        check(self._lib.bl_clock_probe_finish(probe, C.byref(ghz)))
        return float(ghz.value)

    # ---- device arrays (torch plumbing)
    def empty_u64(self, n):
        return self._empty_words(n, 1)

    def empty_u128(self, n):
        return self._empty_words(n, 2)

    def empty_u8(self, n):
        import torch

        return torch.empty(max(int(n), 1), dtype=torch.uint8, device=self.torch_device)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _host_u64(t, n):
    return t[:n].cpu().numpy().view(np.uint64).copy()


class _DeviceArray:
    """carrier of a __cuda_array_interface__ description (torch.as_tensor reads it without copying)"""


def _device_view(ctx, ptr, shape, typestr):
    """a tensor over library-owned device memory (no copy): valid while its owner is open"""
    import torch

    holder = _DeviceArray()
    holder.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)
    return torch.as_tensor(holder, device=ctx.torch_device)


class TextIndex:
    """The names and qualities of a parsed text on the device (bl_text_index): what from_text_indexed and
    Reader.device_batches(indexed=True) return beside the batch.  Close it (or its context) when done; it must outlive every
    format that reads it."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self._h = handle
        self._lib = ctx._lib
        n, fq, t, nb, r = C.c_uint64(), C.c_int(), C.c_void_p(), C.c_uint64(), C.c_void_p()
        check(self._lib.bl_text_index_info(handle, C.byref(n), C.byref(fq), C.byref(t), C.byref(nb), C.byref(r)))
        self.n_records, self.is_fastq, self.n_bytes = int(n.value), bool(fq.value), int(nb.value)
        self._d_text, self._d_records = t.value, r.value
        ctx._tables.add(self)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):
                self._lib.bl_text_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def offsets(self):
        """int64 device tensor [n_records + 1]: the offsets of the batch the index was built with, a view of the index's array"""
        return _device_view(self.ctx, self._lib.bl_text_index_offsets(self._h), (self.n_records + 1,), "<i8")

    def text(self):
        """the indexed text, downloaded"""
        if not self.n_bytes:
            return b""
        self.ctx.sync()
        return _device_view(self.ctx, self._d_text, (self.n_bytes,), "|u1").cpu().numpy().tobytes()

    def records(self):
        """the 16-byte records, downloaded: a numpy structured array (capi.TEXT_RECORD_DTYPE)"""
        if not self.n_records:
            return np.zeros(0, dtype=capi.TEXT_RECORD_DTYPE)
        self.ctx.sync()
        return _device_view(self.ctx, self._d_records, (self.n_records, 2), "<i8").cpu().numpy().view(capi.TEXT_RECORD_DTYPE).reshape(-1).copy()

    def names(self):
        """a host list of the names (bytes: the header lines without marker and terminator) — for tests; the writer never needs it"""
        text = self.text()
        return [text[int(r["name_begin"]):int(r["name_begin"]) + int(r["name_len"])] for r in self.records()]


def _indexed_batch(ctx, h, ix):
    """(Batch, TextIndex) of the two handles bl_text_index_build returns: the batch gets a device copy of the index's offsets"""
    index = TextIndex(ctx, ix)
    b = Batch(ctx, h)
    d_offsets = index.offsets.clone()
    n, total = b.n_seqs, b.n_bases
    if n > 1 and total and total % n == 0 and bool((d_offsets[1:] - d_offsets[:-1] == total // n).all()):
        b.read_len = total // n  # the library's rule: more than one sequence, all equally long
    b._d_offsets = d_offsets
    b._offsets_from_device = True
    return b, index


class CountTable:
    """Sorted distinct keys with 32-bit counts and a prefix index on the device (bl_table).  Close it (or its context) when done; it
    must outlive every asynchronous kmer_counts that reads it."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self._h = handle
        self._lib = ctx._lib
        n, kw, kb, pb = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(self._lib.bl_table_info(handle, C.byref(n), C.byref(kw), C.byref(kb), C.byref(pb)))
        self.n_distinct, self.key_words, self.key_bits, self.prefix_bits = int(n.value), int(kw.value), int(kb.value), int(pb.value)
        ctx._tables.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bl_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _arrays(self):
        k, c = C.c_void_p(), C.c_void_p()
        check(self._lib.bl_table_arrays(self._h, C.byref(k), C.byref(c)))
        return k.value, c.value

    def _view(self, ptr, shape, dtype):
        """a tensor over the table's own memory (no copy): valid while the table is open"""
        import torch

        if self.n_distinct == 0:
            return torch.empty(shape, dtype=dtype, device=self.ctx.torch_device)
        holder = _DeviceArray()
        holder.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<i8" if dtype == torch.int64 else "<i4", data=(int(ptr), False), version=2,
                                               strides=None)
        return torch.as_tensor(holder, device=self.ctx.torch_device)

    @property
    def keys(self):
        """the sorted distinct keys: int64[n_distinct] or int64[n_distinct, 2] (low, high), a view of the table's array"""
        import torch

        shape = (self.n_distinct, 2) if self.key_words == 2 else (self.n_distinct,)
        return self._view(self._arrays()[0], shape, torch.int64)

    @property
    def counts(self):
        """int32[n_distinct] holding the uint32 counts, a view of the table's array"""
        import torch

        return self._view(self._arrays()[1], (self.n_distinct,), torch.int32)

    def lookup(self, keys, n=None):
        """int32 tensor (uint32 bits) of the stored count of every key of keys[:n], 0 for a key that is not in the table"""
        import torch

        c = self.ctx
        if self.key_words == 2:
            n = c._keys128(keys, n)
        else:
            if keys.dim() != 1 or keys.element_size() != 8 or not keys.is_contiguous():
                raise ValueError("one-word keys are a contiguous int64[n] tensor")
            n = keys.numel() if n is None else int(n)
            c._inputs_ready()
        out = torch.empty(max(n, 1), dtype=torch.int32, device=c.torch_device)
        call = self._lib.bl_table_lookup_u128 if self.key_words == 2 else self._lib.bl_table_lookup_u64
        check(call(c._h, self._h, C.c_void_p(keys.data_ptr()), n, C.c_void_p(out.data_ptr())))
        return out[:n]

    def histogram(self, n_bins):
        """numpy uint64[n_bins]: hist[c] = distinct keys with count c, the last bin those with count >= n_bins - 1"""
        hist = np.zeros(max(int(n_bins), 1), np.uint64)
        check(self._lib.bl_table_histogram(self.ctx._h, self._h, hist.ctypes.data_as(C.c_void_p), int(n_bins)))
        return hist

    # ---- table algebra (bl_table_combine): one merge of the two sorted tables, no rebuild
    _COUNT_MODES = dict(sum=capi.COUNT_SUM, min=capi.COUNT_MIN, max=capi.COUNT_MAX, left=capi.COUNT_LEFT, right=capi.COUNT_RIGHT)

    def combine_raw(self, other, op, mode, min_count=0, max_count=2**32 - 1, table=True):
        """bl_table_combine: (CountTable or None, stats dict); other None: the empty table.  The library checks op, mode and bounds."""
        if not 0 <= int(min_count) < 2**32 or not 0 <= int(max_count) < 2**32:
            raise ValueError("count bounds are 32-bit unsigned")
        h, st = C.c_void_p(), capi.TableStats()
        check(self._lib.bl_table_combine(self.ctx._h, self._h, other._h if other is not None else None, int(op), int(mode), int(min_count),
                                         int(max_count), C.byref(h) if table else None, C.byref(st)))
        return (CountTable(self.ctx, h) if table else None), st.as_dict()

    def _combine(self, other, op, count, min_count, max_count):
        if count not in self._COUNT_MODES:
            raise ValueError(f"count is one of {sorted(self._COUNT_MODES)}")
        return self.combine_raw(other, op, self._COUNT_MODES[count], min_count, max_count)[0]

    def union(self, other, count="sum", min_count=0, max_count=2**32 - 1):
        """The keys of either table; where both hold a key its count is count(a, b): "sum" (saturating at 2^32 - 1), "min", "max", "left"
        (this table's) or "right".  Then only the keys with min_count <= count <= max_count are kept.  A new CountTable; the inputs stay."""
        return self._combine(other, capi.TABLE_UNION, count, min_count, max_count)

    def intersect(self, other, count="min", min_count=0, max_count=2**32 - 1):
        """The keys of both tables with count(a, b), bounded as in union"""
        return self._combine(other, capi.TABLE_INTERSECT, count, min_count, max_count)

    def subtract(self, other, min_count=0, max_count=2**32 - 1):
        """The keys of this table that `other` lacks, with their counts, bounded as in union"""
        return self._combine(other, capi.TABLE_SUBTRACT, "left", min_count, max_count)

    def subtract_counts(self, other, min_count=0, max_count=2**32 - 1):
        """Every key of this table whose count a exceeds its count b in `other` (0 where absent), with a - b, bounded as in union"""
        return self._combine(other, capi.TABLE_COUNT_SUBTRACT, "left", min_count, max_count)

    def filter(self, min_count=0, max_count=2**32 - 1):
        """The keys with min_count <= count <= max_count: filter(2) is the table of the solid k-mers"""
        if not 0 <= int(min_count) < 2**32 or not 0 <= int(max_count) < 2**32:
            raise ValueError("count bounds are 32-bit unsigned")
        h = C.c_void_p()
        check(self._lib.bl_table_filter(self.ctx._h, self._h, int(min_count), int(max_count), C.byref(h)))
        return CountTable(self.ctx, h)

    def compare(self, other):
        """The statistics of the pair without building a table: n_a_only, n_b_only, n_both, sum_min, sum_max (and n_out, sum_out of the
        plain sum union), plus jaccard = n_both / |A u B| and weighted_jaccard = sum_min / sum_max (0.0 where the denominator is 0)"""
        st = self.combine_raw(other, capi.TABLE_UNION, capi.COUNT_SUM, table=False)[1]
        union = st["n_a_only"] + st["n_b_only"] + st["n_both"]
        st["jaccard"] = st["n_both"] / union if union else 0.0
        st["weighted_jaccard"] = st["sum_min"] / st["sum_max"] if st["sum_max"] else 0.0
        return st

    # ---- the graph on the keys (bl_table_adjacency, bl_table_unitigs): a table of canonical k-mers, k odd, is a de Bruijn graph
    def adjacency_raw(self, k, mask, links=None, stats=None):
        """bl_table_adjacency: `mask` takes n_distinct bytes, `links` (or None) 2 * n_distinct 32-bit words, `stats` (or None) is a
        capi.GraphStats.  Synchronous; the library checks k and the table."""
        check(self._lib.bl_table_adjacency(self.ctx._h, self._h, int(k), _ptr(mask), _ptr(links), C.byref(stats) if stats is not None else None))

    def adjacency(self, k, links=False):
        """The neighbours of every key in the bidirected de Bruijn graph of this table of canonical k-mers (k odd, at most 63):
        (mask, links, stats).  mask: a uint8 device tensor, one byte per key in key order; bit c (A C G T = 0..3) is set where the k-mer
        with base c appended has its canonical form in the table, bit 4 + c where the one with base c prepended has.  links (None
        without links=True): an int32 device tensor [n_distinct, 2] holding uint32 words, column 0 the key's left side and column 1
        its right side: (j << 1) | t where the side has exactly one neighbour, another key j, whose side t (0 left, 1 right) has
        exactly one too; -1 (BL_LINK_NONE) otherwise.  stats: n_keys, n_arcs, n_isolated, n_dead_end_sides, n_branch_sides,
        n_linked_sides.  Filter the table first (filter(2)) to build the graph of the solid k-mers."""
        import torch

        n, dev = self.n_distinct, self.ctx.torch_device
        mask = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        d_links = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev) if links else None
        st = capi.GraphStats()
        self.ctx._inputs_ready()
        self.adjacency_raw(k, mask, d_links, st)
        stats = {name: value for name, value in st.as_dict().items() if name in ("n_keys", "n_arcs", "n_isolated", "n_dead_end_sides", "n_branch_sides", "n_linked_sides")}
        return mask[:n], (d_links[:n] if links else None), stats

    def unitigs_raw(self, k, batch=True, offsets=None, count_sums=None, nodes=None, stats=None):
        """bl_table_unitigs: `offsets` / `count_sums` / `nodes` (or None) take n_distinct + 1 / n_distinct 64-bit words and n_distinct
        8-byte records.  Returns (handle or None, n_unitigs, n_bases).  Synchronous; the library checks k and the table."""
        h, nu, nb = C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(self._lib.bl_table_unitigs(self.ctx._h, self._h, int(k), C.byref(h) if batch else None, _ptr(offsets), _ptr(count_sums), _ptr(nodes),
                                         C.byref(nu), C.byref(nb), C.byref(stats) if stats is not None else None))
        return (h if batch else None), int(nu.value), int(nb.value)

    def unitig_links_raw(self, k, nodes, offsets, n_unitigs, flags=0, link_offsets=None, links=None, capacity=0, stats=None):
        """bl_unitig_links: `nodes` / `offsets` are what unitigs_raw filled for this table and k, `link_offsets` (or None) takes
        2 * n_unitigs + 1 64-bit words, `links` (None: sizing only) `capacity` 8-byte records, `stats` (or None) is a capi.LinkStats.
        Returns n_links.  Synchronous; the library checks every argument."""
        nl = C.c_uint64()
        check(self._lib.bl_unitig_links(self.ctx._h, self._h, int(k), _ptr(nodes), _ptr(offsets), int(n_unitigs), int(flags), _ptr(link_offsets), _ptr(links),
                                        int(capacity), C.byref(nl), C.byref(stats) if stats is not None else None))
        return int(nl.value)

    def unitigs(self, k, nodes=False, batch=True, links=False, once=False):
        """The unitigs of this table of canonical k-mers (k odd, at most 63): its non-branching paths and cycles compacted on the device,
        every key in exactly one (bl_table_unitigs; the header states the start and orientation rules).  Returns a Unitigs:
        .batch       a device-resident Batch of the unitig strings (L + k - 1 uppercase bases for L keys), numbered by the slot of their
                     start key; it keeps its offsets on the device like the result of select, so kmers, minimizers, kmer_counts,
                     read_counts run on it as they are: the canonical k-mers of the batch are the table's keys, each exactly once
                     (None with batch=False: labels only)
        .offsets     int64 device tensor [n_unitigs + 1]
        .count_sums  int64 device tensor [n_unitigs]: the sum of the unitig's keys' counts; over its number of keys
                     (length - k + 1) BCALM's mean abundance
        .nodes       with nodes=True an int32 device tensor [n_distinct, 2] (uint32 words): the unitig of every key and
                     (rank << 1) | flip — its place counted from the start key, and whether it is read reverse-complemented
        .stats       n_unitigs, n_cycles and longest_unitig (in keys) besides the six of adjacency
        With links=True (k >= 3; bl_unitig_links, the header states the definitions) also the edges between unitig ends:
        .link_offsets  int64 device tensor [2 * n_unitigs + 1]: end e = (unitig << 1) | orientation (0 for +, 1 for -) has the records
                       link_offsets[e] .. link_offsets[e + 1]
        .links         int32 device tensor [n_links, 2] (uint32 words): (from, to), both ends as numbered above — the last k - 1 bases of
                       unitig from >> 1 read in orientation from & 1 are the first k - 1 of unitig to >> 1 read in orientation to & 1.
                       once=True keeps one record of each reverse pair (from <= to ^ 1)
        .link_stats    n_ends, n_links, n_self_reverse, n_dead_ends, n_branch_ends
        Filter the table first (filter(2)) to compact the graph of the solid k-mers."""
        import torch

        n, dev = self.n_distinct, self.ctx.torch_device
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        sums = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        d_nodes = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev) if nodes or links else None
        st = capi.GraphStats()
        self.ctx._inputs_ready()
        h, n_unitigs, n_bases = self.unitigs_raw(k, batch, offsets, sums, d_nodes, st)
        d_out = offsets[:n_unitigs + 1]
        b = None
        if batch:
            fixed = 0  # the library's rule: more than one sequence, all equally long
            if n_unitigs > 1 and n_bases % n_unitigs == 0 and bool((d_out[1:] - d_out[:-1] == n_bases // n_unitigs).all()):
                fixed = n_bases // n_unitigs
            b = Batch(self.ctx, h, read_len=fixed)
            b._d_offsets = d_out
            b._offsets_from_device = True
        u = Unitigs(b, d_out, sums[:n_unitigs], d_nodes[:n] if nodes else None, st.as_dict(), n_unitigs, n_bases)
        u.k, u._ctx, u._lib = int(k), self.ctx, self._lib
        u._table = self  # read_steps looks the reads' k-mers up in the table the unitigs came from
        if d_nodes is not None:
            u._nodes = d_nodes[:n]
        if links:
            # the header's identity gives the record count before the call: one search pass, no sizing call
            bound = int(st.n_arcs) - int(st.n_linked_sides) + 2 * int(st.n_cycles)
            link_offsets = torch.empty(2 * n_unitigs + 1, dtype=torch.int64, device=dev)
            d_links = torch.empty((max(bound, 1), 2), dtype=torch.int32, device=dev)
            ls = capi.LinkStats()
            n_links = self.unitig_links_raw(k, d_nodes, d_out, n_unitigs, capi.LINKS_ONCE if once else 0, link_offsets, d_links, bound, ls)
            u.link_offsets, u.links, u.link_stats = link_offsets, d_links[:n_links], ls.as_dict()
            u._nodes, u._once = d_nodes[:n], bool(once)
        return u

    # ---- cleaning the graph (bl_unitigs_mark, bl_table_remove_unitigs): the marked unitigs' keys leave, an ordinary table remains
    def remove_unitigs_raw(self, nodes, marks, n_unitigs):
        """bl_table_remove_unitigs: `nodes` are what unitigs_raw filled for this table, `marks` one byte per unitig.  Returns
        (handle, n_removed).  Synchronous; the library checks every argument."""
        h, nr = C.c_void_p(), C.c_uint64()
        check(self._lib.bl_table_remove_unitigs(self.ctx._h, self._h, _ptr(nodes), _ptr(marks), int(n_unitigs), C.byref(h), C.byref(nr)))
        return h, int(nr.value)

    def remove_unitigs(self, unitigs, marks):
        """This table without the keys of the unitigs whose mark is not 0: a new CountTable, the kept keys in order with their counts.
        `unitigs` is what unitigs(k, nodes=True) or unitigs(k, links=True) returned for THIS table, `marks` a uint8 device tensor
        [n_unitigs] (Unitigs.mark's, or any selection of your own).  ValueError where the nodes are not one per key of this table or
        the marks not on its device: the kernels read one node per key and cannot tell."""
        nodes = unitigs.nodes if unitigs.nodes is not None else unitigs._nodes
        if nodes is None:
            raise ValueError("remove_unitigs needs the nodes: unitigs(k, nodes=True) or unitigs(k, links=True)")
        if int(nodes.shape[0]) != self.n_distinct:  # the library cannot know the length: the kernels read one node per key
            raise ValueError("these unitigs are of another table: %d nodes for %d keys" % (int(nodes.shape[0]), self.n_distinct))
        if marks.element_size() != 1 or marks.numel() != unitigs.n_unitigs or not marks.is_contiguous():
            raise ValueError("marks is a contiguous one-byte tensor with one element per unitig")
        if marks.device != nodes.device:
            raise ValueError("marks is a device tensor on the table's device (%s), not on %s" % (nodes.device, marks.device))
        self.ctx._inputs_ready()
        return CountTable(self.ctx, self.remove_unitigs_raw(nodes if self.n_distinct else None, marks if self.n_distinct else None, unitigs.n_unitigs)[0])

    def clean(self, k, tips=None, isolated=None, isolated_mean=2**32 - 1, bubbles=None, bubble_diff=0, max_rounds=8):
        """The table of the cleaned graph: rounds of unitigs(k, batch=False, links=True) -> mark -> remove_unitigs until a round marks
        nothing or max_rounds have run.  tips / isolated / bubbles are the greatest numbers of keys of a tip, an island and a bubble
        branch that go (each 2 * k where not given, False switches the rule off; see Unitigs.mark).  Returns (table, history): a new
        CountTable (this one stays) and the stats of every round, the last round that marked nothing included.  Then unitigs(k) of
        the result gives the contigs."""
        tips, isolated, bubbles = (2 * int(k) if x is None else None if x is False else x for x in (tips, isolated, bubbles))
        table, history, done = self, [], False
        try:
            for _ in range(int(max_rounds)):
                u = table.unitigs(k, batch=False, links=True)
                marks, stats = u.mark(tips=tips, isolated=isolated, isolated_mean=isolated_mean, bubbles=bubbles, bubble_diff=bubble_diff)
                history.append(stats)
                if not (stats["n_tips"] or stats["n_isolated"] or stats["n_bubbles"]):
                    break
                cleaner = table.remove_unitigs(u, marks)
                if table is not self:
                    table.close()
                table = cleaner
            if table is self:  # nothing went: still a table of the caller's own to close
                table = self.filter()
            done = True
            return table, history
        finally:
            if not done and table is not self:  # a round raised: the table of the rounds before it is nobody's
                table.close()


class Unitigs:
    """What CountTable.unitigs returns: batch, offsets, count_sums, nodes, stats (and n_unitigs, n_bases); with links=True also
    link_offsets, links and link_stats."""

    def __init__(self, batch, offsets, count_sums, nodes, stats, n_unitigs, n_bases):
        self.batch, self.offsets, self.count_sums, self.nodes, self.stats = batch, offsets, count_sums, nodes, stats
        self.n_unitigs, self.n_bases = n_unitigs, n_bases
        self.link_offsets = self.links = self.link_stats = None
        self.k, self._ctx, self._lib = None, None, None
        self._nodes, self._once, self._table = None, False, None

    def mark_raw(self, rule, marks, stats=None):
        """bl_unitigs_mark: `rule` a capi.CleanRule, `marks` a one-byte device tensor of n_unitigs elements, `stats` (or None) a
        capi.CleanStats.  Synchronous; the library checks every argument."""
        n_links = int(self.links.shape[0]) if self.links is not None else 0
        check(self._lib.bl_unitigs_mark(self._ctx._h, _ptr(self.offsets), _ptr(self.count_sums), int(self.n_unitigs), _ptr(self.link_offsets),
                                        _ptr(self.links) if n_links else None, n_links, C.byref(rule), _ptr(marks), C.byref(stats) if stats is not None else None))

    def mark(self, tips=None, isolated=None, isolated_mean=None, bubbles=None, bubble_diff=0):
        """Which unitigs a cleaning round removes (bl_unitigs_mark; the header states the rules): (marks, stats).  marks: a uint8 device
        tensor [n_unitigs], 0 keep, 1 tip (a dead-end spur of at most `tips` keys beside a real continuation or a better spur), 2
        isolated (no link at either end, at most `isolated` keys, mean abundance at most `isolated_mean`), 3 bubble (at most `bubbles`
        keys, between the same two anchors as a branch with a greater mean whose length differs by at most `bubble_diff`).  None
        switches a rule off (isolated_mean None: no bound).  stats: n_unitigs, n_tips, n_isolated, n_bubbles, n_keys_marked,
        count_sum_marked.  Needs unitigs(k, links=True) with once=False: the rules read every end's records."""
        import torch

        if self.links is None or self._once:
            raise ValueError("mark needs unitigs(k, links=True, once=False): every end's records")
        rule = capi.CleanRule()
        rule.flags = (capi.CLEAN_TIPS if tips is not None else 0) | (capi.CLEAN_ISOLATED if isolated is not None else 0) | (capi.CLEAN_BUBBLES if bubbles is not None else 0)
        rule.k = self.k
        rule.max_tip_keys, rule.max_isolated_keys, rule.max_bubble_keys = int(tips or 0), int(isolated or 0), int(bubbles or 0)
        rule.max_isolated_mean = 2**64 - 1 if isolated_mean is None else int(isolated_mean)
        rule.max_bubble_diff = int(bubble_diff)
        marks = torch.empty(max(self.n_unitigs, 1), dtype=torch.uint8, device=self._ctx.torch_device)
        st = capi.CleanStats()
        self._ctx._inputs_ready()
        self.mark_raw(rule, marks, st)
        return marks[:self.n_unitigs], st.as_dict()

    def write_fasta(self, path, line_width=0, compress=False):
        """The unitigs as a FASTA file made on the device (Batch.write): names 0, 1, ... with " LN:i:<bases> KC:i:<count sum>" — BCALM's
        header without its km and L fields (no floats; the links between unitigs leave through write_gfa).  compress=True: as BGZF.
        Returns the bytes written."""
        if self.batch is None:
            raise ValueError("unitigs(batch=False) holds no strings to write")
        return self.batch.write(path, compress=compress, fmt="fasta", tags=self.count_sums if self.n_unitigs else None, tag_label="KC:i:", tag_length=True,
                                line_width=line_width)

    def format_gfa_raw(self, rule, out=None, capacity=0):
        """bl_unitigs_format_gfa: `rule` a capi.GfaRule, `out` a uint8 device tensor (None: sizing only) of `capacity` bytes.  Synchronous.
        Returns n_bytes; the library checks every argument."""
        nb = C.c_uint64()
        n_links = int(self.links.shape[0]) if self.links is not None else 0
        check(self._lib.bl_unitigs_format_gfa(self._ctx._h, self.batch._h, _ptr(self.offsets), int(self.n_unitigs), _ptr(self.count_sums) if self.n_unitigs else None,
                                              _ptr(self.links) if n_links else None, n_links, C.byref(rule), _ptr(out), int(capacity), C.byref(nb)))
        return int(nb.value)

    def format_gfa(self, prefix="", first_number=0, header=True):
        """The unitigs and their links as GFA 1 text made on the device (bl_unitigs_format_gfa): a uint8 device tensor.  One H line
        (header=False: none), one S line per unitig — name prefix + decimal(first_number + u), the bases, LN:i: and KC:i: (the count
        sum) — and one L line per link record with the overlap (k - 1)M.  Needs unitigs(k, links=True); once=True writes every edge
        once."""
        import torch

        if self.batch is None:
            raise ValueError("unitigs(batch=False) holds no strings to write")
        if self.links is None:
            raise ValueError("unitigs(links=False) holds no links to write")
        rule = capi.GfaRule()
        rule.flags = 0 if header else capi.GFA_NO_HEADER
        rule.k = self.k
        rule.name_prefix = prefix.encode("latin1") if isinstance(prefix, str) else bytes(prefix)  # (16 bytes without a NUL reach the library, which refuses them)
        rule.first_number = int(first_number) & (2**64 - 1)
        self._ctx._inputs_ready()
        n_bytes = self.format_gfa_raw(rule)
        out = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=self._ctx.torch_device)
        self.format_gfa_raw(rule, out, n_bytes)
        return out[:n_bytes]

    def write_gfa(self, path, prefix="", first_number=0, header=True, compress=False):
        """format_gfa(...) written to `path` (bl_text_write, as Batch.write; compress=True: as BGZF, bl_text_write_bgzf).  Returns the
        bytes written."""
        return self._ctx._write_text(self.format_gfa(prefix, first_number, header), path, False, compress, True)


class ReadSteps:
    """What Batch.read_steps returns: `steps`, an int64 device tensor [n_steps, 4] holding the 32-byte bl_read_step records in ascending
    position (host() turns it into a numpy record array: pos, seq, end, offset, n_kmers, flags), and `stats` (n_valid, n_found, n_steps,
    n_chains, n_linked, longest_step).  It keeps the batch and the unitigs the steps refer to."""

    def __init__(self, batch, unitigs, steps, stats, d_offsets):
        self.batch, self.unitigs, self.steps, self.stats = batch, unitigs, steps, stats
        self.n_steps = int(steps.shape[0])
        self._d_offsets = d_offsets
        self._ctx, self._lib = batch.ctx, batch._lib

    def host(self):
        """a numpy record array of the steps (capi.READ_STEP_DTYPE)"""
        return self.steps.cpu().numpy().view(np.uint8).reshape(-1, 32).copy().view(capi.READ_STEP_DTYPE).reshape(-1)

    def link_support_raw(self, link_offsets, links, n_links, n_unitigs, support, stats=None):
        """bl_link_support: `support` takes n_links uint32 words, `stats` (or None) is a capi.SupportStats.  Synchronous; the library checks
        every argument."""
        check(self._lib.bl_link_support(self._ctx._h, _ptr(self.steps) if self.n_steps else None, self.n_steps, _ptr(link_offsets), _ptr(links) if n_links else None,
                                        int(n_links), int(n_unitigs), _ptr(support) if n_links else None, C.byref(stats) if stats is not None else None))

    def link_support(self, unitigs=None):
        """How many reads crossed every link record (bl_link_support): (support, stats).  support is an int32 device tensor [n_links]
        holding uint32 counts, in the order of unitigs.links: a read's transition a -> b counts on the record a -> b and on its reverse
        b^1 -> a^1 where the array holds them, a self-reverse record once.  stats: n_transitions, n_unmatched (transitions that found no
        record).  `unitigs` (default: the ones the steps were made with) needs unitigs(k, links=True), with either value of once."""
        import torch

        u = unitigs if unitigs is not None else self.unitigs
        if u.links is None:
            raise ValueError("link_support needs unitigs(k, links=True)")
        n_links = int(u.links.shape[0])
        support = torch.empty(max(n_links, 1), dtype=torch.int32, device=self._ctx.torch_device)
        st = capi.SupportStats()
        self._ctx._inputs_ready()
        self.link_support_raw(u.link_offsets, u.links, n_links, u.n_unitigs, support, st)
        return support[:n_links], st.as_dict()

    def format_gaf_raw(self, rule, out=None, capacity=0):
        """bl_steps_format_gaf: `rule` a capi.GafRule, `out` a uint8 device tensor (None: sizing only) of `capacity` bytes.  Synchronous.
        Returns n_bytes; the library checks every argument."""
        nb = C.c_uint64()
        u = self.unitigs
        check(self._lib.bl_steps_format_gaf(self._ctx._h, self.batch._h, _ptr(self._d_offsets), _ptr(self.steps) if self.n_steps else None, self.n_steps,
                                            _ptr(u.offsets), int(u.n_unitigs), C.byref(rule), _ptr(out), int(capacity), C.byref(nb)))
        return int(nb.value)

    def format_gaf(self, read_prefix="read", read_first_number=0, segment_prefix="", segment_first_number=0):
        """The walks as GAF text made on the device (bl_steps_format_gaf): a uint8 device tensor, one line per chain of steps the read
        made through link records.  Reads are named read_prefix + decimal(read_first_number + sequence index) (real read names are not
        built), segments segment_prefix + decimal(segment_first_number + unitig): the names Unitigs.format_gfa prints for the same
        prefix and first_number."""
        import torch

        rule = capi.GafRule()
        rule.flags, rule.k = 0, self.unitigs.k
        rule.read_prefix = read_prefix.encode("latin1") if isinstance(read_prefix, str) else bytes(read_prefix)
        rule.segment_prefix = segment_prefix.encode("latin1") if isinstance(segment_prefix, str) else bytes(segment_prefix)
        rule.read_first_number = int(read_first_number) & (2**64 - 1)
        rule.segment_first_number = int(segment_first_number) & (2**64 - 1)
        self._ctx._inputs_ready()
        n_bytes = self.format_gaf_raw(rule)
        out = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=self._ctx.torch_device)
        self.format_gaf_raw(rule, out, n_bytes)
        return out[:n_bytes]

    def write_gaf(self, path, compress=False, **names):
        """format_gaf(**names) written to `path` (bl_text_write; compress=True: as BGZF, bl_text_write_bgzf).  Returns the bytes written."""
        return self._ctx._write_text(self.format_gaf(**names), path, False, compress, True)


class ReadCounts:
    """The records of bl_scan_read_counts, one per sequence: `records` is the raw device buffer, int64[n_seqs, 6]; the fields are views
    of it (no copy).  The 32-bit fields are int32 tensors holding uint32 bits, the 64-bit ones int64 holding uint64 bits: min_count is
    -1 (0xFFFFFFFF) and weak_begin -1 (UINT64_MAX) where the sequence has no k-mer / no weak k-mer."""

    def __init__(self, ctx, n_seqs):
        import torch

        self.n_seqs = int(n_seqs)
        self.records = torch.zeros((max(self.n_seqs, 1), 6), dtype=torch.int64, device=ctx.torch_device)  # (torch allocations are 16-byte aligned)
        words = self.records.view(torch.int32)  # [n_seqs, 12]
        words[:, 3] = -1      # min_count: the identity record
        self.records[:, 4] = -1  # weak_begin
        n = self.n_seqs
        self.n_kmers, self.n_found, self.n_solid, self.min_count, self.max_count = (words[:n, i] for i in range(5))
        self.sum_counts, self.weak_begin, self.weak_end = (self.records[:n, i] for i in (3, 4, 5))

    def host(self):
        """a numpy structured array of the records (field names as the attributes, plus `reserved`)"""
        dt = np.dtype([("n_kmers", "<u4"), ("n_found", "<u4"), ("n_solid", "<u4"), ("min_count", "<u4"), ("max_count", "<u4"), ("reserved", "<u4"),
                       ("sum_counts", "<u8"), ("weak_begin", "<u8"), ("weak_end", "<u8")])
        return self.records[:self.n_seqs].cpu().numpy().view(dt).reshape(-1).copy()


class ReadQuality:
    """What bl_scan_read_quality wrote, one row per read: `records` is the raw device buffer, int64[n_seqs, 6] (capi.READ_QUALITY_DTYPE;
    begin and end are the trimmed span before the filters), `spans` an int64 device tensor [n_seqs, 2] for select and format — (0, 0)
    where a filter failed — and `stats` the call's totals as a dict, or None where they were not asked for."""

    def __init__(self, n_seqs, records, spans, stats):
        self.n_seqs = int(n_seqs)
        self.records = records
        self.spans = spans
        self.stats = stats

    def host(self):
        """a numpy structured array of the records (capi.READ_QUALITY_DTYPE)"""
        return self.records[:self.n_seqs].cpu().numpy().view(np.dtype(capi.READ_QUALITY_DTYPE)).reshape(-1).copy()


# the public Illumina adapter sequences, as cutadapt's and fastp's documentation give them: what read-through leaves at a read's 3' end
ADAPTERS = {
    "truseq": "AGATCGGAAGAGC",            # TruSeq and most other Illumina kits, both reads
    "nextera": "CTGTCTCTTATACACATCT",     # Nextera / transposase
    "small_rna": "TGGAATTCTCGGGTGCCAAGG",  # small RNA 3' adapter
}


class ReadAdapters:
    """What bl_scan_read_adapters wrote, one row per read: `records` is the raw device buffer, int64[n_seqs, 4] (capi.READ_ADAPTERS_DTYPE;
    begin and end are the span after the four steps, before min_len), `spans` an int64 device tensor [n_seqs, 2] for intersect_spans,
    select and format — (0, 0) where the result is empty or shorter than min_len — and `stats` the call's totals as a dict, or None
    where they were not asked for."""

    def __init__(self, n_seqs, records, spans, stats):
        self.n_seqs = int(n_seqs)
        self.records = records
        self.spans = spans
        self.stats = stats

    def host(self):
        """a numpy structured array of the records (capi.READ_ADAPTERS_DTYPE)"""
        return self.records[:self.n_seqs].cpu().numpy().view(np.dtype(capi.READ_ADAPTERS_DTYPE)).reshape(-1).copy()


class ReadDuplicates:
    """What bl_scan_read_duplicates wrote: `records` is the raw device buffer, int64[n_units, 2] (capi.READ_DUPLICATE_DTYPE, one row per
    UNIT: a read, or a pair of mates), `spans` an int64 device tensor [n_seqs, 2] for intersect_spans, select and format — (0, 0) for
    the reads of a duplicate — and `stats` the call's totals as a dict, or None where they were not asked for."""

    def __init__(self, n_units, records, spans, stats):
        self.n_units = int(n_units)
        self.records = records
        self.spans = spans
        self.stats = stats

    def host(self):
        """a numpy structured array of the records (capi.READ_DUPLICATE_DTYPE)"""
        return self.records[:self.n_units].cpu().numpy().view(np.dtype(capi.READ_DUPLICATE_DTYPE)).reshape(-1).copy()

    @property
    def kept_mask(self):
        """a bool device tensor [n_units]: the unit is no duplicate (empty units included)"""
        return ((self.records[:self.n_units, 1] >> 32) & capi.DUP_DUPLICATE) == 0  # (a row: first | kept << 32, copies | flags << 32)


class Batch:
    """Device-resident sequences (bl_batch)."""

    def __init__(self, ctx, handle, offsets=None, read_len=0):
        self.ctx = ctx
        self._h = handle
        self._lib = ctx._lib
        self._keep = None
        self._d_offsets = None     # read_counts: the device copy, uploaded once (select: written by the library)
        self._offsets_from_device = False  # select: the host copy is downloaded when it is first asked for
        self.offsets = offsets     # the host offsets the batch was made from (uint64 numpy array), None where it was made without
        self.read_len = read_len   # != 0: made as reads of this length laid end to end
        ctx._batches.add(self)

    @property
    def offsets(self):
        if self._host_offsets is None and self._offsets_from_device:
            self._host_offsets = self._d_offsets.cpu().numpy().view(np.uint64).copy()
        return self._host_offsets

    @offsets.setter
    def offsets(self, value):
        self._host_offsets = value

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):  # a closed context has already destroyed its batches
                self._lib.bl_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_bases(self):
        return int(self._lib.bl_batch_n_bases(self._h))

    @property
    def n_seqs(self):
        return int(self._lib.bl_batch_n_seqs(self._h))

    def set_origin(self, origin):
        """This batch is a piece of a longer concatenation whose base `origin` is the batch's base 0: every position a scan reports
        (and folds into xor_pos) becomes origin + position inside the batch (bl_batch_set_origin; biolib_amd.shard cuts contigs with it)."""
        check(self._lib.bl_batch_set_origin(self._h, int(origin)))
        return self

    def download(self, first=0, n=None):
        n = self.n_bases - first if n is None else n
        out = np.empty(n, dtype=np.uint8)
        check(self._lib.bl_batch_download(self._h, first, n, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- raw (asynchronous) entry points: device tensors in, Result filled after ctx.sync()
    def kmers_raw(self, k, seed, flags, first=0, n=0, values=None, hashes=None, valid=None, result=None):
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_kmers(self.ctx._h, self._h, first, n, k, seed, flags, _ptr(values), _ptr(hashes), _ptr(valid), C.byref(result)))
        return result

    def minimizers_raw(self, unit, w, seed, flags, first=0, n=0, values=None, positions=None, hashes=None, capacity=0, result=None):
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_minimizers(self.ctx._h, self._h, first, n, unit, w, seed, flags, _ptr(values), _ptr(positions), _ptr(hashes),
                                           capacity, C.byref(result)))
        return result

    def hash_sample_raw(self, k, seed, threshold, flags, first=0, n=0, values=None, positions=None, hashes=None, capacity=0, result=None):
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_hash_sample(self.ctx._h, self._h, first, n, k, seed, threshold, flags, _ptr(values), _ptr(positions), _ptr(hashes),
                                            capacity, C.byref(result)))
        return result

    def kmers128_raw(self, k, seed, flags, first=0, n=0, values=None, hashes=None, valid=None, result=None):
        """bl_scan_kmers128 (k <= 64): `values` holds two words per position, low then high"""
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_kmers128(self.ctx._h, self._h, first, n, k, seed, flags, _ptr(values), _ptr(hashes), _ptr(valid), C.byref(result)))
        return result

    def kmer_counts_raw(self, table, k, flags, first=0, n=0, counts=None, valid=None, result=None):
        """bl_scan_kmer_counts: `counts` takes one uint32 per position of the range; the table must stay open until the sync"""
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_kmer_counts(self.ctx._h, self._h, first, n, k, flags, table._h, _ptr(counts), _ptr(valid), C.byref(result)))
        return result

    def read_counts_raw(self, table, k, flags, min_count, records, first=0, n=0, offsets=None, mode=READ_COUNTS_INIT, result=None):
        """bl_scan_read_counts: `records` takes 48 bytes per sequence of the batch (16-byte aligned), `offsets` is the device copy of the
        batch's n_seqs + 1 offsets (None: a single-sequence or fixed-read-length batch); the table must stay open until the sync"""
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_read_counts(self.ctx._h, self._h, first, n, k, flags, table._h, min_count, _ptr(offsets), mode, _ptr(records), C.byref(result)))
        return result

    def hash_sample128_raw(self, k, seed, threshold, flags, first=0, n=0, values=None, positions=None, hashes=None, capacity=0, result=None):
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_hash_sample128(self.ctx._h, self._h, first, n, k, seed, threshold, flags, _ptr(values), _ptr(positions), _ptr(hashes),
                                               capacity, C.byref(result)))
        return result

    def super_kmers_raw(self, k, m, seed, flags, first=0, n=0, minimizers=None, first_pos=None, mm_pos=None, sizes=None, hashes=None,
                        capacity=0, result=None):
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_super_kmers(self.ctx._h, self._h, first, n, k, m, seed, flags, _ptr(minimizers), _ptr(first_pos), _ptr(mm_pos),
                                            _ptr(sizes), _ptr(hashes), capacity, C.byref(result)))
        return result

    def syncmers_raw(self, k, s, soff, eoff, seed, flags, first=0, n=0, positions=None, capacity=0, result=None):
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_syncmers(self.ctx._h, self._h, first, n, k, s, soff, eoff, seed, flags, _ptr(positions), capacity, C.byref(result)))
        return result

    def syncmers128_raw(self, k, s, soff, eoff, seed, flags, first=0, n=0, positions=None, capacity=0, result=None):
        """bl_scan_syncmers128 (s <= 32, s <= k <= 64): s-mers hashed as 16-byte keys"""
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_syncmers128(self.ctx._h, self._h, first, n, k, s, soff, eoff, seed, flags, _ptr(positions), capacity, C.byref(result)))
        return result

    def minimizers128_raw(self, unit, w, seed, flags, first=0, n=0, values=None, positions=None, hashes=None, capacity=0, result=None):
        """bl_scan_minimizers128 (unit <= 64, w <= 64): `values` holds two words per record, low then high"""
        result = result if result is not None else Result()
        self.ctx._hold(result, flags)
        check(self._lib.bl_scan_minimizers128(self.ctx._h, self._h, first, n, unit, w, seed, flags, _ptr(values), _ptr(positions), _ptr(hashes),
                                              capacity, C.byref(result)))
        return result

    # ---- convenience wrappers returning host numpy arrays
    def _span(self, first, n):
        end = self.n_bases if not n else min(self.n_bases, first + n)
        return max(end - first, 0)

    def kmers(self, k, seed=0, canonical=False, drop_last=False, first=0, n=0, arrays=True):
        span = self._span(first, n)
        c = self.ctx
        v = c.empty_u64(span) if arrays else None
        h = c.empty_u64(span) if arrays else None
        ok = c.empty_u8(span) if arrays else None
        r = self.kmers_raw(k, seed, _flags(canonical, drop_last, True), first, n, v, h, ok)
        out = r.as_dict()
        out["sum_hash"] = out.pop("xor_pos")
        if arrays:
            out.update(values=_host_u64(v, span), hashes=_host_u64(h, span), valid=ok[:span].cpu().numpy().copy())
        return out

    def kmers128(self, k, seed=0, canonical=False, drop_last=False, first=0, n=0, arrays=True):
        """k-mers up to k = 64 (kmer_view<__uint128_t>): values has shape (n, 2), uint64 — column 0 the low word, column 1 the high word;
        hashes are hash64_u128(lo, hi, seed).  xor_value / aux: XOR of the low / high words."""
        import torch

        span = self._span(first, n)
        c = self.ctx
        v = torch.empty((max(span, 1), 2), dtype=torch.int64, device=c.torch_device) if arrays else None
        h = c.empty_u64(span) if arrays else None
        ok = c.empty_u8(span) if arrays else None
        r = self.kmers128_raw(k, seed, _flags(canonical, drop_last, True), first, n, v, h, ok)
        out = r.as_dict()
        out["sum_hash"] = out.pop("xor_pos")
        if arrays:
            out.update(values=v[:span].cpu().numpy().view(np.uint64).copy(), hashes=_host_u64(h, span), valid=ok[:span].cpu().numpy().copy())
        return out

    def kmer_counts(self, table, k, canonical=False, drop_last=False, first=0, n=0, valid=False):
        """The table's count of the k-mer at every position of the range (k <= 64; 0 where no k-mer starts or the key is absent), looked
        up inside the scan: (counts, result) or, with valid=True, (counts, valid, result).  counts is an int32 device tensor holding the
        uint32 counts, valid a uint8 device tensor; result carries count, xor_value, aux as kmers128 and found (valid k-mers whose key is
        in the table) and sum_counts (wrapping sum of the counts looked up)."""
        import torch

        span = self._span(first, n)
        c = self.ctx
        counts = torch.empty(max(span, 1), dtype=torch.int32, device=c.torch_device)
        ok = c.empty_u8(span) if valid else None
        r = self.kmer_counts_raw(table, k, _flags(canonical, drop_last, True), first, n, counts, ok)
        out = r.as_dict()
        out["found"] = out.pop("xor_hash")
        out["sum_counts"] = out.pop("xor_pos")
        return (counts[:span], ok[:span], out) if valid else (counts[:span], out)

    def _device_offsets(self, offsets):
        """the offsets read_counts hands to the scan: the caller's, or the batch's own uploaded once; None where the batch needs none"""
        import torch

        if offsets is not None:
            if isinstance(offsets, torch.Tensor):
                if not (offsets.is_cuda and offsets.element_size() == 8 and offsets.is_contiguous() and offsets.numel() == self.n_seqs + 1):
                    raise ValueError("offsets: a contiguous 64-bit device tensor of n_seqs + 1 entries")
                return offsets
            host = np.ascontiguousarray(offsets, dtype=np.uint64)
            if len(host) != self.n_seqs + 1:
                raise ValueError("offsets: n_seqs + 1 entries")
            return torch.from_numpy(host.view(np.int64)).to(self.ctx.torch_device)
        if self._d_offsets is None and self.offsets is not None and len(self.offsets) == self.n_seqs + 1:
            self._d_offsets = torch.from_numpy(self.offsets.view(np.int64)).to(self.ctx.torch_device)
        return self._d_offsets  # None on a batch that is neither fixed-length nor a single sequence: the library refuses with a message

    def read_counts(self, table, k, min_count=1, canonical=False, drop_last=False, first=0, n=0, offsets=None, into=None):
        """The counts kmer_counts looks up, reduced per sequence inside the scan: (ReadCounts, result).  One 48-byte record per sequence
        of the batch — n_kmers, n_found, n_solid (count >= min_count), min_count, max_count, sum_counts and the span of the weak
        k-mers (count < min_count) — instead of five bytes per base.  The scan writes the records of the sequences the range
        [first, first + n) meets; every other record of a new buffer is the identity (no k-mers).  into= an earlier ReadCounts merges
        into its records (BL_READ_COUNTS_ACCUMULATE): ranges that cut a read anywhere add up to the whole-batch answer.  offsets: the
        batch's n_seqs + 1 offsets (host array or device tensor), needed only where the batch was not made from offsets by upload /
        from_tensor and is neither fixed-length nor a single sequence (the device parser's batches).  result as kmer_counts."""
        d_offsets = self._device_offsets(offsets)
        rc = into if into is not None else ReadCounts(self.ctx, self.n_seqs)
        if rc.n_seqs != self.n_seqs:
            raise ValueError("into= holds the records of another batch")
        self.ctx._inputs_ready()
        r = self.read_counts_raw(table, k, _flags(canonical, drop_last, True), int(min_count), rc.records, first, n, d_offsets,
                                 READ_COUNTS_ACCUMULATE if into is not None else READ_COUNTS_INIT)
        out = r.as_dict()
        out["found"] = out.pop("xor_hash")
        out["sum_counts"] = out.pop("xor_pos")
        return rc, out

    def select_read_counts_raw(self, counts, valid, quantiles, out_quantiles, out_n_kmers=None, first=0, n=0, offsets=None):
        """bl_select_read_counts: `counts` / `valid` are what kmer_counts_raw wrote for the range, `quantiles` a sequence of (num, den)
        pairs (1 .. 4 of them), `out_quantiles` takes n_seqs * len(quantiles) uint32 words, `out_n_kmers` n_seqs (or None), `offsets` as
        read_counts_raw.  Synchronous; it waits for the scans in flight itself.  The library checks every argument."""
        n_q = len(quantiles)
        num = (C.c_uint32 * max(n_q, 1))(*[int(q[0]) for q in quantiles])
        den = (C.c_uint32 * max(n_q, 1))(*[int(q[1]) for q in quantiles])
        check(self._lib.bl_select_read_counts(self.ctx._h, self._h, first, n, _ptr(counts), _ptr(valid), _ptr(offsets), num, den, n_q,
                                              _ptr(out_quantiles), _ptr(out_n_kmers)))

    # positions per chunk of read_quantiles: 2^26 positions are 320 MB of reused buffers (5 bytes per position), and a scan of that many
    # takes milliseconds, so that the chunk's two launches and its sync are noise; a larger chunk buys nothing but memory
    QUANTILE_CHUNK = 1 << 26

    def _sequence_chunks(self, offsets, chunk_positions):
        """[first, end) ranges that end on sequence boundaries and hold at most chunk_positions (a longer sequence: a range of its own)"""
        n_bases, limit = self.n_bases, 1 << 31
        if offsets is None and (self.read_len or self.n_seqs <= 1):
            length = int(self.read_len) or n_bases
            if min(length, n_bases) > limit:
                raise ValueError("a sequence is longer than 2^31 positions: bl_select_read_counts takes a whole sequence in one range")
            step = max(1, chunk_positions // max(length, 1)) * max(length, 1)
            return [(b, min(b + step, n_bases)) for b in range(0, n_bases, step)]
        if offsets is None:
            raise ValueError("offsets: the batch keeps none and is neither fixed-length nor a single sequence; pass offsets=")
        if hasattr(offsets, "cpu"):  # a device tensor: the chunks are cut on the host
            bounds = offsets.cpu().numpy().view(np.uint64)
        else:
            bounds = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(bounds) != self.n_seqs + 1:
            raise ValueError("offsets: n_seqs + 1 entries")
        out, s, last = [], 0, len(bounds) - 1
        while s < last:
            e = int(np.searchsorted(bounds, bounds[s] + np.uint64(chunk_positions), side="right")) - 1
            e = min(max(e, s + 1), last)
            if int(bounds[e] - bounds[s]) > limit:
                raise ValueError("a sequence is longer than 2^31 positions: bl_select_read_counts takes a whole sequence in one range")
            if bounds[e] > bounds[s]:
                out.append((int(bounds[s]), int(bounds[e])))
            s = e
        return out

    def read_quantiles(self, table, k, quantiles=((1, 2),), canonical=False, drop_last=False, offsets=None, chunk_positions=None):
        """Per-sequence quantiles of the counts kmer_counts looks up — ((1, 2),) is the median k-mer abundance of every read, khmer's
        get_median_count: (quantiles, n_kmers, result).  quantiles is an int32 device tensor [n_seqs, n_q] holding the uint32 values
        sorted[min(m - 1, m * num // den)] of the read's m valid k-mers (0 where m = 0), n_kmers an int32 device tensor [n_seqs].  The
        batch is processed in chunks that end on sequence boundaries (the batch's own host offsets, offsets=, or multiples of read_len):
        each chunk runs kmer_counts_raw into ONE reused pair of buffers and then the selection, so that the caller never holds five
        bytes per base of the whole batch.  chunk_positions (default Batch.QUANTILE_CHUNK) bounds a chunk; a longer sequence gets a chunk
        of its own, one longer than 2^31 positions raises ValueError.  result: the chunks' digests folded — sums added, XOR words XORed —
        which is kmer_counts's over the whole batch, word for word."""
        import torch

        quantiles = tuple((int(a), int(b)) for a, b in quantiles)
        chunk = int(chunk_positions) if chunk_positions else self.QUANTILE_CHUNK
        if chunk < 1:
            raise ValueError("chunk_positions must be positive")
        host_offsets = offsets if offsets is not None else (self.offsets if self.offsets is not None and len(self.offsets) == self.n_seqs + 1 else None)
        chunks = self._sequence_chunks(host_offsets, chunk)
        d_offsets = self._device_offsets(offsets)
        n_seqs, dev = self.n_seqs, self.ctx.torch_device
        out_q = torch.zeros((max(n_seqs, 1), max(len(quantiles), 1)), dtype=torch.int32, device=dev)
        out_m = torch.zeros(max(n_seqs, 1), dtype=torch.int32, device=dev)
        widest = max((e - b for b, e in chunks), default=0)
        counts = torch.empty(max(widest, 1), dtype=torch.int32, device=dev)
        valid = torch.empty(max(widest, 1), dtype=torch.uint8, device=dev)
        self.ctx._inputs_ready()
        flags = _flags(canonical, drop_last, True)
        total = dict(count=0, xor_value=0, xor_hash=0, xor_pos=0, aux=0, status=0)
        if not chunks:  # no position at all: the library still checks the arguments
            self.select_read_counts_raw(counts, valid, quantiles, out_q, out_m, 0, 0, d_offsets)
        for b, e in chunks:
            r = self.kmer_counts_raw(table, k, flags, b, e - b, counts, valid).as_dict()
            self.select_read_counts_raw(counts, valid, quantiles, out_q, out_m, b, e - b, d_offsets)
            for word in ("count", "xor_hash", "xor_pos"):  # sums (xor_hash: found, xor_pos: sum_counts)
                total[word] = (total[word] + r[word]) & (2**64 - 1)
            for word in ("xor_value", "aux"):
                total[word] ^= r[word]
        total["found"] = total.pop("xor_hash")
        total["sum_counts"] = total.pop("xor_pos")
        return out_q[:n_seqs], out_m[:n_seqs], total

    def read_medians(self, table, k, canonical=False, drop_last=False, offsets=None, chunk_positions=None):
        """The median k-mer abundance of every sequence, sorted[m // 2] of its m valid k-mers' counts: an int32 device tensor [n_seqs]
        holding the uint32 values.  read_quantiles with ((1, 2),)."""
        return self.read_quantiles(table, k, ((1, 2),), canonical, drop_last, offsets, chunk_positions)[0][:, 0]

    # ---- select and trim: a new batch from per-read spans
    def select_raw(self, spans, flags=0, offsets=None, out_offsets=None, source_index=None):
        """bl_batch_select: `spans` holds n_seqs (begin, end) pairs of 64-bit words (16-byte aligned), `offsets` as read_counts_raw,
        `out_offsets` / `source_index` (or None) take n_seqs + 1 / n_seqs words.  Synchronous; it waits for the scans in flight itself.
        Returns (handle, n_seqs, n_bases) of the new batch; the library checks every argument."""
        h, ns, nb = C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(self._lib.bl_batch_select(self.ctx._h, self._h, _ptr(offsets), _ptr(spans), int(flags), C.byref(h), _ptr(out_offsets), _ptr(source_index),
                                        C.byref(ns), C.byref(nb)))
        return h, int(ns.value), int(nb.value)

    def select(self, spans, keep_empty=False, offsets=None):
        """A new device-resident batch whose sequences are spans of this one's reads (bl_batch_select): (Batch, source_index).
        spans: an int64 device tensor [n_seqs, 2] of read-relative (begin, end), clamped to the read; a read whose span is empty is
        dropped, or, with keep_empty, stays as an empty sequence so that sequence i of the result is read i (paired reads stay in
        step).  source_index: an int64 device tensor, the read every sequence of the result came from.  The new batch keeps its
        offsets on the device (`.offsets`, the host copy, is downloaded when first asked for) and `.read_len` where all its sequences
        are equally long, so read_counts and read_quantiles run on it as they are.  offsets: as read_counts."""
        import torch

        n_seqs = self.n_seqs
        if not (isinstance(spans, torch.Tensor) and spans.is_cuda and spans.dtype == torch.int64 and spans.is_contiguous() and spans.numel() == 2 * n_seqs):
            raise ValueError("spans: a contiguous int64 device tensor [n_seqs, 2]")
        d_offsets = self._device_offsets(offsets)
        dev = self.ctx.torch_device
        out_offsets = torch.empty(n_seqs + 1, dtype=torch.int64, device=dev)
        source_index = torch.empty(max(n_seqs, 1), dtype=torch.int64, device=dev)
        if n_seqs == 0:
            spans = torch.zeros((1, 2), dtype=torch.int64, device=dev)  # (the library wants a pointer)
        self.ctx._inputs_ready()
        h, n_out, n_bases = self.select_raw(spans, capi.SELECT_KEEP_EMPTY if keep_empty else 0, d_offsets, out_offsets, source_index)
        d_out = out_offsets[:n_out + 1]
        fixed = 0  # the library's rule: more than one sequence, all equally long
        if n_out > 1 and n_bases and n_bases % n_out == 0 and bool((d_out[1:] - d_out[:-1] == n_bases // n_out).all()):
            fixed = n_bases // n_out
        b = Batch(self.ctx, h, read_len=fixed)
        b._d_offsets = d_out
        b._offsets_from_device = True
        return b, source_index[:n_out]

    # ---- leaving the device: FASTA / FASTQ text
    def format_raw(self, rule, out=None, capacity=0, index=None, source_index=None, spans=None, tags=None, offsets=None):
        """bl_batch_format: `rule` a capi.FormatRule, `out` a uint8 device tensor (None: sizing only) of `capacity` bytes, `index` a
        TextIndex or None, the arrays 64-bit device tensors or None.  Synchronous.  Returns (n_bytes, n_records); the library checks
        every argument."""
        nb, nr = C.c_uint64(), C.c_uint64()
        check(self._lib.bl_batch_format(self.ctx._h, self._h, _ptr(offsets), index._h if index is not None else None, _ptr(source_index), _ptr(spans), _ptr(tags),
                                        C.byref(rule), _ptr(out), int(capacity), C.byref(nb), C.byref(nr)))
        return int(nb.value), int(nr.value)

    @staticmethod
    def format_rule(fmt="fastq", tag_label="", prefix="", first_number=0, line_width=0, quality_fill="I", skip_empty=False, tag_length=False):
        r = capi.FormatRule()
        r.format = {"fasta": capi.FORMAT_FASTA, "fastq": capi.FORMAT_FASTQ}[fmt] if isinstance(fmt, str) else int(fmt)
        r.flags = (capi.FORMAT_SKIP_EMPTY if skip_empty else 0) | (capi.FORMAT_TAG_LENGTH if tag_length else 0)
        r.line_width = int(line_width)
        r.quality_fill = quality_fill if isinstance(quality_fill, int) else (quality_fill.encode("latin1") if isinstance(quality_fill, str) else bytes(quality_fill))[0]
        r.name_prefix = prefix.encode("latin1") if isinstance(prefix, str) else bytes(prefix)  # (16 bytes without a NUL reach the library, which refuses them)
        r.first_number = int(first_number) & (2**64 - 1)
        r.tag_label = tag_label.encode("latin1") if isinstance(tag_label, str) else bytes(tag_label)
        return r

    def format(self, fmt="fastq", index=None, source_index=None, spans=None, tags=None, tag_label="", prefix="", first_number=0, line_width=0, quality_fill="I",
               skip_empty=False, tag_length=False):
        """This batch as FASTA / FASTQ text made on the device (bl_batch_format): a uint8 device tensor.  Sequence i becomes
        marker, name, tags, the bases (FASTA: wrapped at line_width) and for FASTQ "+" and the quality.
        index         a TextIndex: names (and for FASTQ qualities) come from the indexed text; without one, names are generated,
                      prefix + decimal(first_number + source read), and the quality is quality_fill
        source_index  int64 device tensor [n_seqs]: the indexed read of every sequence (what select returned); None: sequence i is read i
        spans         int64 device tensor [index.n_records, 2]: the spans that went into select — the quality is cut at their begins;
                      a batch made by apply_edits takes the spans and index of the batch it came from
        tags          int64 device tensor [n_seqs] (uint64 bits): appends " " + tag_label + decimal(tags[i]); tag_length appends " LN:i:" + length
        skip_empty    drop empty sequences (otherwise they are written with empty lines, so that mates stay in step)"""
        import torch

        rule = self.format_rule(fmt, tag_label, prefix, first_number, line_width, quality_fill, skip_empty, tag_length)
        n = self.n_seqs
        for name, t, count in (("source_index", source_index, n), ("tags", tags, n), ("spans", spans, None)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.element_size() == 8 and t.is_contiguous() and (count is None or t.numel() >= count)):
                raise ValueError(name + ": a contiguous 64-bit device tensor")
        if spans is not None and (index is None or spans.numel() < 2 * index.n_records):
            raise ValueError("spans: one (begin, end) pair per record of the index")
        d_offsets = self._device_offsets(None)
        self.ctx._inputs_ready()
        n_bytes, _ = self.format_raw(rule, None, 0, index, source_index, spans, tags, d_offsets)
        out = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=self.ctx.torch_device)
        self.format_raw(rule, out, n_bytes, index, source_index, spans, tags, d_offsets)
        return out[:n_bytes]

    def write(self, path, append=False, compress=False, eof=True, **how):
        """format(**how) written to `path` (bl_text_write: the download in chunks through two pinned buffers, a chunk written while the
        next copies).  compress=True writes BGZF instead (bl_text_write_bgzf: the text is deflated on the device, chunk by chunk, and only
        compressed bytes are downloaded); eof=False leaves the EOF marker out, for a file that further calls append to — the last call
        writes it.  Returns the bytes written to the file (with compress: what the file grew by; 0 where `path` is no regular file)."""
        return self.ctx._write_text(self.format(**how), path, append, compress, eof)

    def read_spans_raw(self, records, rule, spans, stat=None, offsets=None):
        """bl_read_spans: `records` are the whole-batch records of read_counts_raw, `rule` a capi.SpanRule, `spans` takes n_seqs pairs of
        64-bit words, `stat` (or None) is a 32-bit word per read.  Asynchronous on the context's stream."""
        check(self._lib.bl_read_spans(self.ctx._h, self._h, _ptr(offsets), _ptr(records), _ptr(stat), C.byref(rule), _ptr(spans)))

    @staticmethod
    def _fraction(x, default):
        if x is None:
            return default
        if isinstance(x, (tuple, list)):
            return int(x[0]), int(x[1])
        from fractions import Fraction

        f = Fraction(x).limit_denominator(1 << 16)
        return f.numerator, f.denominator

    def read_spans(self, read_counts, k, trim="prefix", min_len=None, min_kmers=0, solid_min=None, solid_max=None, stat=None, stat_range=None, offsets=None):
        """One span per read from the ReadCounts of a whole-batch read_counts(table, k, min_count) (bl_read_spans): an int64 device
        tensor [n_seqs, 2] for select.  trim: "none", "prefix" (khmer's trim-low-abund: cut at the first weak k-mer, keeping all of it
        but its last base), "suffix" (the mirror image) or "longer".  The span is (0, 0) where it is shorter than min_len (default k),
        the read has fewer than min_kmers valid k-mers, its solid fraction lies outside [solid_min, solid_max] — (num, den) pairs or
        numbers in [0, 1] — or stat (an int32 device tensor [n_seqs], e.g. read_medians) lies outside stat_range = (lo, hi)."""
        import torch

        trims = {"none": capi.TRIM_NONE, "prefix": capi.TRIM_PREFIX, "suffix": capi.TRIM_SUFFIX, "longer": capi.TRIM_LONGER}
        if trim not in trims:
            raise ValueError("trim: none, prefix, suffix or longer")
        if read_counts.n_seqs != self.n_seqs:
            raise ValueError("read_counts holds the records of another batch")
        rule = capi.SpanRule()
        rule.trim, rule.k = trims[trim], int(k)
        rule.min_len = int(k) if min_len is None else int(min_len)
        rule.min_kmers = int(min_kmers)
        rule.solid_min_num, rule.solid_min_den = self._fraction(solid_min, (0, 1))
        rule.solid_max_num, rule.solid_max_den = self._fraction(solid_max, (1, 1))
        rule.stat_lo, rule.stat_hi = (0, 2**32 - 1) if stat_range is None else (int(stat_range[0]), int(stat_range[1]))
        if stat is not None:
            if not (stat.is_cuda and stat.element_size() == 4 and stat.is_contiguous() and stat.numel() == self.n_seqs):
                raise ValueError("stat: a contiguous 32-bit device tensor of n_seqs entries")
        spans = torch.zeros((max(self.n_seqs, 1), 2), dtype=torch.int64, device=self.ctx.torch_device)
        self.ctx._inputs_ready()
        self.read_spans_raw(read_counts.records, rule, spans, stat, self._device_offsets(offsets))
        return spans[:self.n_seqs]

    def trim_by_counts(self, table, k, min_count, trim="prefix", min_len=None, min_kmers=0, solid_min=None, solid_max=None, canonical=False,
                       drop_last=False, keep_empty=False, offsets=None):
        """Abundance trimming and filtering in one chain on the device: read_counts(table, k, min_count), read_spans, select.
        (Batch, source_index, ReadCounts): the trimmed reads as a new batch, where each came from, and the source's records."""
        rc, _ = self.read_counts(table, k, min_count, canonical, drop_last, offsets=offsets)
        spans = self.read_spans(rc, k, trim, min_len, min_kmers, solid_min, solid_max, offsets=offsets)
        out, source_index = self.select(spans, keep_empty, offsets=offsets)
        return out, source_index, rc

    # ---- quality trimming and filtering: spans from the quality bytes of the indexed text
    def read_quality_raw(self, index, rule, records=None, spans=None, stats=None):
        """bl_scan_read_quality: `index` the TextIndex this batch was built with, `rule` a capi.QualityRule, `records` (n_seqs rows of 48
        bytes) and `spans` (n_seqs pairs of 64-bit words) 16-byte aligned device tensors or None, `stats` a capi.QualityStats or None.
        Asynchronous on the context's stream without stats.  The library checks every argument."""
        check(self._lib.bl_scan_read_quality(self.ctx._h, self._h, index._h if index is not None else None, C.byref(rule), _ptr(records), _ptr(spans),
                                             C.byref(stats) if stats is not None else None))

    @staticmethod
    def quality_rule(phred=33, front_q=0, back_q=0, maxsum_q=(0, 0), window=None, low_q=0, max_low=None, mean_q=0, max_ambiguous=None, min_len=0,
                     max_len=0, max_ee=None, quality_fill="I"):
        r = capi.QualityRule()
        r.phred_base = int(phred)
        r.quality_fill = quality_fill if isinstance(quality_fill, int) else (quality_fill.encode("latin1") if isinstance(quality_fill, str) else bytes(quality_fill))[0]
        r.front_q, r.back_q = int(front_q), int(back_q)
        r.maxsum_front_q, r.maxsum_back_q = (int(maxsum_q), int(maxsum_q)) if isinstance(maxsum_q, int) else (int(maxsum_q[0]), int(maxsum_q[1]))
        r.window_len, r.window_q = (0, 0) if window is None else (int(window[0]), int(window[1]))
        r.low_q = int(low_q)
        r.low_max_num, r.low_max_den = Batch._fraction(max_low, (1, 1))
        r.mean_q = int(mean_q)
        r.max_ambiguous = 2**32 - 1 if max_ambiguous is None else int(max_ambiguous)
        r.min_len, r.max_len = int(min_len), int(max_len)
        r.max_ee = 2**64 - 1 if max_ee is None else min(int(math.floor(max_ee * 2**31)), 2**64 - 1)
        return r

    def read_quality(self, index, phred=33, front_q=0, back_q=0, maxsum_q=(0, 0), window=None, low_q=0, max_low=None, mean_q=0, max_ambiguous=None,
                     min_len=0, max_len=0, max_ee=None, quality_fill="I", stats=False):
        """Trim and filter every read by its quality values (bl_scan_read_quality): a ReadQuality.  `index` is the TextIndex this batch
        came with (from_text_indexed, device_batches(indexed=True)); a FASTA index gives quality_fill everywhere.  The Phred value of a
        byte is min(max(byte - phred, 0), 93).  Trimming, in this order, each off at 0 / None:
        front_q, back_q   cut the leading values below front_q and the trailing ones below back_q
        maxsum_q          (front, back) or one number: the running-sum cut of BWA and cutadapt -q
        window            (W, q): cut at the first window of W values whose mean is below q, and the values below q in front of it
        Then the filters over the trimmed span: min_len, max_len (0: none), max_ambiguous bases that are not ACGTU, max_low = the
        fraction ((num, den) or a number) of values below low_q allowed, mean_q, max_ee = the expected number of errors allowed.
        stats=True makes the call synchronous and fills `.stats`."""
        import torch

        rule = self.quality_rule(phred, front_q, back_q, maxsum_q, window, low_q, max_low, mean_q, max_ambiguous, min_len, max_len, max_ee, quality_fill)
        n = self.n_seqs
        dev = self.ctx.torch_device
        records = torch.zeros((max(n, 1), 6), dtype=torch.int64, device=dev)  # (torch allocations are 16-byte aligned)
        spans = torch.zeros((max(n, 1), 2), dtype=torch.int64, device=dev)
        st = capi.QualityStats() if stats else None
        self.ctx._inputs_ready()
        self.read_quality_raw(index, rule, records, spans, st)
        return ReadQuality(n, records[:n], spans[:n], st.as_dict() if stats else None)

    def intersect_spans_raw(self, a, b, flags, out, offsets=None):
        """bl_spans_intersect: `a`, `b` (or None) and `out` hold n_seqs pairs of 64-bit words, 16-byte aligned; out may be a or b.
        Asynchronous on the context's stream."""
        check(self._lib.bl_spans_intersect(self.ctx._h, self._h, _ptr(offsets), _ptr(a), _ptr(b), int(flags), _ptr(out)))

    def intersect_spans(self, a, b=None, paired=False, offsets=None):
        """The spans of `a` and `b` joined read by read (bl_spans_intersect): an int64 device tensor [n_seqs, 2].  Both are clamped to
        the read as select clamps them; the result is [max of the begins, min of the ends), (0, 0) where that is empty.  b=None: a
        alone.  paired: reads 2j and 2j + 1 are mates, and where either span is empty both become (0, 0)."""
        import torch

        n = self.n_seqs
        for name, t in (("a", a), ("b", b)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == 2 * n):
                raise ValueError(name + ": a contiguous int64 device tensor [n_seqs, 2]")
        out = torch.zeros((max(n, 1), 2), dtype=torch.int64, device=self.ctx.torch_device)
        if n == 0:
            return out[:0]
        self.ctx._inputs_ready()
        self.intersect_spans_raw(a, b, capi.SPANS_PAIRED if paired else 0, out, self._device_offsets(offsets))
        return out[:n]

    def trim_by_quality(self, index, paired=False, keep_empty=None, **rule):
        """Quality trimming and filtering in one chain on the device: read_quality(index, **rule), intersect_spans(paired) where the
        reads are interleaved mates, select.  (Batch, source_index, spans, ReadQuality): the trimmed reads as a new batch, where each
        came from, the spans that went into select (what format takes for the qualities) and the source's records.  keep_empty defaults
        to `paired`, so that mates stay in step."""
        rq = self.read_quality(index, **rule)
        spans = self.intersect_spans(rq.spans, None, True) if paired else rq.spans
        out, source_index = self.select(spans, paired if keep_empty is None else keep_empty)
        return out, source_index, spans, rq

    # ---- adapters, read-through between mates and poly tails: spans from the bases
    def read_adapters_raw(self, rule, records=None, spans=None, stats=None, spans_in=None, offsets=None):
        """bl_scan_read_adapters: `rule` a capi.AdapterRule, `spans_in` (n_seqs pairs of 64-bit words) or None, `records` (n_seqs rows of
        32 bytes) and `spans` 16-byte aligned device tensors or None, `stats` a capi.AdapterStats or None, `offsets` as select.
        Asynchronous on the context's stream without stats.  The library checks every argument."""
        check(self._lib.bl_scan_read_adapters(self.ctx._h, self._h, _ptr(offsets), _ptr(spans_in), C.byref(rule), _ptr(records), _ptr(spans),
                                              C.byref(stats) if stats is not None else None))

    @staticmethod
    def _poly_mask(letters):
        mask = 0
        for ch in (letters.decode("latin1") if isinstance(letters, (bytes, bytearray)) else letters):
            code = "ACGT".find(ch.upper().replace("U", "T"))
            if code < 0:
                raise ValueError("a poly base is one of ACGT: %r" % (ch,))
            mask |= 1 << code
        return mask

    @staticmethod
    def adapter_rule(adapters=(), paired=False, min_overlap=3, max_error=0.1, pair_min_overlap=30, pair_max_error=0.2, pair_max_diff=5, poly_before="",
                     poly_after="", poly_min_len=10, poly_per=8, poly_max_mismatch=5, min_len=0):
        """The capi.AdapterRule (bl_adapter_rule) of read_adapters' arguments, for read_adapters_raw: `adapters` one sequence or up to 8 (str or
        bytes, 1 .. 64 bases), max_error and pair_max_error a number or (num, den), the poly arguments strings of bases.  Raises ValueError
        for what cannot be written into the struct; the library refuses everything else."""
        r = capi.AdapterRule()
        if isinstance(adapters, (str, bytes, bytearray)):
            adapters = [adapters]
        adapters = [a.encode("latin1") if isinstance(a, str) else bytes(a) for a in adapters]
        if len(adapters) > capi.MAX_ADAPTERS:
            raise ValueError("at most %d adapters" % capi.MAX_ADAPTERS)
        r.flags = capi.ADAPTERS_PAIRED if paired else 0
        r.n_adapters = len(adapters)
        for a, text in enumerate(adapters):
            if not 1 <= len(text) <= capi.ADAPTER_MAX_LEN:
                raise ValueError("an adapter holds 1 .. %d bases" % capi.ADAPTER_MAX_LEN)
            r.adapter_len[a] = len(text)
            C.memmove(r.adapters[a], text, len(text))
        r.min_overlap = int(min_overlap)
        r.error_num, r.error_den = Batch._fraction(max_error, (1, 10))
        r.pair_min_overlap = int(pair_min_overlap)
        r.pair_error_num, r.pair_error_den = Batch._fraction(pair_max_error, (1, 5))
        r.pair_max_diff = int(pair_max_diff)
        r.poly_before, r.poly_after = Batch._poly_mask(poly_before), Batch._poly_mask(poly_after)
        r.poly_min_len, r.poly_per, r.poly_max_mismatch = int(poly_min_len), int(poly_per), int(poly_max_mismatch)
        r.min_len = int(min_len)
        return r

    def read_adapters(self, adapters=(), paired=False, spans=None, min_overlap=3, max_error=0.1, pair_min_overlap=30, pair_max_error=0.2, pair_max_diff=5,
                      poly_before="", poly_after="", poly_min_len=10, poly_per=8, poly_max_mismatch=5, min_len=0, stats=False, offsets=None):
        """Cut poly tails, read-through between mates and 3' adapters from every read (bl_scan_read_adapters; the header states the
        rule): a ReadAdapters.  `spans`: the spans to start from (read_quality's), None for the whole reads.  Four steps, each off at
        its empty value:
        poly_before   bases such as "G" or "ACGT": a 3' tail of at least poly_min_len of one of them goes, with one mismatch allowed per
                      poly_per bases (0: none) and poly_max_mismatch at most
        paired        reads 2j and 2j + 1 are mates: where the first I bases of one are the reverse complement of the first I of the other
                      (I >= pair_min_overlap, at most pair_max_error of them and pair_max_diff differing), both end at I
        adapters      up to 8 sequences of up to 64 bases (biolib_amd.ADAPTERS has the Illumina ones): the best match without indels of
                      at least min_overlap bases with at most max_error ((num, den) or a number) of them differing; the read ends there
        poly_after    as poly_before, on what is left
        A result shorter than min_len gets the span (0, 0).  stats=True makes the call synchronous and fills `.stats`."""
        import torch

        rule = self.adapter_rule(adapters, paired, min_overlap, max_error, pair_min_overlap, pair_max_error, pair_max_diff, poly_before, poly_after,
                                 poly_min_len, poly_per, poly_max_mismatch, min_len)
        n = self.n_seqs
        dev = self.ctx.torch_device
        if spans is not None and not (isinstance(spans, torch.Tensor) and spans.is_cuda and spans.dtype == torch.int64 and spans.is_contiguous() and
                                      spans.numel() == 2 * n):
            raise ValueError("spans: a contiguous int64 device tensor [n_seqs, 2]")
        records = torch.zeros((max(n, 1), 4), dtype=torch.int64, device=dev)  # (torch allocations are 16-byte aligned)
        out = torch.zeros((max(n, 1), 2), dtype=torch.int64, device=dev)
        st = capi.AdapterStats() if stats else None
        self.ctx._inputs_ready()
        self.read_adapters_raw(rule, records, out, st, spans, self._device_offsets(offsets))
        return ReadAdapters(n, records[:n], out[:n], st.as_dict() if stats else None)

    def trim_adapters(self, adapters, paired=False, spans=None, keep_empty=None, **rule):
        """Adapter trimming in one chain on the device: read_adapters(adapters, paired, spans, **rule), intersect_spans(paired) where the
        reads are interleaved mates, select.  (Batch, source_index, spans, ReadAdapters): the trimmed reads as a new batch, where each
        came from, the spans that went into select (what format takes for the qualities) and the source's records.  `spans` is where a
        quality step's result goes in: b.trim_adapters(A, paired=True, spans=rq.spans) follows read_quality.  keep_empty defaults to
        `paired`, so that mates stay in step."""
        ra = self.read_adapters(adapters, paired, spans, **rule)
        out_spans = self.intersect_spans(ra.spans, None, True) if paired else ra.spans
        out, source_index = self.select(out_spans, paired if keep_empty is None else keep_empty)
        return out, source_index, out_spans, ra

    # ---- duplicates: exact copies of reads and pairs
    def read_duplicates_raw(self, rule, records=None, spans=None, stats=None, spans_in=None, scores=None, offsets=None):
        """bl_scan_read_duplicates: `rule` a capi.DedupRule, `spans_in` (n_seqs pairs of 64-bit words) and `scores` (n_seqs 64-bit words)
        or None, `records` (n_units rows of 16 bytes) and `spans` 16-byte aligned device tensors or None, `stats` a capi.DedupStats or
        None, `offsets` as select.  The library checks every argument."""
        check(self._lib.bl_scan_read_duplicates(self.ctx._h, self._h, _ptr(offsets), _ptr(spans_in), _ptr(scores), C.byref(rule), _ptr(records),
                                                _ptr(spans), C.byref(stats) if stats is not None else None))

    def read_duplicates(self, paired=False, spans=None, canonical=False, prefix_len=0, scores=None, stats=False, offsets=None, hash_bits=0, seed=0):
        """Find the exact duplicates among the reads, or among the pairs of interleaved mates (bl_scan_read_duplicates; the header
        states the rule): a ReadDuplicates.  `spans`: the spans to compare (read_adapters'), None for the whole reads.
        canonical    a read also equals its reverse complement, a pair the pair with its mates swapped
        prefix_len   only the first prefix_len bases of every span count (0: all)
        scores       an int64 device tensor, one value per READ (read_quality's records[:, 2], the sum of the Phred values): the member
                     of a class with the largest score stays, the first on a tie; None: the first stays
        hash_bits and seed change how the work is done, never a result.  stats=True fills `.stats`."""
        import torch

        n = self.n_seqs
        dev = self.ctx.torch_device
        if spans is not None and not (isinstance(spans, torch.Tensor) and spans.is_cuda and spans.dtype == torch.int64 and spans.is_contiguous() and
                                      spans.numel() == 2 * n):
            raise ValueError("spans: a contiguous int64 device tensor [n_seqs, 2]")
        if scores is not None:
            if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.int64 and scores.numel() == n):
                raise ValueError("scores: an int64 device tensor [n_seqs]")
            scores = scores.contiguous()
        rule = capi.DedupRule()
        rule.flags = (capi.DEDUP_PAIRED if paired else 0) | (capi.DEDUP_CANONICAL if canonical else 0)
        rule.hash_bits, rule.prefix_len, rule.seed = int(hash_bits), int(prefix_len), int(seed) & (2**64 - 1)
        n_units = n // 2 if paired else n
        records = torch.zeros((max(n_units, 1), 2), dtype=torch.int64, device=dev)  # (torch allocations are 16-byte aligned)
        out = torch.zeros((max(n, 1), 2), dtype=torch.int64, device=dev)
        st = capi.DedupStats() if stats else None
        self.ctx._inputs_ready()
        self.read_duplicates_raw(rule, records, out, st, spans, scores, self._device_offsets(offsets))
        return ReadDuplicates(n_units, records[:n_units], out[:n], st.as_dict() if stats else None)

    def dedup(self, paired=False, spans=None, keep_empty=None, **rule):
        """Duplicate removal in one chain on the device: read_duplicates(paired, spans, **rule), intersect_spans(paired) where the reads
        are interleaved mates, select.  (Batch, source_index, spans, ReadDuplicates): the reads that stay as a new batch, where each
        came from, the spans that went into select (what format takes for the qualities) and the source's records.  `spans` is where
        the trimming steps' result goes in: b.dedup(paired=True, spans=ra.spans, scores=rq.records[:, 2]) follows read_quality and
        read_adapters.  keep_empty defaults to False here: a duplicate pair goes as a whole."""
        rd = self.read_duplicates(paired, spans, **rule)
        out_spans = self.intersect_spans(rd.spans, None, True) if paired else rd.spans
        out, source_index = self.select(out_spans, False if keep_empty is None else keep_empty)
        return out, source_index, out_spans, rd

    # ---- threading: the reads' steps through the compacted graph
    def read_steps_raw(self, table, k, flags, nodes, unitig_offsets, n_unitigs, steps, capacity, first=0, n=0, offsets=None, stats=None):
        """bl_scan_read_steps: `nodes` / `unitig_offsets` are what CountTable.unitigs_raw filled for `table` and k, `steps` (or None with
        capacity 0: the sizing call) takes `capacity` 32-byte records, `offsets` as read_counts_raw.  Synchronous; it waits for the scans
        in flight itself.  Returns (rc, capi.StepStats): rc is BL_OK or BL_ERR_CAPACITY, any other error raises."""
        stats = stats if stats is not None else capi.StepStats()
        rc = self._lib.bl_scan_read_steps(self.ctx._h, self._h, int(first), int(n), int(k), int(flags), table._h, _ptr(nodes), _ptr(unitig_offsets),
                                          int(n_unitigs), _ptr(offsets), _ptr(steps), int(capacity), C.byref(stats))
        if rc != capi.BL_ERR_CAPACITY:
            check(rc)
        return rc, stats

    # positions per call of read_steps: the library's own bound on a range
    STEPS_CHUNK = 1 << 31

    def read_steps(self, unitigs, offsets=None, chunk_positions=None):
        """Every read threaded through the compacted graph (bl_scan_read_steps; the header states the rules): a ReadSteps.  `unitigs` is
        what CountTable.unitigs(k, nodes=True) or unitigs(k, links=True) returned; the table it came from must still be open.  One
        32-byte record per unitig visit: the k-mers at pos .. pos + n_kmers - 1 of sequence seq are the k-mers offset .. of unitig
        end >> 1 read in orientation end & 1; flags has STEP_LINKED where the read came from the previous step over a link.  A sizing
        call, then one allocation.  A batch of more than 2^31 positions (or chunk_positions) goes in chunks that end on sequence
        boundaries, as read_quantiles cuts them, so that no step is cut.  offsets as read_counts."""
        import torch

        nodes = unitigs.nodes if unitigs.nodes is not None else unitigs._nodes
        table = unitigs._table
        if nodes is None or table is None or getattr(table, "_h", None) is None:
            raise ValueError("read_steps needs unitigs(k, nodes=True) or unitigs(k, links=True) of a table that is still open")
        if table.n_distinct == 0:
            nodes = None
        d_offsets = self._device_offsets(offsets)
        limit = int(chunk_positions) if chunk_positions else self.STEPS_CHUNK
        if self.n_bases <= limit:
            chunks = [(0, self.n_bases)]
        else:
            host_offsets = offsets if offsets is not None else (self.offsets if self.offsets is not None and len(self.offsets) == self.n_seqs + 1 else None)
            chunks = self._sequence_chunks(host_offsets, limit)
        self.ctx._inputs_ready()
        args = (table, unitigs.k, 0, nodes, unitigs.offsets if table.n_distinct else None, unitigs.n_unitigs)
        sized = [self.read_steps_raw(*args, None, 0, b, e - b, d_offsets)[1].as_dict() if e > b else None for b, e in chunks]
        total = sum(st["n_steps"] for st in sized if st)
        steps = torch.empty((max(total, 1), 4), dtype=torch.int64, device=self.ctx.torch_device)  # (torch allocations are 16-byte aligned)
        stats, at = dict(n_valid=0, n_found=0, n_steps=0, n_chains=0, n_linked=0, longest_step=0), 0
        if not any(sized):  # no position at all: the library still checks the arguments
            self.read_steps_raw(*args, None, 0, 0, 0, d_offsets)
        for (b, e), st in zip(chunks, sized):
            if not st:
                continue
            if st["n_steps"]:
                self.read_steps_raw(*args, steps[at:], st["n_steps"], b, e - b, d_offsets)
            at += st["n_steps"]
            for name in stats:
                stats[name] = max(stats[name], st[name]) if name == "longest_step" else stats[name] + st[name]
        return ReadSteps(self, unitigs, steps[:total], stats, d_offsets)

    # ---- repair: single-substitution correction from a count table
    def read_edits_raw(self, table, k, flags, min_count, min_support, edits, capacity, first=0, n=0, stats=None):
        """bl_scan_read_edits: `edits` (or None with capacity 0: the counting call) takes `capacity` 16-byte records.  Synchronous; it
        waits for the scans in flight itself.  Returns (rc, capi.EditStats): rc is BL_OK or BL_ERR_CAPACITY, any other error raises."""
        stats = stats if stats is not None else capi.EditStats()
        rc = self._lib.bl_scan_read_edits(self.ctx._h, self._h, int(first), int(n), int(k), int(flags), table._h, int(min_count), int(min_support),
                                          _ptr(edits), int(capacity), C.byref(stats))
        if rc != capi.BL_ERR_CAPACITY:
            check(rc)
        return rc, stats

    def read_edits(self, table, k, min_count, min_support=1, canonical=False, first=0, n=0, capacity=None):
        """The single-base repairs the count table supports for the weak runs that begin in the range (bl_scan_read_edits): (edits, stats).
        A weak run — consecutive k-mers of one read with count < min_count — that has the exact extent a substitution at one base p
        gives it, with a solid k-mer on one side, is repaired iff exactly one other base at p makes all of its k-mers solid.  edits: an
        int64 device tensor [n_edits, 2] holding the 16-byte bl_edit records in ascending position (edits_host turns it into a numpy
        record array, edit_reads into (read, position in the read)); stats: runs by class.  Run once more with the reported count
        when `capacity` (default: one edit per 64 positions) was too small."""
        import torch

        span = self._span(first, n)
        cap = max(int(capacity if capacity is not None else span // 64 + 64), 1)
        self.ctx._inputs_ready()
        while True:
            edits = torch.zeros((cap, 2), dtype=torch.int64, device=self.ctx.torch_device)
            rc, stats = self.read_edits_raw(table, k, _flags(canonical, False, False), min_count, min_support, edits, cap, first, n)
            if rc == capi.BL_OK:
                return edits[:int(stats.n_edits)], stats.as_dict()
            cap = int(stats.n_edits)

    @staticmethod
    def edits_host(edits):
        """the records of read_edits as a numpy record array: pos, from, to, support, anchor, reserved"""
        return edits.cpu().numpy().view(np.uint8).reshape(-1, 16).copy().view(capi.EDIT_DTYPE).reshape(-1)

    def edit_reads(self, edits, offsets=None):
        """(read, position inside the read) of every edit, two int64 device tensors, for reporting: torch.searchsorted over the device
        offsets (offsets: as read_counts; a fixed-length or single-sequence batch needs none)."""
        import torch

        pos = edits[:, 0].contiguous()
        d_offsets = self._device_offsets(offsets)
        if d_offsets is None:
            if self.n_seqs > 1 and not self.read_len:
                raise ValueError("offsets: this batch does not know its own")
            L = self.read_len if self.read_len else max(self.n_bases, 1)
            read = torch.div(pos, L, rounding_mode="floor")
            return read, pos - read * L
        read = torch.searchsorted(d_offsets, pos, right=True) - 1  # the LAST sequence that starts at or before pos: empty ones are skipped
        return read, pos - d_offsets[read]

    def apply_edits(self, edits):
        """A new batch with the edits of read_edits applied (bl_batch_apply_edits): the same reads, offsets and origin, every byte
        verbatim except the edited ones.  This batch is not modified."""
        if not (edits.is_cuda and edits.element_size() == 8 and edits.is_contiguous() and edits.dim() == 2 and edits.shape[1] == 2):
            raise ValueError("edits: a contiguous int64 device tensor [n_edits, 2]")
        self.ctx._inputs_ready()
        h = C.c_void_p()
        n = int(edits.shape[0])
        check(self._lib.bl_batch_apply_edits(self.ctx._h, self._h, _ptr(edits) if n else None, n, C.byref(h)))
        b = Batch(self.ctx, h, offsets=self._host_offsets, read_len=self.read_len)
        b._d_offsets = self._d_offsets
        b._offsets_from_device = self._offsets_from_device
        return b

    def correct_by_counts(self, table, k, min_count, min_support=1, canonical=False, passes=1):
        """read_edits and apply_edits chained: (Batch, [edits of each pass], [stats of each pass]).  passes > 1 repeats on the result —
        a repaired base can complete the shape of a neighbouring run — and stops early when a pass makes no edit."""
        batch, all_edits, all_stats = self, [], []
        for _ in range(max(int(passes), 1)):
            edits, stats = batch.read_edits(table, k, min_count, min_support, canonical)
            all_edits.append(edits)
            all_stats.append(stats)
            if stats["n_edits"] == 0:
                break
            batch = batch.apply_edits(edits)
        if batch is self:
            batch = self.apply_edits(all_edits[0])  # no edit at all: still a batch of its own
        return batch, all_edits, all_stats

    def hash_sample128(self, k, seed=0, threshold=2**64 - 1, canonical=False, drop_last=False, first=0, n=0, capacity=None, device=False):
        """k-mers up to k = 64 with hash64_u128(value, seed) < threshold, in position order; values has shape (count, 2) as in kmers128.
        Run again with the count the scan reports when `capacity` (default: the expected number of records) was too small.
        device=True keeps the tensors on the GPU: values_device (int64[capacity, 2], the keys sort_unique128 / jaccard128 take) and
        hashes_device, the first n entries of each."""
        import torch

        span = self._span(first, n)
        guess = capacity if capacity is not None else int(span * min(1.0, (threshold + 1) / 2**64) * 1.1) + 4096
        c = self.ctx

        def run(cap):
            v = torch.empty((cap, 2), dtype=torch.int64, device=c.torch_device)
            p, h = c.empty_u64(cap), c.empty_u64(cap)
            r = Result()
            try:
                self.hash_sample128_raw(k, seed, threshold, _flags(canonical, drop_last, True), first, n, v, p, h, cap, r)
            finally:
                self._last_count = r.count
            cnt = int(r.count)
            out = r.as_dict()
            if device:
                out.update(values_device=v, hashes_device=h, n=cnt)
            else:
                out.update(values=v[:cnt].cpu().numpy().view(np.uint64).copy(), positions=_host_u64(p, cnt), hashes=_host_u64(h, cnt))
            return out

        return self._with_capacity(guess, run)

    def _with_capacity(self, guess, run):
        cap = max(int(guess), 64)
        while True:
            try:
                return run(cap)
            except BiolibError as e:
                if e.code != capi.BL_ERR_CAPACITY:
                    raise
                cap = int(self._last_count) + 64

    def minimizers(self, unit, w, seed=0, canonical=False, first=0, n=0, capacity=None):
        span = self._span(first, n)
        guess = capacity if capacity is not None else int(span * 2.4 / (w + 1)) + 4096

        def run(cap):
            c = self.ctx
            v, p, h = c.empty_u64(cap), c.empty_u64(cap), c.empty_u64(cap)
            r = Result()
            try:
                self.minimizers_raw(unit, w, seed, _flags(canonical, False, True), first, n, v, p, h, cap, r)
            finally:
                self._last_count = r.count
            cnt = int(r.count)
            out = r.as_dict()
            out.update(values=_host_u64(v, cnt), positions=_host_u64(p, cnt), hashes=_host_u64(h, cnt))
            return out

        return self._with_capacity(guess, run)

    def hash_sample(self, k, seed=0, threshold=2**64 - 1, canonical=False, drop_last=False, first=0, n=0, device=False):
        """k-mers with hash64(value, seed) < threshold (hash_sampler over kmer_view).  device=True keeps the value tensor on the GPU."""
        span = self._span(first, n)
        cap = span + 64
        c = self.ctx
        v, p, h = c.empty_u64(cap), c.empty_u64(cap), c.empty_u64(cap)
        r = self.hash_sample_raw(k, seed, threshold, _flags(canonical, drop_last, True), first, n, v, p, h, cap)
        cnt = int(r.count)
        out = r.as_dict()
        if device:
            out.update(values_device=v, n=cnt)
        else:
            out.update(values=_host_u64(v, cnt), positions=_host_u64(p, cnt), hashes=_host_u64(h, cnt))
        return out

    def super_kmer_records(self, k, m, seed=0, canonical=False, first=0, n=0, fused=True):
        """(records int64[n,2], minimizer hashes int64[n]) on the device: the packed super-k-mers of the range, straight from the
        scan (bl_scan_super_kmer_records; fused=False: bl_scan_super_kmers + bl_pack_super_kmers, the same records)"""
        import torch

        span = self._span(first, n)
        c = self.ctx

        def run(cap):
            hs = c.empty_u64(cap)
            r = Result()
            if fused:
                recs = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=c.torch_device)
                c._hold(r, _flags(canonical, False, True))
                try:
                    check(self._lib.bl_scan_super_kmer_records(c._h, self._h, int(first), int(n), int(k), int(m), int(seed), _flags(canonical, False, True),
                                                               C.c_void_p(recs.data_ptr()), C.c_void_p(hs.data_ptr()), int(cap), C.byref(r)))
                finally:
                    self._last_count = r.count
                cnt = int(r.count)
                return recs[:cnt], hs[:cnt]
            fp, sz, mp = c.empty_u64(cap), c.empty_u8(cap), c.empty_u8(cap)
            try:
                self.super_kmers_raw(k, m, seed, _flags(canonical, False, True), first, n, None, fp, mp, sz, hs, cap, r)
            finally:
                self._last_count = r.count
            cnt = int(r.count)
            recs = torch.empty((max(cnt, 1), 2), dtype=torch.int64, device=c.torch_device)
            check(self._lib.bl_pack_super_kmers(c._h, self._h, C.c_void_p(fp.data_ptr()), C.c_void_p(sz.data_ptr()), C.c_void_p(mp.data_ptr()), cnt, int(k), int(m),
                                                C.c_void_p(recs.data_ptr())))
            c.sync()
            return recs[:cnt], hs[:cnt]

        return self._with_capacity(int(span * 2.4 / (k - m + 2)) + 4096, run)

    def super_kmer_records128(self, k, m, seed=0, canonical=False, first=0, n=0, fused=True):
        """(records int64[n, 4], minimizer hashes int64[n]) on the device: the 32-byte super-k-mer records of the range for k up to 64,
        straight from the scan (bl_scan_super_kmer_records128; fused=False: bl_scan_super_kmers + bl_pack_super_kmers128, the same records)"""
        import torch

        span = self._span(first, n)
        c = self.ctx

        def run(cap):
            hs = c.empty_u64(cap)
            if fused:
                r = Result()
                recs = torch.empty((max(cap, 1), 4), dtype=torch.int64, device=c.torch_device)  # (the allocator aligns to 512 bytes)
                c._hold(r, _flags(canonical, False, True))
                try:
                    check(self._lib.bl_scan_super_kmer_records128(c._h, self._h, int(first), int(n), int(k), int(m), int(seed), _flags(canonical, False, True),
                                                                  C.c_void_p(recs.data_ptr()), C.c_void_p(hs.data_ptr()), int(cap), C.byref(r)))
                finally:
                    self._last_count = r.count
                cnt = int(r.count)
                return recs[:cnt], hs[:cnt]
            fp, sz, mp = c.empty_u64(cap), c.empty_u8(cap), c.empty_u8(cap)
            r = Result()
            try:
                self.super_kmers_raw(k, m, seed, _flags(canonical, False, True), first, n, None, fp, mp, sz, hs, cap, r)
            finally:
                self._last_count = r.count
            cnt = int(r.count)
            recs = torch.empty((max(cnt, 1), 4), dtype=torch.int64, device=c.torch_device)
            check(self._lib.bl_pack_super_kmers128(c._h, self._h, C.c_void_p(fp.data_ptr()), C.c_void_p(sz.data_ptr()), C.c_void_p(mp.data_ptr()), cnt, int(k), int(m),
                                                   C.c_void_p(recs.data_ptr())))
            c.sync()
            return recs[:cnt], hs[:cnt]

        return self._with_capacity(int(span * 2.4 / (k - m + 2)) + 4096, run)

    def super_kmers(self, k, m, seed=0, canonical=False, first=0, n=0, capacity=None):
        span = self._span(first, n)
        guess = capacity if capacity is not None else int(span * 2.4 / (k - m + 2)) + 4096

        def run(cap):
            c = self.ctx
            mn, fp, hs = c.empty_u64(cap), c.empty_u64(cap), c.empty_u64(cap)
            mp, sz = c.empty_u8(cap), c.empty_u8(cap)
            r = Result()
            try:
                self.super_kmers_raw(k, m, seed, _flags(canonical, False, True), first, n, mn, fp, mp, sz, hs, cap, r)
            finally:
                self._last_count = r.count
            cnt = int(r.count)
            out = r.as_dict()
            out.update(minimizers=_host_u64(mn, cnt), first_pos=_host_u64(fp, cnt), mm_pos=mp[:cnt].cpu().numpy().copy(),
                       sizes=sz[:cnt].cpu().numpy().copy(), hashes=_host_u64(hs, cnt))
            return out

        return self._with_capacity(guess, run)

    def syncmers(self, k, s, start_offset, end_offset, seed=0, canonical=False, drop_last=False, first=0, n=0, positions=True, capacity=None):
        span = self._span(first, n)
        if not positions:
            r = self.syncmers_raw(k, s, start_offset, end_offset, seed, _flags(canonical, drop_last, True), first, n)
            return r.as_dict()
        guess = capacity if capacity is not None else int(span * 2.6 / (k - s + 1)) + 4096

        def run(cap):
            p = self.ctx.empty_u64(cap)
            r = Result()
            try:
                self.syncmers_raw(k, s, start_offset, end_offset, seed, _flags(canonical, drop_last, True), first, n, p, cap, r)
            finally:
                self._last_count = r.count
            out = r.as_dict()
            out.update(positions=_host_u64(p, int(r.count)))
            return out

        return self._with_capacity(guess, run)

    def syncmers128(self, k, s, start_offset, end_offset, seed=0, canonical=False, drop_last=False, first=0, n=0, positions=True, capacity=None):
        """syncmers of k-mers up to k = 64 (syncmer_sampler over kmer_view<__uint128_t>): as syncmers(), with the s-mers (s <= 32) hashed
        as 16-byte keys, hash64_u128(s-mer, 0, seed) — for k <= 32 the records differ in general from syncmers()'s."""
        span = self._span(first, n)
        if not positions:
            r = self.syncmers128_raw(k, s, start_offset, end_offset, seed, _flags(canonical, drop_last, True), first, n)
            return r.as_dict()
        guess = capacity if capacity is not None else int(span * 2.6 / max(k - s + 1, 1)) + 4096

        def run(cap):
            p = self.ctx.empty_u64(cap)
            r = Result()
            try:
                self.syncmers128_raw(k, s, start_offset, end_offset, seed, _flags(canonical, drop_last, True), first, n, p, cap, r)
            finally:
                self._last_count = r.count
            out = r.as_dict()
            out.update(positions=_host_u64(p, int(r.count)))
            return out

        return self._with_capacity(guess, run)

    def minimizers128(self, unit, w, seed=0, canonical=False, drop_last=False, first=0, n=0, capacity=None, arrays=True):
        """window minimizers of k-mers up to k = 64 (minimizer_sampler over kmer_view<__uint128_t>): as minimizers(), with the units hashed
        as 16-byte keys, hash64_u128(lo, hi, seed), and drop_last honoured for every w.  values has shape (count, 2) as in kmers128."""
        import torch

        span = self._span(first, n)
        if not arrays:
            r = self.minimizers128_raw(unit, w, seed, _flags(canonical, drop_last, True), first, n)
            return dict(r.as_dict(), redone=int(r.redone))
        guess = capacity if capacity is not None else int(span * 2.6 / (w + 1)) + 4096
        c = self.ctx

        def run(cap):
            v = torch.empty((cap, 2), dtype=torch.int64, device=c.torch_device)
            p, h = c.empty_u64(cap), c.empty_u64(cap)
            r = Result()
            try:
                self.minimizers128_raw(unit, w, seed, _flags(canonical, drop_last, True), first, n, v, p, h, cap, r)
            finally:
                self._last_count = r.count
            cnt = int(r.count)
            out = dict(r.as_dict(), redone=int(r.redone))
            out.update(values=v[:cnt].cpu().numpy().view(np.uint64).copy().reshape(cnt, 2), positions=_host_u64(p, cnt), hashes=_host_u64(h, cnt))
            return out

        return self._with_capacity(guess, run)


class Reader:
    """FASTA / FASTQ (plain or gzip) reader of the library (bl_reader_*): host records or device batches."""

    def __init__(self, path, threads=0, shard=None):
        """threads: inflate workers for gzip and BGZF input (0 = one per core, at most 16); plain files use one read-ahead thread.
        shard=(rank, world): this reader takes part `rank` of a plain or BGZF file that `world` readers read between them (BGZF:
        device batches only; the parts' records in rank order are the file's records)"""
        self._lib = capi.lib()
        h = C.c_void_p()
        if shard is not None:
            check(self._lib.bl_reader_open_shard(str(path).encode(), int(shard[0]), int(shard[1]), C.byref(h)))
        else:
            check(self._lib.bl_reader_open_threads(str(path).encode(), int(threads), C.byref(h)))
        self._h = h

    @property
    def shard_range(self):
        """(first byte, end byte) of the file whose members are this reader's own (end = 2^64 - 1: to the end of the file)"""
        a, b = C.c_uint64(), C.c_uint64()
        check(self._lib.bl_reader_shard_range(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    @property
    def kind(self):
        """'plain', 'gzip' or 'bgzf'"""
        return self._lib.bl_reader_kind(self._h).decode()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bl_reader_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def records(self):
        """yield (name, sequence bytes) — host only, no GPU needed"""
        name, seq, n = C.c_char_p(), C.c_void_p(), C.c_uint64()
        while True:
            rc = self._lib.bl_reader_next_record(self._h, C.byref(name), C.byref(seq), C.byref(n))
            if rc == 1:
                return
            check(rc)
            yield name.value.decode("latin1"), C.string_at(seq.value, n.value) if n.value else b""

    def text_spans(self, max_bytes=0):
        """yield the decompressed text as bytes objects cut at record boundaries (what the device-side parser takes)"""
        p, n = C.c_void_p(), C.c_uint64()
        while True:
            rc = self._lib.bl_reader_next_text(self._h, int(max_bytes), C.byref(p), C.byref(n))
            if rc == 1:
                return
            check(rc)
            yield C.string_at(p.value, n.value)

    def device_batches(self, ctx, max_text_bytes=0, indexed=False):
        """yield Batch objects parsed ON THE DEVICE from spans of the decompressed text (regular FASTA / 4-line FASTQ only;
        names are not kept): parallel inflate -> one H2D copy -> bl_batch_from_text.  indexed=True: yield (Batch, TextIndex) — the same
        spans, every batch with the names and qualities of its text (bl_reader_next_batch_device_indexed), for Batch.write(append=True)"""
        while indexed:
            b, ix, ns, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
            check(self._lib.bl_reader_next_batch_device_indexed(ctx._h, self._h, int(max_text_bytes), C.byref(b), C.byref(ix), C.byref(ns), C.byref(nb)))
            if not b.value:
                return
            yield _indexed_batch(ctx, b, ix)
        while True:
            b, ns, nb = C.c_void_p(), C.c_uint64(), C.c_uint64()
            check(self._lib.bl_reader_next_batch_device(ctx._h, self._h, int(max_text_bytes), C.byref(b), C.byref(ns), C.byref(nb)))
            if not b.value:
                return
            yield Batch(ctx, b)

    def batches(self, ctx, max_bases=0, names=True):
        """yield (Batch, names, offsets) of whole records holding at most max_bases bases each (names=False: the list stays
        empty — one call per name is what a Python loop over millions of short reads spends its time on)"""
        while True:
            b, ns, nb = C.c_void_p(), C.c_uint64(), C.c_uint64()
            check(self._lib.bl_reader_next_batch(ctx._h, self._h, int(max_bases), C.byref(b), C.byref(ns), C.byref(nb)))
            if not b.value:
                return
            offs_p, n2 = C.c_void_p(), C.c_uint64()
            check(self._lib.bl_reader_last_batch(self._h, None, C.byref(offs_p), C.byref(n2)))
            offs = np.ctypeslib.as_array(C.cast(offs_p, C.POINTER(C.c_uint64)), shape=(n2.value + 1,)).copy()
            nm = [self._lib.bl_reader_last_name(self._h, i).decode("latin1") for i in range(n2.value)] if names else []
            yield Batch(ctx, b), nm, offs
