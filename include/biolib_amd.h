/* biolib_amd.h — C ABI of the MI355X-native k-mer / minimizer streaming scan.
 *
 * This is the drop-in boundary.  The reference (yhhshb/biolib) has no FFI layer:
 * its boundary is the header-only C++ template surface, so each entry point below names the
 * reference template whose bulk result it produces, and the headers under include/compat/ re-expose those
 * templates (same names, signatures and iteration protocol) on top of these calls.
 *
 *   bl_scan_kmers        wrapper::kmer_view<uint64_t,It>                  include/kmer_view.hpp:25-83 and 162-234
 *                        + hash::hash64::hash(value, seed)                include/hash.hpp:50-59
 *   bl_scan_kmers128     wrapper::kmer_view<__uint128_t,It>               the same template on the reference's 128-bit KmerType, k <= 64
 *                        + hash::hash64::hash<__uint128_t>(value, seed)   include/hash.hpp:55-59 (16 key bytes)
 *   bl_scan_hash_sample128  sampler::hash_sampler over that view          include/hash_sampler.hpp:73-78,136-141
 *   bl_scan_minimizers   wrapper::minimizer_view<K,M,hash64,It>           include/minimizer_view.hpp:14-98 (intended semantics)
 *                        sampler::minimizer_sampler<It,Hash>              include/minimizer_sampler.hpp:12-70
 *   bl_scan_super_kmers  wrapper::super_kmer_view<K,M,hash64>             include/super_kmer_view.hpp:11-58, 121-135
 *   bl_scan_super_kmer_records  the same groups as self-contained records  include/super_kmer_view.hpp:20-24 (the record), §8f rank 4
 *   bl_scan_minimizers128  sampler::minimizer_sampler over kmer_view<__uint128_t,It>  unit <= 64, w <= 64; unit keys of 16 bytes
 *   bl_scan_syncmers     sampler::syncmer_sampler<It,minimizer_position_extractor>
 *                                                                         include/syncmer_sampler.hpp:9-137, include/kmer_view.hpp:250-283
 *   bl_scan_syncmers128  the same sampler over kmer_view<__uint128_t,It>  k <= 64, s <= 32; s-mer keys of 16 bytes (kmer_view.hpp:266-283 in KmerType)
 *   bl_sort_unique_u128, bl_jaccard_sorted_u128, bl_write_run_u128 ..     the consumer of those k-mers: emem::external_memory_vector<__uint128_t>,
 *                        sampler::ordered_unique_sampler, algorithm::jaccard  include/external_memory_vector.hpp, ordered_unique_sampler.hpp, jaccard.hpp
 *   bl_hash64_u64        hash::hash64::hash<uint64_t>                     include/hash.hpp:55-59 (host-side convenience, bit-exact)
 *   bl_hash64_u128       hash::hash64::hash<__uint128_t>                  the same for a 16-byte value
 *
 * Conventions
 *   - Plain C: opaque handles, plain pointers and sizes.  Never throws; every call returns a status
 *     (0 = BL_OK, negative = error) and bl_last_error() gives the message of the calling thread's
 *     last failure.
 *   - A batch is a set of sequences concatenated without separators; offsets[0..n_seqs] delimits
 *     them.  All positions reported are 0-based indices into that concatenation ("global positions");
 *     position - offsets[seq] is the reference's per-view position.
 *   - Output arrays are DEVICE pointers supplied by the caller (any may be NULL = not wanted) and
 *     hold `capacity` records; the scan always returns the full count, so a short buffer is
 *     detected (BL_ERR_CAPACITY) and can be re-run.  Records are in increasing position order.
 *   - All work is enqueued on the context's HIP stream.  Scans are asynchronous unless
 *     BL_FLAG_SYNC is given; results (`bl_result`) are valid after bl_ctx_sync().
 *   - One context per (host thread, device).  A context is not thread-safe; distinct contexts are
 *     independent.
 */
#ifndef BIOLIB_AMD_H
#define BIOLIB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BL_VERSION 100 /* 0.1.0 */

enum {
    BL_OK = 0,
    BL_ERR_INVALID = -1,     /* bad argument (k > 32, w > 64, NULL handle, misaligned pointer, ...) */
    BL_ERR_HIP = -2,         /* a HIP runtime call failed */
    BL_ERR_OOM = -3,         /* device or pinned-host allocation failed */
    BL_ERR_CAPACITY = -4,    /* output arrays too small: result.count says how many records exist */
    BL_ERR_NO_DEVICE = -5,   /* no gfx950 device visible */
    BL_ERR_INTERNAL = -6,    /* an internal consistency check failed (never expected; results invalid) */
    BL_ERR_IO = -7           /* bl_text_write: the file could not be opened, or a write came back short */
};

enum {
    BL_FLAG_CANONICAL = 1u << 0, /* numeric min(forward, reverse complement), kmer_view.hpp:196 */
    BL_FLAG_DROP_LAST = 1u << 1, /* reproduce the `it != cend()` idiom: the k-mer that ends a sequence is skipped (quirk Q1) */
    BL_FLAG_SYNC = 1u << 2       /* wait for completion and fill `result` before returning */
};

typedef struct bl_ctx bl_ctx;
typedef struct bl_batch bl_batch;

/* Filled asynchronously; read after bl_ctx_sync() (or immediately with BL_FLAG_SYNC).  The struct passed to a scan
 * must stay alive until then (the library writes it during the sync); pass NULL if the digest is not wanted. */
typedef struct bl_result {
    uint64_t count;      /* records found (k-mers / minimizer occurrences / super-k-mers / syncmers) */
    uint64_t xor_value;  /* XOR of the 2-bit packed values of all records */
    uint64_t xor_hash;   /* XOR of their 64-bit hashes */
    uint64_t xor_pos;    /* XOR of their global positions (k-mer scan: wrapping SUM of hashes instead) */
    uint64_t aux;        /* super-k-mers: number of group ends seen (== count when consistent); 128-bit k-mer scans: XOR of the high words */
    int32_t status;      /* BL_OK or BL_ERR_CAPACITY */
    int32_t redone;      /* diagnostic: tiles whose pass 1 could not decide a window on what it looks at (an approximation of the hash's
                          * high dword, or high dwords alone) and were counted a second time on the hashes themselves; the records are the
                          * same either way */
} bl_result;

const char* bl_last_error(void);
int bl_version(void);
int bl_device_count(int* n);

/* ---- contexts ---------------------------------------------------------------------------------- */
int bl_ctx_create(int device, bl_ctx** out);
/* Destroying a context also destroys the batches created on it that are still alive (their handles
 * become invalid). */
int bl_ctx_destroy(bl_ctx* ctx);
/* Borrow the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream): every call of this context is then
 * enqueued on it, in order with the caller's own work.  NULL is a stream like any other here — the legacy default
 * stream, which is what torch's default stream is — so a NULL handle is honoured, not read as "unset".
 * bl_ctx_use_own_streams returns to the context's own (non-blocking) streams, which are NOT ordered with any other
 * stream: device buffers handed to the library must then be complete (synchronise the producing stream first). */
int bl_ctx_set_stream(bl_ctx* ctx, void* hip_stream);
int bl_ctx_use_own_streams(bl_ctx* ctx);
int bl_ctx_sync(bl_ctx* ctx);
/* Execution lanes of a context that runs on its own streams: with n = 2 consecutive asynchronous scans alternate between two
 * streams, staggered so that the record pass of one scan runs beside the hashing pass of the next (+12 % on MI355X).  Scans in
 * flight together must not share output arrays.  n = 1 (default) keeps scans strictly ordered.  Ignored on a borrowed stream. */
/* (Measured on MI355X: a stream of minimizer scans with records runs fastest in ranges of 0.5-1 Gbp — 525-535 Gbp/s with two lanes, 2-2.5 %
 * above ranges of 1.5 Gbp; below 0.3 Gbp the per-scan launches show.  Consecutive scans must not share output arrays: double-buffer them.) */
int bl_ctx_set_lanes(bl_ctx* ctx, int n);

/* ---- batches (device-resident sequences) -------------------------------------------------------- */
/* Copy host sequences to the device.  offsets has n_seqs+1 entries, offsets[0] = 0,
 * offsets[n_seqs] = n_bases; NULL offsets = one sequence. */
int bl_batch_upload(bl_ctx* ctx, const char* bases, uint64_t n_bases, const uint64_t* offsets, uint64_t n_seqs, bl_batch** out);
/* The same for reads of ONE length laid end to end (a shorter last read is kept): no offsets array to build or to check — a
 * batch of 150-bp reads has 7 million of them per gigabase.  Such batches are scanned by the read-tiled kernels. */
int bl_batch_upload_reads(bl_ctx* ctx, const char* bases, uint64_t n_bases, uint64_t read_len, bl_batch** out);
/* Wrap bases already in device memory (16-byte aligned, not copied, must outlive the batch).
 * Sequences are either given by host `offsets` (as above) or, if offsets is NULL and read_len > 0,
 * consecutive slices of read_len bases (a shorter last read is kept); both NULL/0 = one sequence. */
int bl_batch_from_device(bl_ctx* ctx, const void* d_bases, uint64_t n_bases, const uint64_t* offsets, uint64_t n_seqs,
                         uint64_t read_len, bl_batch** out);
/* Generate SURVEY.md §8d synthetic DNA on the device:
 *   base[i] = "ACGT"[(splitmix64(seed + (i>>5)) >> (2*(i&31))) & 3], reads = consecutive read_len slices
 * (read_len = 0: one sequence). */
int bl_batch_synth(bl_ctx* ctx, uint64_t seed, uint64_t n_bases, uint64_t read_len, bl_batch** out);
int bl_batch_destroy(bl_batch* batch);
uint64_t bl_batch_n_bases(const bl_batch* batch);
uint64_t bl_batch_n_seqs(const bl_batch* batch);
const void* bl_batch_device_bases(const bl_batch* batch);
/* A batch that is a PIECE of a longer concatenation (one GPU's part of a contig that was cut across GPUs, SURVEY.md §8e;
 * the reference streams a contig of any length through one view, kmer_view.hpp:46-54): `origin` is the position its base 0 has
 * in the whole.  Every position a scan of this batch reports (d_positions, d_first_pos) and folds into xor_pos is then
 * origin + the position inside the batch, so the records of the pieces concatenate to the records of the whole; the
 * ranges [first, first+n) of the scan calls stay relative to the batch.  Default 0. */
int bl_batch_set_origin(bl_batch* batch, uint64_t origin);
uint64_t bl_batch_origin(const bl_batch* batch);
/* Copy bases [first, first+n) back to the host (synchronous). */
int bl_batch_download(bl_batch* batch, uint64_t first, uint64_t n, char* out);

/* ---- scans ---------------------------------------------------------------------------------------
 * Every scan works on the windows / k-mers whose FIRST base lies in [first, first+n) of the batch
 * (n = 0 means "to the end"); bases beyond the range are read as needed, so the union of the results
 * of consecutive ranges equals the result of one scan over their union.  A range may hold at most
 * 2^31 positions. */

/* k-mers (C2): for every position p in the range, dense arrays indexed by p - first:
 *   d_values[p-first]  2-bit packed (canonical) k-mer, first base in the most significant pair
 *   d_hashes[p-first]  hash64(value, seed) = low 64 bits of MurmurHash3_x64_128 of its 8 raw bytes
 *   d_valid[p-first]   1 if a k-mer starts at p (no break inside, not crossing a sequence end), else 0
 * result: count, xor_value, xor_hash, xor_pos := wrapping sum of hashes.  1 <= k <= 32. */
int bl_scan_kmers(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint64_t seed, uint32_t flags,
                  uint64_t* d_values, uint64_t* d_hashes, uint8_t* d_valid, bl_result* result);

/* k-mers up to k = 64: wrapper::kmer_view<__uint128_t,It> (the reference templates kmer_view on KmerType; its super-k-mer driver
 * uses typedef __uint128_t kmer_t) with hash::hash64::hash<__uint128_t>.  Arrays and result as bl_scan_kmers, except:
 *   d_values[2*(p-first)], d_values[2*(p-first)+1]  the k-mer as a 128-bit integer, LOW word first, then the HIGH word — the
 *                      little-endian object representation of __uint128_t, so d_values is a valid __uint128_t[n]; it must be
 *                      16-byte aligned (BL_ERR_INVALID otherwise).  First base in the most significant occupied pair.
 *   d_hashes[p-first]  hash64(value, seed) = first word of MurmurHash3_x64_128 over those 16 BYTES, whatever k is (sizeof(KmerType)
 *                      in the reference's template), seed truncated to 32 bits.  For k <= 32 the value equals bl_scan_kmers' with a
 *                      high word of 0, but the hash DIFFERS from bl_scan_kmers' hash of 8 bytes — as in the reference, where the
 *                      hash depends on KmerType.
 *   canonical          numeric minimum of the two 128-bit values, the reverse complement taken in 2k bits.  (The reference's own
 *                      reverse-strand update shifts a 64-bit operand by up to 126 bits, kmer_view.hpp:195,223: undefined for
 *                      k >= 33.  This is the intended meaning, its formulas evaluated in KmerType)
 * result: count, xor_value := XOR of the low words, aux := XOR of the high words, xor_hash, xor_pos := wrapping sum of hashes.
 * 1 <= k <= 64 (bl_scan_kmers keeps its own limit of 32).
 * What takes these values on: bl_sort_u128 / bl_sort_unique_u128 / bl_count_sorted_u128 / bl_jaccard_sorted_u128 / bl_partition_u128 and
 * the run-file calls bl_write_run_u128 .. bl_merge_runs_u128 (16-byte keys in this layout); syncmers: bl_scan_syncmers128; window
 * minimizers: bl_scan_minimizers128; super-k-mer records and the exact counter: bl_pack_super_kmers128 .. bl_count_super_kmers128;
 * the count of every position's k-mer in a table of counted k-mers, without writing the values at all: bl_scan_kmer_counts.
 * NOT covered for k > 32: biolib_amd::read_pool. */
int bl_scan_kmers128(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint64_t seed, uint32_t flags,
                     uint64_t* d_values /* 2 per position: lo, hi */, uint64_t* d_hashes, uint8_t* d_valid, bl_result* result);

/* minimizers (C3): hashed unit = (canonical) `unit`-mer, window = w consecutive units inside one
 * sequence and one break-free run, leftmost minimum hash; one record each time the minimizer
 * occurrence changes (or a run begins):
 *   d_values[r] unit value, d_positions[r] global start position of the unit, d_hashes[r] its hash.
 * Range: [first, first+n) takes the windows whose first base lies in it; units behind the range are read as needed, and window
 * first-1 in front of it.  An occurrence belongs to the range in which its FIRST electing window starts: one that window first-1
 * elects too is reported by the range before and not again, so consecutive ranges concatenate exactly to the scan of their union.
 * In biolib's naming this is minimizer_view(k = unit + w - 1, m = unit).  1 <= unit <= 32, 1 <= w <= 64. */
int bl_scan_minimizers(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t unit, uint32_t w, uint64_t seed,
                       uint32_t flags, uint64_t* d_values, uint64_t* d_positions, uint64_t* d_hashes, uint64_t capacity,
                       bl_result* result);

/* hash_sampler over kmer_view (reference hash_sampler.hpp:73-78,136-141): the k-mers whose
 * hash64(value, seed) is BELOW `threshold` (the reference computes threshold = rate * 2^64-1 in double), position-ordered,
 * same arrays as bl_scan_minimizers.  threshold = UINT64_MAX with BL_FLAG_DROP_LAST gives exactly the k-mers the
 * reference idiom visits.  (bl_scan_minimizers with w = 1 is the same list without a threshold.) */
int bl_scan_hash_sample(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint64_t seed, uint64_t threshold,
                        uint32_t flags, uint64_t* d_values, uint64_t* d_positions, uint64_t* d_hashes, uint64_t capacity,
                        bl_result* result);

/* The same sampler over kmer_view<__uint128_t> (1 <= k <= 64): the k-mers of bl_scan_kmers128 whose 16-byte hash is below `threshold`,
 * position-ordered.  d_values holds two words per record (low, high; 16-byte aligned), d_positions and d_hashes one.  Nothing is
 * written at or beyond `capacity`; the result always carries the full count (BL_ERR_CAPACITY when it exceeds capacity).
 * result: count, xor_value := XOR of the low words, aux := XOR of the high words, xor_hash, xor_pos := XOR of the positions. */
int bl_scan_hash_sample128(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint64_t seed, uint64_t threshold,
                           uint32_t flags, uint64_t* d_values /* 2 per record */, uint64_t* d_positions, uint64_t* d_hashes,
                           uint64_t capacity, bl_result* result);

/* window minimizers of k-mers up to k = 64: sampler::minimizer_sampler over kmer_view<__uint128_t> (the reference's
 * minimizer_sampler.hpp does not compile; this is bl_scan_minimizers' contract evaluated in KmerType = __uint128_t).
 *   units     the k-mers of bl_scan_kmers128, 1 <= unit <= 64: the same value, validity and canonical form; a unit's hash is
 *             bl_hash64_u128(lo, hi, seed) — 16 key bytes whatever `unit` is
 *   windows   w consecutive unit start positions p .. p+w-1, 1 <= w <= 64; the window exists iff all w units are valid (hence one
 *             sequence, one break-free run).  Its occurrence is the position of the smallest hash, the LEFTMOST of equal ones
 *   records   window p yields one iff it exists and window p-1 does not exist or has its occurrence at another position:
 *             d_values[2r], d_values[2r+1] the unit (low word, high word; d_values must be 16-byte aligned, else BL_ERR_INVALID),
 *             d_positions[r] the global start of the unit, d_hashes[r] its hash
 *   range     [first, first+n) takes the windows whose first base lies in it; units behind the range are read as needed, and window
 *             first-1 in front of it, so consecutive ranges concatenate exactly to the scan of their union.  n = 0: to the end
 *   BL_FLAG_DROP_LAST  the unit that ends its sequence is no item (as in bl_scan_kmers128) and takes part in no window: what a
 *             kmer_view range [cbegin, cend) gives the sampler (quirk Q1).  bl_scan_minimizers honours the flag for its w = 1 unit
 *             lists only; this call honours it for every w
 *   capacity  nothing is written at or beyond `capacity`; the result always carries the full count (BL_ERR_CAPACITY when it exceeds
 *             capacity).  Any of the three arrays may be NULL; with all three NULL the call only counts
 * result: count, xor_value := XOR of the low words, aux := XOR of the high words, xor_hash, xor_pos := XOR of the positions, redone = 0
 * (the windows are decided on the 64-bit hashes themselves: there is no approximate pass).
 * unit <= 32 through this entry: the values are bl_scan_minimizers' with a zero high word, but the key is 16 bytes instead of 8, so
 * the records differ in general — as the reference's template does between KmerType = uint64_t and __uint128_t.  w = 1 lists every
 * valid unit: bl_scan_hash_sample128 at threshold = UINT64_MAX, short of a unit whose hash is exactly 2^64 - 1.
 * bl_scan_minimizers keeps its limit of 32.  NOT provided: minimizer_view / super_kmer_view with m > 32, read_pool, and a read-tiled or
 * approximate-hash variant of this kernel.  (Super-k-mer records and the counter for k > 32: bl_pack_super_kmers128 ..
 * bl_count_super_kmers128; sort, unique, Jaccard, owner split and run files of the 16-byte units: the bl_*_u128 calls.) */
int bl_scan_minimizers128(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t unit, uint32_t w, uint64_t seed,
                          uint32_t flags, uint64_t* d_values /* 2 per record */, uint64_t* d_positions, uint64_t* d_hashes,
                          uint64_t capacity, bl_result* result);

/* super-k-mers (C4): maximal groups of consecutive k-mers sharing one minimizer occurrence
 * (m-mer, w = k - m + 1):
 *   d_minimizers[r] m-mer value, d_first_pos[r] global position of the group's first k-mer,
 *   d_mm_pos[r] minimizer offset inside that k-mer, d_sizes[r] number of k-mers (<= w),
 *   d_hashes[r] hash of the minimizer.  Any of the arrays may be NULL.
 * Range: [first, first+n) takes the k-mers whose first base lies in it.  A group that straddles an end of the range is CLIPPED to the
 * range: d_first_pos is the first of its k-mers inside the range, d_sizes the number of them inside it, and d_mm_pos the minimizer's
 * offset in that first k-mer (the minimizer's own position, d_first_pos + d_mm_pos, does not change).  The sizes of consecutive ranges
 * therefore sum to the k-mers of their union, and their records are the union's with every straddling group in two pieces. */
int bl_scan_super_kmers(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t m, uint64_t seed,
                        uint32_t flags, uint64_t* d_minimizers, uint64_t* d_first_pos, uint8_t* d_mm_pos, uint8_t* d_sizes,
                        uint64_t* d_hashes, uint64_t capacity, bl_result* result);

/* syncmers (C5): k-mers whose minimum-hash s-mer (leftmost in the canonical k-mer, hash seed `seed`,
 * 0 in the reference) sits at offset start_offset or end_offset:
 *   d_positions[r] global position of the k-mer (may be NULL: count only).
 * result: count, xor_pos. */
int bl_scan_syncmers(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t s, uint32_t start_offset,
                     uint32_t end_offset, uint64_t seed, uint32_t flags, uint64_t* d_positions, uint64_t capacity,
                     bl_result* result);

/* syncmers of k-mers up to k = 64: syncmer_sampler with minimizer_position_extractor over kmer_view<__uint128_t>.
 * 1 <= s <= 32 and s <= k <= 64 (bl_scan_syncmers keeps its own limit of 32), W = k - s + 1 <= 64.
 * The k-mers, their validity and canonical form are bl_scan_kmers128's.  For a valid k-mer of 128-bit value v, s-mer number j from the
 * first base is x_j = (v >> 2(k-s-j)) & (4^s - 1), j = 0 .. W-1; its hash is bl_hash64_u128(x_j, 0, seed) — the reference's
 * `km & mask` is a KmerType value, so the key is 16 bytes with a zero high word (kmer_view.hpp:272-275).  The k-mer is a record iff
 * the smallest j of minimal hash (the leftmost minimum: the `>=` loop of kmer_view.hpp:274-282 runs from the right) equals
 * start_offset or end_offset; an offset >= W matches nothing.
 *   d_positions[r] global position of the k-mer, increasing (may be NULL: count only); nothing is written at or beyond `capacity`,
 *   the result always carries the full count (BL_ERR_CAPACITY when it exceeds capacity).
 * result: count, xor_pos; the other digest words are 0.
 * k <= 32 through this entry: the k-mers are those of the 64-bit call, but the s-mer keys are 16 bytes instead of 8, so the records
 * differ in general from bl_scan_syncmers' — as the reference's template does between KmerType = uint64_t and __uint128_t. */
int bl_scan_syncmers128(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t s, uint32_t start_offset,
                        uint32_t end_offset, uint64_t seed, uint32_t flags, uint64_t* d_positions, uint64_t capacity,
                        bl_result* result);

/* on != 0: every later scan on this context decides its windows on the 64-bit hashes themselves — no pass 1 on the approximate high
 * dword, no closed-syncmer form (§5.4).  Same records, 2-4 % slower; for checks and A/B measurements. */
int bl_ctx_set_exact_windows(bl_ctx* ctx, int on);
/* Tuning and test switches of a context, by name (BL_ERR_INVALID for a name or value it does not know).  None of them changes a result.
 *   "exact_windows"   0 / 1       = bl_ctx_set_exact_windows
 *   "lanes"           1 / 2       = bl_ctx_set_lanes
 *   "position_tiled"  0 / 1       1: batches of fixed-length reads are scanned by the position-tiled kernels too (default 0: read-tiled
 *                                 where that layout applies)
 *   "packed_codes"    0 / 1       1 (default): a batch that owns its bases (upload, synth, the parser, select, apply_edits) keeps a packed
 *                                 copy of them, 2 bits per base and a bit per 16 bases (+0.26 bytes per base), made once when the batch is,
 *                                 and the window scans stage their tiles from it.  0: batches made LATER get none, and scans ignore the copy
 *                                 of a batch that has one.  bl_batch_from_device batches, whose memory is the caller's,
 *                                 never get one
 *   "direct_codes"    0 / 1       1 (default): the read-tiled pass 1 of a batch with a packed copy does not stage a tile that holds no bad
 *                                 chunk; its lanes read their codes from the copy.  0: every tile is staged in LDS
 *   "emit_lds_bytes"  0 or bytes  two-lane contexts: LDS footprint the record pass's workgroups are padded to, which caps how many of
 *                                 them a CU holds beside the next scan's hashing pass (0: the built-in default per scan kind)
 *   "count128_tables" 0 / 1       0: bl_count_super_kmers128 counts every bucket by expand + sort + run-length instead of the LDS tables
 *                                 (default 1)
 *   "jaccard128_path" 0 / 1 / 2   which kernel bl_jaccard_sorted_u128 runs: 1 the merge kernel, 2 the search kernel, 0 (default) the
 *                                 merge kernel when the larger set is less than 4 times the smaller one
 *   "table_prefix_bits" -1 / 0..24  the width P of the prefix index of tables built LATER (bl_table_build_*): -1 (default) the library
 *                                 chooses from the number of distinct keys, 0 .. 24 forces it, clamped to the table's key_bits
 *                                 
 * The library reads no environment variable on the scan path. */
int bl_ctx_set_option(bl_ctx* ctx, const char* name, int64_t value);
/* Which kernels ran.  The window scans (bl_scan_minimizers, bl_scan_hash_sample, bl_scan_super_kmers, bl_scan_super_kmer_records,
 * bl_scan_super_kmer_records128, bl_scan_syncmers) choose among about a hundred kernel instantiations by mode, window width, unit length,
 * strand flag, batch layout, syncmer offsets and the exact_windows switch.  Every launch records a short stable name, e.g.
 * "count<MM,W=7>" (pass 1), "frl<MM,W=11,NS=15,U=31,L=150,approx>" followed by "frl_redo<MM,W=11,NS=15,U=31,L=150>" (read-tiled pass 1
 * on the approximate dword and its second run), "emit<SK,wide>" (pass 2).  bl_ctx_last_scan_kernels copies the names of the most recent
 * window scan issued on the context, in launch order, one per line, NUL-terminated, into buf; bl_scan_kernel_names copies every name a
 * launch can record.  *needed (nullable) takes the bytes required; BL_ERR_CAPACITY, with nothing written, when capacity is smaller.
 * For tests and diagnostics: a call that scanned nothing (an empty range) recorded nothing.  Neither call synchronises. */
int bl_ctx_last_scan_kernels(bl_ctx* ctx, char* buf, uint64_t capacity, uint64_t* needed);
int bl_scan_kernel_names(char* buf, uint64_t capacity, uint64_t* needed);

/* Elapsed GPU time of the most recent scan call on this context, from HIP events recorded on the
 * context's stream around its kernels (milliseconds).  Synchronises. */
int bl_ctx_last_scan_ms(bl_ctx* ctx, float* ms);
/* Per-launch timing of the main scan kernel alone: after bl_ctx_kernel_timing(ctx, 1) every scan
 * brackets its tile kernel with a HIP event pair on the context's stream; bl_ctx_kernel_time
 * synchronises and returns the summed kernel time and the number of launches since timing was
 * switched on (switching it on or off resets both).  bl_scan_read_steps brackets its node pass in the same way: one launch per call. */
int bl_ctx_kernel_timing(bl_ctx* ctx, int enable);
int bl_ctx_kernel_time(bl_ctx* ctx, double* total_ms, uint64_t* launches);
/* Markers on the device's timeline that do not stop it.  bl_ctx_mark enqueues one behind everything issued so far on the
 * context's stream(s); bl_ctx_mark_times synchronises, returns for each marker the milliseconds after marker 0 was reached at
 * which the work in front of it had finished (with two lanes: on both), and forgets the markers.  A benchmark times its steps
 * with them: a bl_ctx_sync between steps would cost the overlap of one step's last record pass with the next step's first scan.
 * At most 4,096 markers may be outstanding (BL_ERR_CAPACITY from bl_ctx_mark beyond that).  bl_ctx_mark_times with a capacity
 * below the number of markers returns that number in *n_marks and keeps them: BL_OK for capacity 0 (a size query), BL_ERR_CAPACITY otherwise. */
int bl_ctx_mark(bl_ctx* ctx);
int bl_ctx_mark_times(bl_ctx* ctx, double* ms, uint32_t capacity, uint32_t* n_marks);

/* ---- ingest: FASTA / FASTQ, plain or gzip -> batches -----------------------------
 * Record semantics are those of the reader biolib's own tools use (reference tests/kseq.h:185-234): a record
 * starts at '>' or '@'; the name ends at the first whitespace; sequence lines are concatenated, empty lines and a
 * line-final '\r' dropped; FASTQ quality must match the sequence length.  Bases are not altered: the scans treat
 * everything but ACGTUacgtu as a break, exactly as the reference table does (constants.hpp:12-21). */
typedef struct bl_reader bl_reader;
/* The file is decompressed by background threads that run ahead of the parser: BGZF (bgzip) members are inflated in parallel
 * by `threads` workers (0 = one per core, at most 16); any other gzip file by the same number of workers that each decode a
 * part of the ONE deflate stream from a block start they find by themselves, without the 32 KiB of text before it, which is
 * filled in when the part before is done (pipes and files of a few MiB: one zlib thread); plain files are read ahead. */
int bl_reader_open(const char* path, bl_reader** out);
int bl_reader_open_threads(const char* path, int threads, bl_reader** out);
/* One part of a file, for several readers (GPUs, ranks) that take one file between them.  A PLAIN text file: part `rank` is the
 * byte range from the first record start that can be recognised in the text behind byte size / world * rank (a line that opens a
 * record, a newline in front of it) to the next part's; every call of the reader works on such a part.  A BGZF file: part `rank` holds the
 * members from the first member boundary at or behind byte size / world * rank to the next part's, and delivers the records that
 * BEGIN in its text — from the first record start that can be recognised there (a line that opens a record, a newline in front of
 * it inside the part's text) to the place where the next part's reader finds its own, found by inflating into the next part.
 * The parts' records, in rank order, are the file's records; the readers do not talk to each other.
 * RESTRICTION: a FASTQ record start is recognised as a line that opens with '@' and whose second-next line opens with '+', i.e.
 * FOUR-LINE FASTQ (one sequence line, one quality line per record: what sequencers and every current tool write).  Multi-line
 * FASTQ — which the whole-file readers accept, as kseq does — must be read with world = 1: in parts, its boundaries may not be
 * found (records then fall to an earlier part) or, rarely, a quality line may be taken for a header.  FASTA has no such limit.
 * Device batches only
 * (bl_reader_next_batch_device) from a BGZF part.  BL_ERR_INVALID for a gzip file that is not BGZF (one stream, no entry points).  This is how north_star's "shard by read" reaches the
 * file: the reference's drivers read one file per process (tests/test_kmer_view.cpp:23-42). */
int bl_reader_open_shard(const char* path, uint32_t rank, uint32_t world, bl_reader** out);
/* the bytes of the file whose members are the reader's own: [first_byte, end_byte), end_byte = UINT64_MAX for the last part
 * (0 / UINT64_MAX for a reader of the whole file) */
int bl_reader_shard_range(bl_reader* reader, uint64_t* first_byte, uint64_t* end_byte);
int bl_reader_close(bl_reader* reader);
/* "plain", "gzip" or "bgzf": how the file is being read */
const char* bl_reader_kind(bl_reader* reader);
/* Host only: next record.  Returns BL_OK, 1 at end of file, or an error.  Pointers stay valid until the next call. */
int bl_reader_next_record(bl_reader* reader, const char** name, const char** seq, uint64_t* seq_len);
/* Next batch of whole records holding at most max_bases bases (0 = the rest of the file; always at least one
 * record), uploaded to the device.  At end of file *out is NULL and *n_seqs is 0.  A thread of the reader parses the following
 * batch meanwhile; max_bases is fixed by the first call (BL_ERR_INVALID if a later call differs), and single records
 * (bl_reader_next_record) cannot be mixed with batches on one reader. */
int bl_reader_next_batch(bl_ctx* ctx, bl_reader* reader, uint64_t max_bases, bl_batch** out, uint64_t* n_seqs, uint64_t* n_bases);
/* The high-throughput path for regular files: the decompressed TEXT, cut at record boundaries (4-line FASTQ: in front of a header
 * line, recognised by the '+' line two lines on; FASTA: before a line-initial '>'), goes to the device-side parser
 * (bl_batch_from_text) — parallel inflate, one H2D copy, parsing on the GPU.  A thread of the reader assembles the next spans
 * while the caller works on the current one, in buffers that live with the reader (page-locked for bl_reader_next_batch_device).
 * bl_reader_next_text hands out the next span of at most max_bytes (0 = 64 MiB; a longer single record is not split), valid
 * until the next call, 1 at end of file; max_bytes is fixed by the first call (BL_ERR_INVALID if a later call differs).
 * bl_reader_next_batch_device parses the span on the device (names are not kept; *out NULL at end of file; BL_ERR_INVALID for
 * layouts the device parser refuses — reopen and use the record calls).  Records and spans cannot be mixed on one reader. */
int bl_reader_next_text(bl_reader* reader, uint64_t max_bytes, const char** text, uint64_t* n_bytes);
int bl_reader_next_batch_device(bl_ctx* ctx, bl_reader* reader, uint64_t max_text_bytes, bl_batch** out, uint64_t* n_seqs, uint64_t* n_bases);
/* Host copy of the batch produced last: concatenated bases, offsets[n_seqs+1], names. */
int bl_reader_last_batch(bl_reader* reader, const char** bases, const uint64_t** offsets, uint64_t* n_seqs);
const char* bl_reader_last_name(bl_reader* reader, uint64_t i);

/* ---- set operations on k-mer lists (the consumer in reference tests/test_jaccard.cpp:55-130) ---
 * bl_sort_unique_u64: sorts d_keys[0..n) in place and removes duplicates (ordered_unique_sampler.hpp:115-130 over a
 * sorted vector); *n_unique = number of distinct keys now at the front.  Synchronous.
 * bl_jaccard_sorted_u64: |A n B| and |A u B| of two sorted duplicate-free device arrays (jaccard.hpp:8-37). */
int bl_sort_unique_u64(bl_ctx* ctx, uint64_t* d_keys, uint64_t n, uint64_t* n_unique);
int bl_jaccard_sorted_u64(bl_ctx* ctx, const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* intersection,
                          uint64_t* union_size);

/* ---- multi-GPU k-mer counting pieces ------------------------------------------------------
 * bl_partition_u64: reorder keys into `parts` (<= 64) buckets by hash64(key, seed) % parts — the owner rank of a
 *   k-mer in a partitioned count; counts[b] (host) = size of bucket b, buckets are contiguous in d_out in bucket order.
 * bl_sort_u64: in-place ascending sort (duplicates kept).  bl_count_sorted_u64: run-length count of a sorted list.
 * The exchange between the two (all-to-all over RCCL / xGMI) is biolib_amd/shard.py:exchange_and_count. */
int bl_partition_u64(bl_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t parts, uint64_t seed, uint64_t* d_out, uint64_t* counts);
int bl_sort_u64(bl_ctx* ctx, uint64_t* d_keys, uint64_t n);
int bl_count_sorted_u64(bl_ctx* ctx, const uint64_t* d_sorted, uint64_t n, uint64_t* d_unique, uint32_t* d_counts, uint64_t* n_unique);

/* ---- the same set operations on 16-byte keys: k-mers of kmer_view<__uint128_t> (k up to 64) -----------------------------------------
 * What the reference's Jaccard tool does after `typedef __uint128_t kmer_t;` (tests/test_jaccard.cpp): sort, unique, intersection.
 * KEY LAYOUT  16 bytes per key: the LOW word, then the HIGH word — the object representation of __uint128_t, what bl_scan_kmers128,
 *             bl_scan_hash_sample128 and bl_expand_super_kmers128 write; an array of n keys is a valid __uint128_t[n].
 * ORDER       the numeric order of the 128-bit value: the high word decides, then the low word, both unsigned.
 * ALIGNMENT   every key array must be 16-byte aligned (BL_ERR_INVALID otherwise).
 * n = 0 succeeds and touches nothing.  Temporaries come from the context's scratch; the calls are synchronous.
 * bl_sort_u128: ascending, in place, duplicates kept.  key_bits (1 .. 128) is the number of low bits that can be non-zero — 2k for
 *   k-mers; the caller promises that the bits above are zero and the radix sort runs over [0, key_bits) only.  128 is always valid.
 * bl_sort_unique_u128: sort + remove duplicates; *n_unique distinct keys are at the front afterwards.
 * bl_count_sorted_u128: run-length count of a sorted list (n < 2^32): distinct keys, their multiplicities, their number.
 * bl_jaccard_sorted_u128: |A n B| and |A u B| of two sorted duplicate-free arrays.  With duplicates in an input the two numbers are
 *   unspecified, but no access leaves the arrays.  Two kernels: a merge-path kernel that streams both sets once (sets of comparable
 *   size) and a binary-search kernel (sets of very different size); the option "jaccard128_path" of bl_ctx_set_option forces one.
 * bl_partition_u128: bl_partition_u64's contract with bucket = bl_hash64_u128(lo, hi, seed) % parts, 1 <= parts <= 64; d_out takes
 *   n keys, counts[b] (host) = size of bucket b. */
int bl_sort_u128(bl_ctx* ctx, uint64_t* d_keys /* 2 per key: lo, hi */, uint64_t n, uint32_t key_bits);
int bl_sort_unique_u128(bl_ctx* ctx, uint64_t* d_keys, uint64_t n, uint32_t key_bits, uint64_t* n_unique);
int bl_count_sorted_u128(bl_ctx* ctx, const uint64_t* d_sorted, uint64_t n, uint64_t* d_unique, uint32_t* d_counts, uint64_t* n_unique);
int bl_jaccard_sorted_u128(bl_ctx* ctx, const uint64_t* d_a, uint64_t na, const uint64_t* d_b, uint64_t nb, uint64_t* intersection,
                           uint64_t* union_size);
int bl_partition_u128(bl_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t parts, uint64_t seed, uint64_t* d_out, uint64_t* counts);

/* ---- the count table: what consumes (key, multiplicity) arrays ------------------------------------------------------------------------
 * bl_count_super_kmers, bl_count_super_kmers128, bl_count_sorted_u64 / _u128 return distinct k-mers with their multiplicities (the
 * super-k-mer counters in no particular order).  A bl_table holds such a list so that it can be asked: the count of any key
 * (bl_table_lookup_*), the count of every k-mer of a batch (bl_scan_kmer_counts), the spectrum (bl_table_histogram).  The object is
 * opaque, owned by the library and tied to the context it was built on (every call that takes a context and a table refuses a table of
 * another context); destroy it with bl_table_destroy — before or after its context, but not while a scan that reads it is in flight.
 *
 * bl_table_build_u64 / _u128: n keys of one word, or of two words (low, high: the KEY LAYOUT and ALIGNMENT above), in ANY order, with
 *   duplicates allowed — the outputs of several counting calls can be concatenated.  Equal keys are merged and their counts added,
 *   saturating at 2^32 - 1.  d_counts == NULL: every entry counts 1 (a membership set; the multiplicities of a raw key list).  The
 *   table copies what it needs: the caller's arrays are not modified and may be freed afterwards.  key_bits is the number of low bits
 *   that can be non-zero (1 .. 64, 1 .. 128; 2k for k-mers, as in bl_sort_u128); the build checks the promise with an OR over all keys:
 *   a key with a bit at or above key_bits gives BL_ERR_INVALID.  n = 0 builds an empty table in which every lookup answers 0.
 *   n >= 2^32 and a misaligned 128-bit array give BL_ERR_INVALID.  Synchronous; temporaries from the context's scratch, as the set
 *   operations.
 * STORAGE  sorted distinct keys (128-bit ORDER as above), uint32_t counts, and a prefix index of 2^P + 1 uint32_t words: index[j] is
 *   the first slot whose key has key >> (key_bits - P) >= j.  A search reads two neighbouring index words and bisects only between
 *   them.  No answer depends on P.  The library chooses P from the number of distinct keys, 0 <= P <= min(key_bits, 24);
 *   bl_ctx_set_option(ctx, "table_prefix_bits", v) forces it for later builds.
 * bl_table_info: the number of distinct keys, words per key (1 or 2), key_bits and P (any pointer may be NULL).
 * bl_table_arrays: the table's own sorted keys (n_distinct * key_words words) and counts, device pointers valid until bl_table_destroy
 *   (NULL for an empty table).
 * bl_table_lookup_u64 / _u128: d_counts_out[i] = the stored count of d_queries[i], 0 if the key is not in the table.  Queries may come in
 *   any order and may repeat; a query with a bit at or above the table's key_bits is absent.  The width must match the table
 *   (BL_ERR_INVALID otherwise).  Synchronous; n = 0 touches nothing.
 * bl_table_histogram: hist[c] (HOST, n_bins words) = the number of distinct keys with count c for c < n_bins - 1, hist[n_bins - 1] =
 *   those with count >= n_bins - 1.  1 <= n_bins <= 65536.  Synchronous. */
typedef struct bl_table bl_table;
int bl_table_build_u64(bl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_counts, uint64_t n, uint32_t key_bits, bl_table** out);
int bl_table_build_u128(bl_ctx* ctx, const uint64_t* d_keys /* 2 per key: lo, hi */, const uint32_t* d_counts, uint64_t n, uint32_t key_bits,
                        bl_table** out);
int bl_table_destroy(bl_table* table);
int bl_table_info(const bl_table* table, uint64_t* n_distinct, uint32_t* key_words, uint32_t* key_bits, uint32_t* prefix_bits);
int bl_table_arrays(const bl_table* table, const uint64_t** d_keys, const uint32_t** d_counts);
int bl_table_lookup_u64(bl_ctx* ctx, const bl_table* table, const uint64_t* d_queries, uint64_t n, uint32_t* d_counts_out);
int bl_table_lookup_u128(bl_ctx* ctx, const bl_table* table, const uint64_t* d_queries /* 2 per key */, uint64_t n, uint32_t* d_counts_out);
int bl_table_histogram(bl_ctx* ctx, const bl_table* table, uint64_t* hist, uint32_t n_bins);

/* Table algebra: a new table from two tables A and B of the same context, key_words and key_bits (the kmc_tools simple operations), in
 * one linear merge of the two sorted arrays — no sort, no rebuild.  For a key x with stored count a in A and b in B:
 *   BL_TABLE_UNION           x in A or B; c = f(a, b) where both hold it, else the count of the table that holds it
 *   BL_TABLE_INTERSECT       x in both; c = f(a, b)
 *   BL_TABLE_SUBTRACT        x in A and not in B; c = a
 *   BL_TABLE_COUNT_SUBTRACT  x in A and a > b, with b = 0 where B lacks x; c = a - b
 * f is count_mode: BL_COUNT_SUM (saturating at 2^32 - 1, as the build), _MIN, _MAX, _LEFT (a) or _RIGHT (b); the two subtractions take
 * BL_COUNT_LEFT only.  After the op a key is kept iff count_lo <= c <= count_hi ((0, UINT32_MAX): all).  b == NULL is the empty table;
 * a == b is legal.  The inputs are not modified.  *out is an ordinary table (sorted distinct keys, exact-size arrays, a prefix index
 * chosen under the current "table_prefix_bits"): every bl_table_* call and both scans take it; an empty result is the n = 0 table.
 * Results are bit-reproducible.
 * stats (nullable) — everything but n_out and sum_out is independent of op, mode and bounds:
 *   n_a_only, n_b_only, n_both   |A \ B|, |B \ A|, |A n B|: Jaccard = n_both / (n_a_only + n_b_only + n_both)
 *   sum_min                      sum of min(a, b) over the common keys   }  wrapping 64-bit sums;
 *   sum_max                      sum of max(a, b) over the union, an absent count being 0   }  weighted Jaccard = sum_min / sum_max
 *   n_out, sum_out               the size of the result and the sum of its counts
 * out == NULL: only the counting pass runs, nothing is allocated (a comparison of two tables).
 * BL_ERR_INVALID with a message: NULL ctx or a, a table of another context, tables of different key_words or key_bits, an unknown op or
 * mode, a mode the op does not take, count_lo > count_hi.  BL_ERR_CAPACITY: the result would have 2^32 entries or more (stats filled,
 * nothing allocated).  Synchronous; temporaries from the context's scratch, as the set operations.
 * bl_table_filter(ctx, a, lo, hi, out) is bl_table_combine(ctx, a, NULL, BL_TABLE_UNION, BL_COUNT_LEFT, lo, hi, out, NULL): the solid
 * table (lo = 2) or a table without its repeat tail (hi). */
enum { BL_TABLE_UNION = 0, BL_TABLE_INTERSECT = 1, BL_TABLE_SUBTRACT = 2, BL_TABLE_COUNT_SUBTRACT = 3 };
enum { BL_COUNT_SUM = 0, BL_COUNT_MIN = 1, BL_COUNT_MAX = 2, BL_COUNT_LEFT = 3, BL_COUNT_RIGHT = 4 };
typedef struct {
    uint64_t n_a_only, n_b_only, n_both, n_out, sum_min, sum_max, sum_out, reserved;
} bl_table_stats;
int bl_table_combine(bl_ctx* ctx, const bl_table* a, const bl_table* b /* NULL = empty */, uint32_t op, uint32_t count_mode, uint32_t count_lo,
                     uint32_t count_hi, bl_table** out /* NULL = stats only */, bl_table_stats* stats /* nullable */);
int bl_table_filter(bl_ctx* ctx, const bl_table* a, uint32_t count_lo, uint32_t count_hi, bl_table** out);

/* The fused scan: the table's count of the k-mer at every position of a range, without the k-mers ever being written.
 * The k-mers, their validity, the canonical form, BL_FLAG_DROP_LAST and the range rules (at most 2^31 positions, n = 0: to the end,
 * consecutive ranges concatenate) are exactly bl_scan_kmers128's; no hash is computed.  1 <= k <= 64; a table of one-word keys takes
 * k <= 32 (the high word is 0); 2k <= the table's key_bits, otherwise BL_ERR_INVALID with a message.
 *   d_counts[p-first]  the table's count of the k-mer at p; 0 where no k-mer starts or the key is absent.  Every position of the range
 *                      is written.  NULL: digest only
 *   d_valid[p-first]   as bl_scan_kmers128 (may be NULL)
 * result: count := valid k-mers in the range, xor_value := XOR of their low words, aux := XOR of their high words (all three as
 * bl_scan_kmers128), and — the two hash words have no hash to carry here and are REUSED, both as sums —
 *   xor_hash := the NUMBER of valid k-mers whose key is in the table, xor_pos := the wrapping SUM of the counts looked up; redone = 0.
 * Asynchronous like every scan (BL_FLAG_SYNC applies): the table must stay alive until the sync. */
int bl_scan_kmer_counts(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, const bl_table* table,
                        uint32_t* d_counts, uint8_t* d_valid, bl_result* result);

/* The same scan reduced per sequence on the chip: one 48-byte record per read instead of five bytes per base.  The k-mers, their
 * validity, the canonical form, BL_FLAG_DROP_LAST, 1 <= k <= 64, the table rules, the range rules and the asynchrony are exactly
 * bl_scan_kmer_counts's, and `result` is word for word what that call returns for the same arguments.
 *   min_count   >= 1 (0: BL_ERR_INVALID): a k-mer is solid if its count >= min_count, weak otherwise (an absent key counts 0)
 *   d_offsets   DEVICE copy of the n_seqs + 1 offsets the batch was made from: the sequence of position p is the last one whose offset
 *               is <= p.  May be NULL for a single-sequence batch and for a fixed-read-length batch (sequence = p / read_len); NULL on
 *               any other batch is BL_ERR_INVALID.  The array is trusted for content, not for safety: every search in it stays inside
 *               [0, n_seqs], so a wrong array gives wrong statistics but no access outside d_offsets or d_records.
 *   d_records   bl_batch_n_seqs(batch) records, indexed by sequence, 16-byte aligned (NULL or misaligned: BL_ERR_INVALID)
 * The call touches only the records of the sequences from the one that holds `first` to the one that holds the range's last position,
 * empty sequences between them included (they keep the identity record); no other record is written.
 *   BL_READ_COUNTS_INIT        the touched records are first set to the identity — zeros, min_count 0xFFFFFFFF, weak_begin
 *                              UINT64_MAX, weak_end 0 — and then filled
 *   BL_READ_COUNTS_ACCUMULATE  they are merged into as they stand: ranges that cut a read anywhere add up to the whole-batch answer
 * An empty range succeeds and writes nothing.  The records are integer sums, minima and maxima: bit-reproducible. */
typedef struct bl_read_counts {
    uint32_t n_kmers;    /* valid k-mers of the read inside the range */
    uint32_t n_found;    /* ... whose key is in the table (a stored count of 0 is found) */
    uint32_t n_solid;    /* ... whose count >= min_count */
    uint32_t min_count;  /* smallest count over the valid k-mers (absent = 0); 0xFFFFFFFF if n_kmers == 0 */
    uint32_t max_count;  /* largest; 0 if n_kmers == 0 */
    uint32_t reserved;   /* 0 */
    uint64_t sum_counts; /* exact sum of the counts */
    uint64_t weak_begin; /* read-relative position of the first valid k-mer with count < min_count; UINT64_MAX if none */
    uint64_t weak_end;   /* 1 + read-relative position of the last such k-mer; 0 if none */
} bl_read_counts;
enum { BL_READ_COUNTS_INIT = 0, BL_READ_COUNTS_ACCUMULATE = 1 };
int bl_scan_read_counts(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, const bl_table* table,
                        uint32_t min_count, const uint64_t* d_offsets, uint32_t mode, bl_read_counts* d_records, bl_result* result);

/* Per-sequence quantiles of the k-mer counts — the median k-mer abundance of a read among them — by exact selection on the device.
 * The one per-read statistic that is not associative and so cannot ride the scan: it is taken from the arrays bl_scan_kmer_counts wrote.
 *   d_counts[p-first], d_valid[p-first]   what bl_scan_kmer_counts wrote for the range [first, first + n); both required, at any
 *               element alignment.  The range rules are that call's (n = 0: to the end, at most 2^31 positions).  The call knows nothing
 *               of k, strand, BL_FLAG_DROP_LAST or the table: a position takes part iff d_valid is non-zero.
 *   d_offsets   as bl_scan_read_counts: the device copy of the n_seqs + 1 offsets; NULL for a single-sequence or fixed-read-length
 *               batch, BL_ERR_INVALID on any other.  Trusted for content, not for safety: whatever it holds, no access leaves
 *               d_counts, d_valid, d_offsets, d_quantiles or d_n_kmers.
 *   q_num, q_den   HOST arrays of n_q quantiles q_num[j] / q_den[j]; 1 <= n_q <= 4, q_den >= 1, q_num <= q_den
 *   d_quantiles    bl_batch_n_seqs(batch) rows of n_q words, indexed by sequence
 *   d_n_kmers      bl_batch_n_seqs(batch) words (may be NULL)
 * For a sequence with m valid positions, their counts sorted ascending as unsigned 32-bit words (an absent key counts 0):
 *   d_quantiles[seq * n_q + j] = sorted[min(m - 1, floor(m * q_num[j] / q_den[j]))]   (the product in 64 bits), 0 where m = 0
 *   d_n_kmers[seq] = m
 * so (1, 2) is the median sorted[m / 2], (0, 1) the minimum and (1, 1) the maximum.
 * A sequence is written iff it lies whole inside the range: first <= offsets[i] and offsets[i + 1] <= first + n, empty sequences by
 * the same rule.  A sequence cut by either end of the range is not touched: a median does not add up across ranges.
 * The call first waits for the context's scans in flight (a preceding bl_scan_kmer_counts needs no BL_FLAG_SYNC) and returns when the
 * results are written.  They are exact: bit-reproducible.  An empty range succeeds and writes nothing.
 * One wave selects inside a sequence of up to 1,024 positions, one workgroup inside a longer one: a whole chromosome as ONE sequence
 * is correct but served by a single workgroup. */
int bl_select_read_counts(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, const uint32_t* d_counts, const uint8_t* d_valid,
                          const uint64_t* d_offsets, const uint32_t* q_num, const uint32_t* q_den, uint32_t n_q, uint32_t* d_quantiles,
                          uint32_t* d_n_kmers);

/* Select and trim reads on the device: a NEW batch whose sequences are per-read spans of `batch` — whole-read filtering, trimming at a
 * weak k-mer, coverage binning — at copy speed, without the bases or an index of them leaving the device.  The result is an ordinary
 * batch of the same context for every scan; the source batch is not modified.
 *   d_offsets   as bl_scan_read_counts: the device copy of the source's n_seqs + 1 offsets; NULL for a single-sequence or a
 *               fixed-read-length batch, BL_ERR_INVALID on any other
 *   d_spans     bl_batch_n_seqs(batch) pairs, d_spans[2i] = begin, d_spans[2i+1] = end, read-relative; required and 16-byte aligned
 *               (BL_ERR_INVALID otherwise).  With L the read's length the span is [min(begin, L), min(end, L)), empty when that end <=
 *               that begin.  A read with an empty span is dropped.
 *   flags       BL_SELECT_KEEP_EMPTY: a dropped read stays in the result as an empty sequence, so that the result has the source's
 *               n_seqs and sequence i of the result is read i of the source (mates of paired reads stay aligned).  Without it the kept
 *               reads are compacted in source order.  Any other bit: BL_ERR_INVALID.
 *   *out        a batch the library owns (bl_batch_destroy): the kept spans concatenated, every byte copied verbatim (non-ACGT bytes, 0
 *               and 255 included), origin 0.  It is a fixed-length batch where it holds more than one sequence and all are equally
 *               long (the text parser's rule: whole-read filtering of 150-bp reads stays on the read-tiled kernels); otherwise it
 *               carries start bits built from the new offsets.  With every read dropped it is a valid batch of 0 bases: 0 sequences,
 *               or n_seqs empty ones under BL_SELECT_KEEP_EMPTY.
 *   d_out_offsets    (nullable) takes the result's n_seqs_out + 1 offsets; room for the SOURCE's n_seqs + 1 entries
 *   d_source_index   (nullable) takes n_seqs_out entries, the source sequence of every result sequence (the identity under
 *                    BL_SELECT_KEEP_EMPTY); room for the source's n_seqs entries.  The hook for names and qualities: bl_batch_format takes
 *                    it with the index of the source's text, or the host keeps them.
 *   n_seqs_out, n_bases_out   (nullable) host words
 * Synchronous (the total is needed on the host to allocate); the call first waits for the context's scans in flight, so spans made by
 * bl_read_spans behind a bl_scan_read_counts need no sync.  Temporaries come from the context's scratch.
 * Offsets and spans are trusted for content, not for safety: every offset is clamped to [0, n_bases] and offsets[i + 1] < offsets[i]
 * is a read of length 0, so whatever the two arrays hold, no access leaves the batch's bases [0, n_bases), d_offsets[0 .. n_seqs],
 * d_spans or the outputs.  No byte at or behind n_bases of the source is read (a bl_batch_from_device batch has no slack).
 * BL_ERR_INVALID with a message, nothing launched: NULL ctx, batch, out or d_spans, a batch of another context, misaligned d_spans,
 * unknown flag bits. */
enum { BL_SELECT_KEEP_EMPTY = 1u << 0 };
int bl_batch_select(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const uint64_t* d_spans, uint32_t flags,
                    bl_batch** out, uint64_t* d_out_offsets, uint64_t* d_source_index, uint64_t* n_seqs_out, uint64_t* n_bases_out);

/* The decision step in front of bl_batch_select: one span per read from the WHOLE-read records of bl_scan_read_counts (a scan of the
 * whole batch with the same k).  L is the read's length; a read has no weak k-mer when weak_begin == UINT64_MAX.
 *   no weak k-mer, or BL_TRIM_NONE   [0, L)
 *   BL_TRIM_PREFIX                   [0, min(L, weak_begin + k - 1)): khmer's cut — all of the first weak k-mer except its last base
 *   BL_TRIM_SUFFIX                   [min(L, weak_end), L): the mirror image
 *   BL_TRIM_LONGER                   the longer of the two, PREFIX on a tie
 * The span is (0, 0) where it is shorter than min_len or a keep condition fails: n_kmers < min_kmers, the solid fraction outside
 * [solid_min, solid_max], or (with d_stat) d_stat[i] outside [stat_lo, stat_hi].  d_stat is any per-read 32-bit word, e.g. a column
 * of bl_select_read_counts's quantiles (n_q = 1) for coverage binning by median.
 * d_offsets as above; d_records and d_spans 16-byte aligned, bl_batch_n_seqs(batch) entries each.  Asynchronous on the context's
 * stream, like the scans.  BL_ERR_INVALID for a NULL or misaligned argument, a bad trim, k, fraction or reserved. */
enum { BL_TRIM_NONE = 0, BL_TRIM_PREFIX = 1, BL_TRIM_SUFFIX = 2, BL_TRIM_LONGER = 3 };
typedef struct bl_span_rule {
    uint32_t trim, k;     /* k of the scan that made the records, 1..64 */
    uint64_t min_len;     /* a span shorter than this becomes empty */
    uint32_t min_kmers;   /* n_kmers below this: empty */
    uint32_t solid_min_num, solid_min_den, solid_max_num, solid_max_den; /* keep iff n_solid*min_den >= n_kmers*min_num and
                             n_solid*max_den <= n_kmers*max_num, products in 64 bits; den >= 1, num <= den; (0,1) and (1,1): no condition */
    uint32_t stat_lo, stat_hi; /* with d_stat: keep iff stat_lo <= d_stat[i] <= stat_hi */
    uint32_t reserved;    /* 0 */
} bl_span_rule;
int bl_read_spans(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const bl_read_counts* d_records, const uint32_t* d_stat /* nullable */,
                  const bl_span_rule* rule, uint64_t* d_spans);

/* Correct substitution errors from a count table: the chain's repair step (Quake, Musket, BFC and Lighter use a k-mer spectrum this
 * way).  bl_scan_read_edits finds the edits, bl_batch_apply_edits makes the corrected batch, an ordinary batch for every scan.
 *
 * The rule.  A read of L bases has n = L - k + 1 k-mer positions j = 0 .. n - 1 (none if L < k).  Validity and the canonical form are
 * exactly bl_scan_kmer_counts's under the same BL_FLAG_CANONICAL.  A position is INVALID (no valid k-mer starts there), SOLID (valid,
 * table count >= min_count) or WEAK (valid, count < min_count; an absent key counts 0).  A weak run is a maximal interval [a, b] of
 * consecutive WEAK positions of one read; runs never cross reads.  A substitution at read-relative base p touches exactly the k-mers
 * max(0, p - k + 1) .. min(p, n - 1).  Every run is counted under the first of these classes that applies:
 *   1 shape      left-anchored: a >= 1 and state[a - 1] SOLID; then p = a + k - 1 and the run fits iff b = min(p, n - 1).
 *                right-anchored: not left-anchored, b <= n - 2 and state[b + 1] SOLID; then p = b and the run fits iff
 *                a = max(0, b - k + 1).  An unanchored run or one of the wrong length is a MISFIT (two errors closer than k are).
 *   2 support    b - a + 1 < min_support: LOW SUPPORT.  1 <= min_support <= k; 1 is no condition.
 *   3 alternatives   for each of the three other 2-bit codes c: the k-mers a .. b with the code at p replaced by c, made canonical as
 *                the scan does; c qualifies iff every one of them is SOLID.
 *   4 decision   exactly one qualifying c: an EDIT; none: NO BASE; two or three: AMBIGUOUS, no edit.
 * An edit replaces the byte at p by "ACGT"[c] with the original byte's 0x20 (case) bit (U and T share a code, so a U is
 * only ever replaced by A, C or G, and U is never written).
 * Consequence: the edit at p touches exactly the k-mers a .. b of its own run, so the edits of different runs are independent.  After
 * all edits of a batch are applied every k-mer of a corrected run is SOLID, and every other position of the batch keeps its state and
 * its count.  Not attempted: insertions and deletions, two errors within k of each other, ties broken by counts, qualities.
 *
 * bl_scan_read_edits judges the weak runs whose FIRST position a lies in [first, first + n) (n = 0: to the end; at most 2^31
 * positions).  It reads states and bases in front of and behind the range as needed, so the edits of consecutive ranges concatenate
 * and their stats add up exactly to those of one call over the union, wherever the cut falls.  Read boundaries come from the batch
 * itself (start bits or the fixed read length): no offsets array is taken.
 *   k            1 .. 64; the table rules are bl_scan_kmer_counts's (a one-word table takes k <= 32, 2k <= key_bits)
 *   flags        BL_FLAG_CANONICAL only; BL_FLAG_SYNC is accepted and means nothing here; BL_FLAG_DROP_LAST and unknown bits are refused
 *   min_count    >= 1
 *   d_edits      16-byte aligned, room for `capacity` records, written in strictly ascending pos: a bit-reproducible order, no atomic
 *                decides placement.  Nothing is written at or beyond capacity.  NULL with capacity 0 is the counting call.
 *   stats        (nullable) host struct, always the full counts; n_runs is the sum of the five classes.
 * BL_ERR_CAPACITY when n_edits > capacity (stats still complete).  Synchronous; it first waits for the context's scans in flight.
 * An empty range, an empty batch and an empty table succeed; with an empty table every valid k-mer is weak and every run a misfit.
 *
 * bl_batch_apply_edits returns a NEW batch of the same context with the source's geometry — n_bases, n_seqs, fixed read length or
 * start bits, origin; the source is not modified.  Every byte is copied verbatim except bases[pos] = to for every edit.  `from` is
 * not checked; an edit with pos >= n_bases is ignored; among neighbouring edits with equal pos the first wins (an unsorted array with
 * duplicates is the caller's problem); whatever the array holds, no store leaves the new batch.  n_edits = 0 gives a plain copy.
 * Synchronous.
 *
 * BL_ERR_INVALID with a message, nothing launched: NULL or foreign-context ctx, batch, table or out; misaligned d_edits; d_edits NULL
 * with a capacity (or with n_edits); k out of range; a table too narrow for k; min_count = 0; min_support outside 1 .. k; bad flags;
 * a range that starts beyond the batch or holds more than 2^31 positions. */
typedef struct bl_edit {        /* 16 bytes, 16-byte aligned arrays */
    uint64_t pos;               /* position of the byte in the batch (batch-relative; the origin is NOT added: bl_batch_apply_edits consumes it) */
    uint8_t  from, to;          /* the byte that was there, the byte to write */
    uint8_t  support;           /* b - a + 1: the k-mers that vouch for the edit, 1..64 */
    uint8_t  anchor;            /* 0 left-anchored, 1 right-anchored */
    uint32_t reserved;          /* 0 */
} bl_edit;
typedef struct bl_edit_stats { uint64_t n_runs, n_edits, n_ambiguous, n_no_base, n_misfit, n_low_support, reserved[2]; } bl_edit_stats;
int bl_scan_read_edits(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, const bl_table* table,
                       uint32_t min_count, uint32_t min_support, bl_edit* d_edits, uint64_t capacity, bl_edit_stats* stats);
int bl_batch_apply_edits(bl_ctx* ctx, const bl_batch* batch, const bl_edit* d_edits, uint64_t n_edits, bl_batch** out);

/* The graph on a table's keys: the compacted de Bruijn graph (BCALM's unitigs; what assemblers, variant callers and the colored-graph
 * tools work on) of a table of canonical k-mers.  The keys are the nodes, the arcs are implied by (k - 1)-overlaps; bl_table_adjacency
 * asks the table for all eight neighbours of every key, bl_table_unitigs compacts the non-branching paths.  Usually the table is first
 * reduced to its solid k-mers with bl_table_filter.
 * SCOPE  the bidirected graph of canonical k-mers, k ODD, 1 <= k <= 63.  A key holds the first base in its most significant pair
 *   (A C G T = 0 1 2 3); canonical is the numeric minimum of the value and its reverse complement taken in 2k bits, exactly
 *   bl_scan_kmers128's with BL_FLAG_CANONICAL.  An even k (a k-mer can be its own reverse complement) and a table of forward k-mers
 *   (it needs another start rule) are refused.
 * MASK  the key x at slot i gets one byte.  Bit c (c = 0..3) is set iff the canonical form of f = ((x << 2) | c) mod 4^k is a key: the
 *   RIGHT side of x, base c appended.  Bit 4 + c is set iff the canonical form of f = (x >> 2) | (c << (2k - 2)) is a key: the LEFT side,
 *   base c prepended.  The neighbour y = canon(f) is entered by its side t: going right, t is left if y == f, else right; going left, t
 *   is right if y == f, else left.  The degree of a side is the number of bits of its nibble.  Arcs to the key itself count (AAA's right
 *   nibble has bit A), and two bases that lead to one key (f1 = rc(f2); k = 1 only) set two bits.
 * LINKS  side s of key i is linked to side t of key j iff side s has degree 1 and its one neighbour is (j, t), j != i, and side t of j
 *   has degree 1.  Links are symmetric.  d_links[2i + s] = (j << 1) | t or BL_LINK_NONE, s = 0 for the left side and 1 for the right.
 * UNITIGS  sides connected by links and by passing through a key form paths and cycles; each is one unitig and each key lies in exactly
 *   one.  A path of one key: the key as stored, flip 0.  A path of several keys starts at the end key with the smaller slot and leaves it
 *   through its linked side; a key is read as stored (flip 0) when the walk leaves it through its right side (it entered through the
 *   left), otherwise reverse-complemented (flip 1).  A cycle starts at its smallest slot, leaves through that key's right side (flip 0)
 *   and ends in front of the start: the link of the start's left side counts as cut.  Unitigs are numbered in ascending slot of their
 *   start key.  A unitig of L keys is a string of L + k - 1 uppercase ACGT bytes: the k bases of the oriented start key, then the last
 *   base of every later oriented key.  Its count sum is the 64-bit sum of its keys' counts (divided by L: BCALM's mean abundance).
 *
 * bl_table_adjacency: d_mask takes n = n_distinct bytes, d_links (nullable) 2n words; stats (nullable, host) gets its first six words:
 *   n_keys, n_arcs (all set mask bits), n_isolated (keys with no arc), n_dead_end_sides (degree 0), n_branch_sides (degree >= 2),
 *   n_linked_sides; the others are 0.
 * bl_table_unitigs: *out (nullable: labels only) is a NEW batch the library owns (bl_batch_destroy), an ordinary batch of the context
 *   for every scan: the unitig strings concatenated, origin 0; a fixed-length batch only where it holds more than one unitig and all are
 *   equally long, otherwise it carries start bits.  d_out_offsets (nullable) takes n_unitigs + 1 offsets into it, room for n + 1;
 *   d_count_sums (nullable) n_unitigs sums, room for n; d_nodes (nullable) one bl_unitig_node per key: its unitig and
 *   (rank << 1) | flip, rank counted from the start key.  n_unitigs, n_bases (nullable) are host words; stats gets all nine words:
 *   n_unitigs, n_cycles and longest_unitig (in keys) besides the six above.  An empty table gives zero unitigs: a valid batch of 0
 *   bases and 0 sequences, as bl_batch_select makes one.  Results are bit-reproducible: no atomic decides a placement.
 * Both calls are synchronous; temporaries come from the context's scratch (bl_table_unitigs: about 133 bytes per key).
 * BL_ERR_INVALID with a message, nothing written: NULL ctx or table; a table of another context; k even, 0 or above 63; 2k above the
 * table's key_bits; a table of one-word keys with k > 31; 2^31 keys or more; a table that holds a key with a bit at or above 2k or a key
 * greater than its own reverse complement (one reduction over the keys in front of everything else; the message names the first such
 * slot); bl_table_adjacency with d_mask NULL on a table that is not empty. */
#define BL_LINK_NONE 0xFFFFFFFFu
typedef struct bl_graph_stats {
    uint64_t n_keys, n_arcs;
    uint64_t n_isolated, n_dead_end_sides, n_branch_sides, n_linked_sides;
    uint64_t n_unitigs, n_cycles, longest_unitig;
    uint64_t reserved[3];
} bl_graph_stats;
typedef struct bl_unitig_node { uint32_t unitig; uint32_t rank_flip; /* (rank << 1) | flip */ } bl_unitig_node;
int bl_table_adjacency(bl_ctx* ctx, const bl_table* table, uint32_t k, uint8_t* d_mask /* n */, uint32_t* d_links /* 2n, nullable */,
                       bl_graph_stats* stats /* nullable */);
int bl_table_unitigs(bl_ctx* ctx, const bl_table* table, uint32_t k, bl_batch** out /* nullable: labels only */,
                     uint64_t* d_out_offsets /* n + 1, nullable */, uint64_t* d_count_sums /* n, nullable */,
                     bl_unitig_node* d_nodes /* n, nullable */, uint64_t* n_unitigs, uint64_t* n_bases,
                     bl_graph_stats* stats /* nullable */);

/* The compacted graph as a graph: which unitig end continues into which other unitig, in which orientation (what Bandage, assemblers,
 * variant callers and tip / bubble removal read), and the whole as GFA 1 text.
 * SCOPE  the graph of bl_table_unitigs, k odd, 3 <= k <= 63.  k = 1 is refused: two bases can lead to one key there, so two mask bits of
 *   one side could name the same neighbour side; for k >= 3 they cannot, and link records are unique.
 * ENDS  unitig u of L keys has two ends.  Its + end is the side by which the walk leaves its last key (rank L - 1): that key's right side
 *   where its flip is 0, its left side where it is 1.  Its - end is the side by which the walk entered its first key (rank 0): the left
 *   side where flip is 0, the right side where it is 1.  In one formula, the end at side s of a key with flip f has orientation
 *   o = (s == left) XOR f, and ends are numbered e = (u << 1) | o, 0 for + and 1 for -.  A cycle's two ends are its start key's left side
 *   (the cut link) and the out side of its last key.
 * LINKS  for every end e = (key i, side s) and every set bit c of that side's mask nibble (MASK above), in ascending c, there is one
 *   record {from, to}: from = e; with (j, t) the neighbour as MASK defines it, to = (unitig(j) << 1) | ((t == right) XOR flip(j)).  (j, t)
 *   is always an end of its unitig.  `to` is read exactly like `from`: the record (u, a) -> (v, b) says that the last k - 1 bases of u
 *   read in orientation a equal the first k - 1 bases of v read in orientation b (- : reverse-complemented).  The reverse
 *   (to ^ 1, from ^ 1) of every record is a record too; a record equal to its own reverse (a hairpin, u+ -> u-) appears once.  A pure
 *   cycle yields u+ -> u+ and u- -> u-.  n_links = n_arcs - n_linked_sides + 2 * n_cycles of bl_graph_stats.
 * CSR  d_link_offsets[e], e in 0 .. 2 * n_unitigs, is the index of end e's first record; records are stored in ascending e, then
 *   ascending c.  BL_LINKS_ONCE keeps a record iff from <= (to ^ 1): one of each reverse pair, a self-reverse record once; the offsets
 *   then count the kept records only.
 *
 * bl_unitig_links: d_nodes (n = n_distinct records) and d_unitig_offsets (n_unitigs + 1 words) are what bl_table_unitigs wrote for the
 *   same table and k.  The canonical-keys check is not repeated: the nodes prove that bl_table_unitigs accepted the table.  They are
 *   trusted for content, not for safety (select's policy): a node whose unitig is at or above n_unitigs is ignored (it names no end and
 *   no record), a rank is only compared; no byte outside the arrays' stated sizes is read or written.  Synchronous; temporaries come from
 *   the context's scratch (36 bytes per end).  *n_links (nullable) is always written: 0 on a refusal, else the number of records (behind
 *   BL_LINKS_ONCE where set).  d_links NULL: sizing only.  capacity < *n_links: BL_ERR_CAPACITY, d_links untouched.  No record at or
 *   behind d_links[*n_links] is written.  d_link_offsets (nullable, 2 * n_unitigs + 1 words) is written whenever the call gets as far as
 *   the count: by a sizing call and in front of BL_ERR_CAPACITY too.  stats (nullable, host): n_ends = 2 * n_unitigs; n_links as
 *   *n_links; n_self_reverse, the records equal to their own reverse; n_dead_ends / n_branch_ends, the ends with no record / with two or
 *   more — both counted before BL_LINKS_ONCE drops anything.  No atomic decides a placement: a rerun is bit-identical.
 *   BL_ERR_INVALID with a message, nothing launched: NULL ctx or table; a table of another context; k even, 0, 1 or above 63; 2k above
 *   the table's key_bits; a table of one-word keys with k > 31; 2^31 keys or more; unknown flags; n_unitigs above n_distinct; d_nodes or
 *   d_unitig_offsets NULL on a table that is not empty.
 * bl_unitigs_format_gfa writes GFA 1 text, every terminator LF:
 *     H\tVN:Z:1.0\n                                                       unless BL_GFA_NO_HEADER
 *     S\t<name u>\t<bases>\tLN:i:<bases' length>[\tKC:i:<d_count_sums[u]>]\n   for u = 0 .. n_unitigs - 1
 *     L\t<name from >> 1>\t<+|->\t<name to >> 1>\t<+|->\t<k - 1>M\n            for every record, in array order
 *   A name is name_prefix + decimal(first_number + u), 64-bit wrap as in bl_batch_format.  `unitigs` and d_unitig_offsets are
 *   bl_table_unitigs's batch and offsets, d_links (NULL iff n_links == 0) bl_unitig_links's records with either flag value.  Sizing and
 *   refusals follow bl_batch_format: *n_bytes (nullable) always receives the size of the text; d_out NULL: sizing only; capacity <
 *   *n_bytes: BL_ERR_CAPACITY, d_out untouched; no byte at or behind d_out[*n_bytes] is written; no byte behind the batch's n_bases is
 *   read (offsets are clamped to it; a link word only becomes a printed number).  bl_text_write carries the text to a file unchanged.
 *   BL_ERR_INVALID with a message, nothing launched: NULL ctx, unitigs or rule; a batch of another context; unknown flags; rule->k even
 *   or outside 3 .. 63; name_prefix without a NUL inside its 16 bytes; reserved != 0; d_out not 16-byte aligned; d_unitig_offsets NULL
 *   with n_unitigs > 0; d_links NULL with n_links > 0.
 * NOT built: L: fields in BCALM FASTA headers, km:f:, GFA 2, P and W lines inside the GFA text (the reads' walks leave as GAF:
 * bl_steps_format_gaf below); of compression (bl_text_write_bgzf) a .gzi index, a
 * run-length block header, matches across members, plain gzip output and compression levels.  (Tip, island and simple-bubble removal is
 * bl_unitigs_mark / bl_table_remove_unitigs below; superbubbles are not built.) */
typedef struct bl_unitig_link { uint32_t from, to; /* (unitig << 1) | orientation */ } bl_unitig_link;
typedef struct bl_link_stats { uint64_t n_ends, n_links, n_self_reverse, n_dead_ends, n_branch_ends, reserved[3]; } bl_link_stats;
enum { BL_LINKS_ONCE = 1u << 0 };
int bl_unitig_links(bl_ctx* ctx, const bl_table* table, uint32_t k, const bl_unitig_node* d_nodes /* n_distinct */,
                    const uint64_t* d_unitig_offsets /* n_unitigs + 1 */, uint64_t n_unitigs, uint32_t flags,
                    uint64_t* d_link_offsets /* 2 n_unitigs + 1, nullable */, bl_unitig_link* d_links /* nullable: sizing */,
                    uint64_t capacity, uint64_t* n_links, bl_link_stats* stats /* nullable */);
enum { BL_GFA_NO_HEADER = 1u << 0 };
typedef struct bl_gfa_rule {
    uint32_t flags, k;        /* k: odd, 3 .. 63; the overlap of every L line is (k - 1)M */
    char     name_prefix[16]; /* names: prefix + decimal(first_number + u), NUL-terminated */
    uint64_t first_number;
    uint64_t reserved;        /* 0 */
} bl_gfa_rule;
int bl_unitigs_format_gfa(bl_ctx* ctx, const bl_batch* unitigs, const uint64_t* d_unitig_offsets, uint64_t n_unitigs,
                          const uint64_t* d_count_sums /* nullable */, const bl_unitig_link* d_links /* nullable iff n_links == 0 */,
                          uint64_t n_links, const bl_gfa_rule* rule, uint8_t* d_out, uint64_t capacity, uint64_t* n_bytes);

/* Cleaning the compacted graph: short dead-end spurs (tips: what a sequencing error that survives bl_table_filter leaves), short isolated
 * unitigs (islands) and the lesser branches of simple bubbles (a heterozygous SNP or a short indel) are marked from the link records
 * alone, and their keys leave the table.  The result is an ordinary count table: bl_table_unitigs compacts it again, and a few rounds of
 * unitigs -> links -> mark -> remove (CountTable.clean in Python) join what the spurs and bubbles had cut.
 * NOTATION  L(u) = d_unitig_offsets[u + 1] - d_unitig_offsets[u] - (k - 1), the keys of unitig u; S(u) = d_count_sums[u].  Ends and records
 *   are bl_unitig_links's WITHOUT BL_LINKS_ONCE: out(e) is the records of end e in array order, deg(e) their number.  The end by which a
 *   record's `to` = x touches the junction is x ^ 1; x itself is its far end.
 * KEEP ORDER  w precedes u iff (S(w) * L(u), L(w), -w) > (S(u) * L(w), L(u), -u) lexicographically: the greater mean abundance, compared
 *   exactly by cross multiplication in 128-bit integers (never in floating point); then the longer one; then the smaller number.
 * ISOLATED (mark 2)  deg(2u) = deg(2u + 1) = 0, L(u) <= max_isolated_keys and S(u) <= max_isolated_mean * L(u).
 * TIP (mark 1)  exactly one end of u is dead (degree 0), e is the other one, and L(u) <= max_tip_keys: u is a tip candidate with live end
 *   e.  It is marked iff there are a record e -> f and a record f ^ 1 -> x with w = x >> 1 != u such that w is not a tip candidate with
 *   live end x ^ 1 (a real continuation leaves the junction), or w is one and precedes u.  So of several short spurs that share a junction
 *   with nothing else, the first in the keep order stays.
 * BUBBLE (mark 3)  deg(2u) = deg(2u + 1) = 1 with records 2u -> f0 and 2u + 1 -> f1, f0 >> 1 != u, f1 >> 1 != u and L(u) <= max_bubble_keys.
 *   u is marked iff there is a record f1 ^ 1 -> x with w = x >> 1 != u such that deg(x) = deg(x ^ 1) = 1, out(x)[0] = f0 and
 *   out(x ^ 1)[0] = f1 (w lies between the same anchors in the same orientations), L(w) <= max_bubble_keys,
 *   |L(w) - L(u)| <= max_bubble_diff and w precedes u.  The first branch of a bubble in the keep order is never marked.
 * Every decision is taken on the input graph at once; no mark depends on another mark, so a rerun is bit-identical, and what only appears
 * after a removal (a tip on a bubble's branch) is left to the next round.  A rule whose flag is not set marks nothing.
 *
 * bl_unitigs_mark: d_unitig_offsets (n_unitigs + 1 words) and d_count_sums (n_unitigs) are bl_table_unitigs's, d_link_offsets
 *   (2 * n_unitigs + 1) and d_links (n_links records) bl_unitig_links's; the table is no argument.  d_marks takes one byte per unitig
 *   (BL_MARK_*), no byte behind them is written; stats (nullable, host): n_unitigs, the marked unitigs of each kind, n_keys_marked = the
 *   sum of their L, count_sum_marked = the sum of their S (both mod 2^64).  The arrays are trusted for content, not for safety (select's
 *   policy): L is taken mod 2^64 and only compared and multiplied, a link offset is clamped to n_links, only the first four records of an
 *   end are read (deg is what the clamped offsets say), a `to` at or above 2 * n_unitigs is ignored, and nothing outside the stated sizes
 *   is read or written.  Synchronous.  n_unitigs = 0 succeeds with zero stats.
 *   BL_ERR_INVALID with a message, nothing launched: NULL ctx or rule; rule->k even or outside 3 .. 63; unknown flags; reserved != 0;
 *   n_unitigs >= 2^31; d_unitig_offsets, d_count_sums, d_link_offsets or d_marks NULL with n_unitigs > 0; d_links NULL with n_links > 0.
 * bl_table_remove_unitigs: *out is a NEW table (bl_table_destroy) of the same key width: key i of `table` is dropped iff
 *   d_nodes[i].unitig < n_unitigs and d_marks[d_nodes[i].unitig] != 0 (d_nodes: bl_table_unitigs's, n_distinct records; a node at or above
 *   n_unitigs keeps its key).  The kept keys stay in order with their counts; all keys dropped gives a valid empty table.  *n_removed
 *   (nullable) = the input's n_distinct minus the output's.  No atomic decides a placement.  Synchronous.
 *   BL_ERR_INVALID: NULL ctx, table or out; a table of another context; d_nodes or d_marks NULL on a table that is not empty.
 * NOT built: complex bubbles (superbubbles), coverage-ratio rules such as relative-coverage tip clipping, read-threaded decisions (their
 * evidence, the reads that crossed every link record, is bl_link_support below; no rule reads it yet), marking and removal fused into
 * bl_table_unitigs. */
enum { BL_CLEAN_TIPS = 1u << 0, BL_CLEAN_ISOLATED = 1u << 1, BL_CLEAN_BUBBLES = 1u << 2 };
enum { BL_MARK_KEEP = 0, BL_MARK_TIP = 1, BL_MARK_ISOLATED = 2, BL_MARK_BUBBLE = 3 };
typedef struct bl_clean_rule {
    uint32_t flags, k; /* BL_CLEAN_*; k: odd, 3 .. 63, the k of the unitigs */
    uint64_t max_tip_keys, max_isolated_keys, max_isolated_mean, max_bubble_keys, max_bubble_diff;
    uint64_t reserved; /* 0 */
} bl_clean_rule;
typedef struct bl_clean_stats { uint64_t n_unitigs, n_tips, n_isolated, n_bubbles, n_keys_marked, count_sum_marked, reserved[2]; } bl_clean_stats;
int bl_unitigs_mark(bl_ctx* ctx, const uint64_t* d_unitig_offsets /* n_unitigs + 1 */, const uint64_t* d_count_sums /* n_unitigs */,
                    uint64_t n_unitigs, const uint64_t* d_link_offsets /* 2 n_unitigs + 1 */, const bl_unitig_link* d_links, uint64_t n_links,
                    const bl_clean_rule* rule, uint8_t* d_marks /* n_unitigs */, bl_clean_stats* stats /* nullable */);
int bl_table_remove_unitigs(bl_ctx* ctx, const bl_table* table, const bl_unitig_node* d_nodes /* n_distinct */, const uint8_t* d_marks,
                            uint64_t n_unitigs, bl_table** out, uint64_t* n_removed /* nullable */);

/* Back from the reads to the graph: where in the compacted graph every k-mer of a read lies, contracted to one record per unitig visit
 * (what read-supported cleaning, path and walk output, pseudo-alignment, bubble phasing and threading long reads through a short-read
 * graph start from).  Terms as above: L(u) = the keys of unitig u; oriented(u, 0) its string, oriented(u, 1) its reverse complement.
 * NODE  let f be the forward k-mer at position p, valid by bl_scan_kmers128's rules, c = canon(f), s = (f != c).  If c is at slot i of
 *   the table and d_nodes[i].unitig = u < n_unitigs, with rank r and flip fl, the position has the node (u, o, off): o = s XOR fl,
 *   off = r where o = 0 and L(u) - 1 - r where o = 1.  Otherwise it has no node.  The k bases at p are oriented(u, o)[off : off + k].
 * STEP  position p + 1 continues p iff both lie in the same sequence, both have nodes, the nodes have the same u and the same o, and
 *   off(p + 1) = off(p) + 1.  A step is a maximal run of positions inside the range in which each continues its predecessor.  The test is
 *   arithmetic only: once round a cyclic unitig (off L - 1 -> off 0) starts a new step, and so does a hairpin u+ -> u-.
 * FLAGS  BL_STEP_LINKED iff position pos - 1 lies in the same sequence and has a node and pos does not continue it: on a table that is
 *   the unitigs' own the read crossed the link record (previous step's end -> this end).  BL_STEP_CONTINUED only where pos = first and
 *   `first` continues first - 1: the range cut a step.  The node at first - 1 is looked up for both flags although it lies in front of
 *   the range.  A call over the whole batch never sets CONTINUED.  The records of consecutive ranges concatenated, every CONTINUED record
 *   folded into its predecessor (n_kmers added, record dropped), are the records of one call over the union, wherever the cut falls.
 *
 * bl_scan_read_steps: the range rules are bl_scan_kmer_counts's (n = 0: to the end, at most 2^31 positions).  k odd, 3 .. 63.  The
 *   canonical form is always used (the table holds canonical keys): BL_FLAG_CANONICAL may be set or not, BL_FLAG_SYNC is accepted,
 *   BL_FLAG_DROP_LAST and unknown bits are refused.  d_nodes (n_distinct records), d_unitig_offsets (n_unitigs + 1 words) and n_unitigs
 *   are what bl_table_unitigs wrote for this table and k.  d_offsets as bl_scan_read_counts: the device copy of the batch's n_seqs + 1
 *   offsets, NULL for a single-sequence or a fixed-read-length batch; the sequence of a position is the last one whose offset is <= it.
 *   Steps are written to d_steps (16-byte aligned) in strictly ascending pos; nothing is written at or beyond `capacity`; d_steps NULL
 *   with capacity 0 is the sizing call; n_steps > capacity: BL_ERR_CAPACITY with complete stats and d_steps untouched.  stats (nullable,
 *   host): n_valid, the valid k-mers of the range; n_found, its positions with a node; n_steps; n_chains, the steps with neither flag;
 *   n_linked; longest_step (in k-mers).  Synchronous; it first waits for the context's scans in flight, like bl_scan_read_edits.
 *   Temporaries come from the context's scratch: 8 bytes per position and 8 per step.  With bl_ctx_kernel_timing on, the node pass is
 *   one launch of bl_ctx_kernel_time's sum.  An empty range, an empty batch and an empty table
 *   succeed: nothing has a node, zero steps.  No atomic decides a placement: a rerun is bit-identical.  The arrays are trusted for
 *   content, not for safety (select's policy): a node at or above n_unitigs is no node, offsets are only subtracted and compared, and no
 *   byte outside the stated sizes is read or written.
 *   BL_ERR_INVALID with a message, nothing launched: NULL ctx, batch or table; a batch or table of another context; k even or outside
 *   3 .. 63; 2k above the table's key_bits; a table of one-word keys with k > 31; 2^31 keys or more; n_unitigs above n_distinct; d_nodes
 *   or d_unitig_offsets NULL on a table that is not empty; d_offsets NULL on a batch that needs it; d_steps misaligned, or NULL with a
 *   capacity; bad flags; a range that starts beyond the batch or holds more than 2^31 positions.
 * bl_link_support: the reads that crossed every link record — the evidence of a read-threaded cleaning rule (no such rule is built).
 *   d_link_offsets, d_links and n_links are bl_unitig_links's, with either value of BL_LINKS_ONCE.  d_support[n_links] is zeroed by the
 *   call.  For every i with d_steps[i + 1].flags & BL_STEP_LINKED and d_steps[i].seq == d_steps[i + 1].seq, with a = d_steps[i].end and
 *   b = d_steps[i + 1].end: 1 is added to every record present among (a -> b) and its reverse (b ^ 1 -> a ^ 1); a self-reverse record gets
 *   the 1 once.  The records are looked for in out(a) and out(b ^ 1); only the first four records of an end are read.  A pair with an end
 *   at or above 2 * n_unitigs is ignored, link offsets are clamped to n_links.  stats (nullable, host): n_transitions, the pairs
 *   considered; n_unmatched, those that found no record.  Sums wrap mod 2^32; they are integer atomic adds, whose order does not show.
 *   Synchronous.  BL_ERR_INVALID: NULL ctx; d_steps NULL with n_steps > 0 or misaligned; n_unitigs >= 2^31; d_link_offsets NULL with
 *   n_unitigs > 0; d_links or d_support NULL with n_links > 0.
 * bl_steps_format_gaf: the walks as GAF text made on the device.  A chain is a step without BL_STEP_LINKED and every following step that
 *   has it (the first step of the array begins a chain whatever it carries).  One line per chain, every terminator LF:
 *     <qname>\t<qlen>\t<qstart>\t<qend>\t+\t<path>\t<plen>\t<pstart>\t<pend>\t<m>\t<m>\t255\n
 *   qname = read_prefix + decimal(read_first_number + seq); qlen = the sequence's length from d_offsets, the fixed read length or the
 *   batch; qstart = the first step's pos relative to its sequence; K = the sum of n_kmers over the chain; qend = qstart + K + k - 1;
 *   path = for every step '>' where o = 0 and '<' where o = 1, then segment_prefix + decimal(segment_first_number + u) — the names
 *   bl_unitigs_format_gfa prints for the same prefix and number; plen = the sum of L(u) over the chain's steps, plus k - 1; pstart = the
 *   first step's offset; pend = pstart + K + k - 1; m = K + k - 1.  Numbers wrap at 2^64 as in bl_batch_format.  On consistent inputs
 *   the spelled path's bytes [pstart, pend) are the read's bytes [qstart, qend).  Per-chain aggregates are differences of prefix sums
 *   over the steps.  A step with BL_STEP_CONTINUED is refused with a message: the caller folds first.  `batch` and d_offsets are those
 *   of bl_scan_read_steps.  Sizing and refusals follow bl_unitigs_format_gfa: *n_bytes (nullable) always receives the size of the text;
 *   d_out NULL: sizing only; capacity < *n_bytes: BL_ERR_CAPACITY, d_out untouched; no byte at or behind d_out[*n_bytes] is written.
 *   Numbers are only printed: garbage steps print garbage and touch nothing else (a unitig at or above n_unitigs has L = 0, a sequence
 *   at or above n_seqs length 0).  bl_text_write / bl_text_write_bgzf carry the text unchanged.  Synchronous; 88 bytes of scratch per step.
 *   BL_ERR_INVALID with a message, nothing launched: NULL ctx, batch or rule; a batch of another context; flags != 0; rule->k even or
 *   outside 3 .. 63; a prefix without a NUL inside its 16 bytes; reserved != 0; d_out or d_steps not 16-byte aligned; d_steps NULL with
 *   n_steps > 0; d_unitig_offsets NULL with n_unitigs > 0; d_offsets NULL on a batch that needs it.
 * NOT built: real read names from a bl_text_index (names are generated), the cs / cg tags, mapping qualities, a strand other than +. */
enum { BL_STEP_LINKED = 1u << 0, BL_STEP_CONTINUED = 1u << 1 };
typedef struct bl_read_step {   /* 32 bytes, 16-byte aligned arrays */
    uint64_t pos;      /* batch-relative position of the step's first k-mer (origin not added) */
    uint64_t seq;      /* index of the sequence */
    uint32_t end;      /* (u << 1) | o: read like a link record's `to` */
    uint32_t offset;   /* off of the first k-mer, counted along oriented(u, o) */
    uint32_t n_kmers;  /* positions of the step */
    uint32_t flags;    /* BL_STEP_LINKED | BL_STEP_CONTINUED */
} bl_read_step;
typedef struct bl_step_stats { uint64_t n_valid, n_found, n_steps, n_chains, n_linked, longest_step, reserved[2]; } bl_step_stats;
typedef struct bl_support_stats { uint64_t n_transitions, n_unmatched, reserved[2]; } bl_support_stats;
typedef struct bl_gaf_rule {
    uint32_t flags, k;           /* flags: 0; k: odd, 3 .. 63, the k of the steps */
    char     read_prefix[16];    /* qname: prefix + decimal(read_first_number + seq), NUL-terminated */
    char     segment_prefix[16]; /* segment names as bl_gfa_rule's name_prefix / first_number */
    uint64_t read_first_number, segment_first_number;
    uint64_t reserved;           /* 0 */
} bl_gaf_rule;
int bl_scan_read_steps(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t flags, const bl_table* table,
                       const bl_unitig_node* d_nodes /* n_distinct */, const uint64_t* d_unitig_offsets /* n_unitigs + 1 */, uint64_t n_unitigs,
                       const uint64_t* d_offsets /* nullable */, bl_read_step* d_steps /* nullable: sizing */, uint64_t capacity,
                       bl_step_stats* stats /* nullable */);
int bl_link_support(bl_ctx* ctx, const bl_read_step* d_steps, uint64_t n_steps, const uint64_t* d_link_offsets /* 2 n_unitigs + 1 */,
                    const bl_unitig_link* d_links, uint64_t n_links, uint64_t n_unitigs, uint32_t* d_support /* n_links */,
                    bl_support_stats* stats /* nullable */);
int bl_steps_format_gaf(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets /* nullable */, const bl_read_step* d_steps, uint64_t n_steps,
                        const uint64_t* d_unitig_offsets /* n_unitigs + 1 */, uint64_t n_unitigs, const bl_gaf_rule* rule, uint8_t* d_out,
                        uint64_t capacity, uint64_t* n_bytes);

/* The chain's exit: reads and unitigs leave as FASTA / FASTQ text made on the device, names and qualities included.
 *
 * bl_text_index_build is bl_batch_from_text that keeps what that call drops.  It accepts and refuses exactly the same texts with the same
 * messages, and its batch equals bl_batch_from_text's byte for byte (bases, offsets, the fixed-length rule).  The index owns
 *   - a device copy of the text in a buffer of its own.  This costs memory: the text stays resident beside the batch, about 2.3 times
 *     the bases for FASTQ, until bl_text_index_destroy
 *   - one 16-byte record per sequence: name_begin (u64, the first byte behind '@' / '>'), name_len (u32, the header line without marker
 *     and terminator, one trailing '\r' dropped) and qual_delta (u32, the quality line's first byte minus name_begin; 0 for FASTA).  No
 *     quality length: it is the sequence's, by the parser's own check.  A record whose name_len or qual_delta does not fit 32 bits is
 *     refused with BL_ERR_INVALID
 *   - the n_records + 1 offsets of the batch it was built with (bl_text_index_offsets, device words): what a ragged batch needs as
 *     d_offsets, and where the writer reads a source read's length.
 * bl_text_index_info: every output nullable; d_records points at the 16-byte records.  bl_text_index_destroy waits for the context's
 * stream first.  An index must be destroyed before its context.
 * bl_reader_next_batch_device_indexed cuts a file's text exactly as bl_reader_next_batch_device does and returns every span's batch with
 * its index (*out_batch NULL at the end of the file), so that a file larger than memory is rewritten span by span.
 *
 * bl_batch_format writes sequence i of `batch` (length L, offsets as bl_batch_select takes them) as one record:
 *     marker name [" LN:i:" L] [" " tag_label d_tags[i]] '\n'  bases  '\n'            and for FASTQ     "+\n" quality '\n'
 *   marker     '>' or '@' by rule->format, whatever the indexed text was: FASTQ -> FASTA and FASTA -> FASTQ are both legal.  All
 *              terminators are LF.
 *   source     s = d_source_index[i], or i where that is NULL.  With an index and s below its record count the name is the record's bytes
 *              of the text; otherwise it is generated, name_prefix + decimal(first_number + s), the quality is the fill, and no record
 *              of the index is read for s.
 *   tags       BL_FORMAT_TAG_LENGTH appends " LN:i:" + decimal(L); d_tags appends " " + tag_label + decimal(d_tags[i]).
 *   bases      the L bytes of the batch verbatim.  FASTA with line_width W > 0: a '\n' behind every W bases and no empty line where W
 *              divides L; an empty sequence is one empty line.
 *   quality    with a FASTQ index: the text's bytes [q + b, q + b + L) where q is record s's quality start and b = d_spans[2s] (0 with
 *              d_spans NULL) — d_spans are the (begin, end) pairs that went into bl_batch_select, one per record of the index.
 *              bl_batch_apply_edits keeps the geometry: a corrected batch takes the spans and index of the batch it came from.
 *              A position at or behind the quality line's end, or outside the text, gives quality_fill.  Without index qualities:
 *              quality_fill L times.
 *   empty      BL_FORMAT_SKIP_EMPTY drops sequences of length 0; otherwise they are written with empty lines (as
 *              BL_SELECT_KEEP_EMPTY leaves them: mates stay in step).
 * *n_bytes always receives the size of the text, *n_records the number of records written (both nullable).  d_out NULL: sizing only.
 * capacity < *n_bytes: BL_ERR_CAPACITY, d_out untouched.  No byte at or behind d_out[*n_bytes] is ever written.  Synchronous like
 * bl_batch_select; it first waits for the context's scans in flight.  Results are bit-reproducible: no atomic decides a placement.
 * The arrays are trusted for content, not for safety (select's policy): offsets are clamped to the batch, name and quality places to the
 * text; no byte behind the batch's n_bases or the text's n_bytes is read.
 * BL_ERR_INVALID with a message, nothing launched: a NULL ctx, batch or rule; a batch or index of another context; d_offsets NULL on a
 * ragged batch; an unknown format or flag; line_width with FASTQ; quality_fill outside 33 .. 126; name_prefix or tag_label without a NUL
 * inside its 16 bytes; reserved != 0; d_spans or d_out not 16-byte aligned.
 *
 * bl_text_write downloads d_text[0, n_bytes) in chunks through two pinned buffers and writes chunk c while chunk c + 1 copies, behind
 * the work on the context's stream.  append != 0 appends.  BL_ERR_IO where the file cannot be opened or a write comes back short.
 * bl_text_write_bgzf (below, "BGZF written on the device") is the same pipeline with the compressor in front. */
typedef struct bl_text_index bl_text_index;
int bl_text_index_build(bl_ctx* ctx, const char* text, uint64_t n_bytes, bl_batch** out_batch, bl_text_index** out_index, uint64_t* n_seqs,
                        uint64_t* n_bases);
int bl_text_index_info(const bl_text_index* index, uint64_t* n_records, int* is_fastq, const uint8_t** d_text, uint64_t* n_bytes,
                       const void** d_records);
const uint64_t* bl_text_index_offsets(const bl_text_index* index);
int bl_text_index_destroy(bl_text_index* index);
int bl_reader_next_batch_device_indexed(bl_ctx* ctx, bl_reader* reader, uint64_t max_text_bytes, bl_batch** out_batch, bl_text_index** out_index,
                                        uint64_t* n_seqs, uint64_t* n_bases);
enum { BL_FORMAT_FASTA = 0, BL_FORMAT_FASTQ = 1 };
enum { BL_FORMAT_SKIP_EMPTY = 1u << 0, BL_FORMAT_TAG_LENGTH = 1u << 1 };
typedef struct bl_format_rule {
    uint32_t format, flags;
    uint32_t line_width;      /* FASTA: bases per line, 0 = one line; must be 0 for FASTQ */
    uint32_t quality_fill;    /* FASTQ without index qualities: this byte, 33..126 */
    char     name_prefix[16]; /* generated names: prefix + decimal(first_number + s), NUL-terminated */
    uint64_t first_number;
    char     tag_label[16];   /* with d_tags: " " + tag_label + decimal(d_tags[i]), e.g. "KC:i:" */
    uint64_t reserved;        /* 0 */
} bl_format_rule;
int bl_batch_format(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const bl_text_index* index /* nullable */,
                    const uint64_t* d_source_index /* nullable */, const uint64_t* d_spans /* nullable */, const uint64_t* d_tags /* nullable */,
                    const bl_format_rule* rule, uint8_t* d_out, uint64_t capacity, uint64_t* n_bytes, uint64_t* n_records);
int bl_text_write(bl_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const char* path, int append);

/* Quality trimming and filtering on the device: the first step of a short-read pipeline (fastp, Trimmomatic, cutadapt -q) from the
 * quality bytes the index keeps.  bl_scan_read_quality makes one span per read, in the form bl_batch_select and bl_batch_format take.
 *
 * `batch` is the batch `index` was built with (same context, n_seqs == n_records, same n_bases; the offsets are the index's own).  Read i
 * has length L; its quality bytes are what bl_batch_format writes as the quality line of sequence i with this index, no d_source_index,
 * no d_spans and the rule's quality_fill: a FASTA index gives the fill everywhere.  The Phred value is
 * v[j] = min(max(byte - phred_base, 0), 93).
 *
 * Trimming.  The span starts as [b, e) = [0, L); three steps in this order, each off at its zero value:
 *   A  edges (front_q, back_q)   b = the first j >= b with v[j] >= front_q, or e; then e = one past the last j in [b, e) with
 *      v[j] >= back_q, or b
 *   B  running sum (maxsum_front_q, maxsum_back_q), the rule of BWA and cutadapt -q; both ends are decided on step A's span.  Back, with
 *      cutoff c: walk i = e - 1 down to b with s += c - v[i] and stop at the first s < 0; e' = the i of the first strict maximum of s
 *      above 0, e where there is none.  Front is the mirror image, b' = i + 1.  The span becomes [b', max(b', e')).
 *   C  window (window_len W = 1 .. 65535, window_q)   the smallest j in [b, e - W] whose W values from j on sum to less than
 *      W * window_q; if there is one, e = j, then e moves left while e > b and v[e - 1] < window_q.  A span shorter than W is not tested.
 * Statistics over the trimmed span, n = e - b: sum of the values; ee = the sum of BL_PHRED_ERR[v] = floor(2^31 * 10^(-v/10) + 1/2), the
 * expected number of errors in units of 2^-31; q_min and q_max (255 and 0 for an empty span); n_low = #{v < low_q}; n_ambiguous = the
 * bases of the span that the scans' encoder takes as invalid (anything but ACGTUacgtu).  The two counts saturate at UINT32_MAX.
 * Filters; each sets its bit of `failed`, and all that fail are set:
 *   BL_QFAIL_MIN_LEN   n < min_len                      BL_QFAIL_LOW    n_low * low_max_den > n * low_max_num
 *   BL_QFAIL_MAX_LEN   max_len != 0 and n > max_len     BL_QFAIL_MEAN   sum < mean_q * n
 *   BL_QFAIL_AMBIGUOUS n_ambiguous > max_ambiguous      BL_QFAIL_EE     ee > max_ee
 * The neutral values are 0, 0, UINT32_MAX, (1, 1), 0 and UINT64_MAX.
 * Outputs, each nullable: d_records[i] (48 bytes, 16-byte aligned; begin and end are the trimmed span BEFORE the filters);
 * d_spans[2i], d_spans[2i+1] = (begin, end) where failed == 0, else (0, 0); *stats (host).  Without stats the call is asynchronous on
 * the context's stream like the scans; with stats it is synchronous.  Results are bit-reproducible: the statistics are integer sums,
 * and no atomic decides a value.  No byte outside the text's n_bytes, the batch's n_bases or the outputs is touched.
 * BL_ERR_INVALID with a message, nothing launched: a NULL ctx, batch, index or rule; a batch or index of another context; a batch that is
 * not the index's; phred_base other than 33 or 64; quality_fill outside 33 .. 126; a threshold above 94; window_len above 65535;
 * low_max_den 0 or low_max_num > low_max_den; reserved != 0; d_records or d_spans not 16-byte aligned.
 *
 * bl_spans_intersect joins two span arrays of one batch (d_offsets as bl_batch_select takes them), one lane per read: both spans are
 * clamped to the read as bl_batch_select clamps them, out = [max of the begins, min of the ends), or (0, 0) where that is empty.  d_b
 * NULL: d_a alone.  BL_SPANS_PAIRED (n_seqs even; reads 2j and 2j + 1 are mates): where either result is empty both become (0, 0), so
 * that a dropped read takes its mate along.  d_out may be d_a or d_b.  Asynchronous.  BL_ERR_INVALID: a NULL ctx, batch, d_a or d_out; a
 * batch of another context; d_offsets NULL on a ragged batch; a misaligned array; unknown flag bits; an odd n_seqs with the flag. */
enum { BL_QFAIL_MIN_LEN = 1, BL_QFAIL_MAX_LEN = 2, BL_QFAIL_AMBIGUOUS = 4, BL_QFAIL_LOW = 8, BL_QFAIL_MEAN = 16, BL_QFAIL_EE = 32 };
typedef struct bl_quality_rule {
    uint32_t phred_base;      /* 33 or 64 */
    uint32_t quality_fill;    /* the byte of a position without a quality byte, 33..126 */
    uint32_t front_q, back_q;                 /* step A; 0 = off */
    uint32_t maxsum_front_q, maxsum_back_q;   /* step B; 0 = off */
    uint32_t window_len, window_q;            /* step C; window_len 0 = off */
    uint32_t low_q, low_max_num, low_max_den; /* fail where n_low * den > n * num; den >= 1, num <= den */
    uint32_t mean_q;
    uint32_t max_ambiguous;
    uint32_t reserved;        /* 0 */
    uint64_t min_len, max_len; /* max_len 0 = no limit */
    uint64_t max_ee;          /* in units of 2^-31 */
} bl_quality_rule;
typedef struct bl_read_quality {
    uint64_t begin, end;      /* the trimmed span, before the filters */
    uint64_t sum, ee;
    uint32_t n_low, n_ambiguous;
    uint8_t  q_min, q_max;
    uint16_t failed;          /* BL_QFAIL_* */
    uint32_t reserved;
} bl_read_quality;
typedef struct bl_quality_stats {
    uint64_t n_reads, n_reads_kept;  /* kept: failed == 0 and a span that is not empty */
    uint64_t n_bases, n_bases_kept;
    uint64_t n_too_short, n_too_long, n_ambiguous, n_low, n_mean, n_ee;  /* reads per filter bit */
    uint64_t reserved[2];
} bl_quality_stats;
int bl_scan_read_quality(bl_ctx* ctx, const bl_batch* batch, const bl_text_index* index, const bl_quality_rule* rule,
                         bl_read_quality* d_records /* nullable */, uint64_t* d_spans /* nullable */, bl_quality_stats* stats /* host, nullable */);
enum { BL_SPANS_PAIRED = 1u << 0 };
int bl_spans_intersect(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets, const uint64_t* d_a, const uint64_t* d_b /* nullable */,
                       uint32_t flags, uint64_t* d_out);

/* Adapter, read-through and poly-tail trimming on the device: the other half of what fastp, cutadapt and Trimmomatic do in front of a
 * k-mer counter.  bl_scan_read_adapters makes one span per read, in the form bl_batch_select, bl_batch_format and bl_spans_intersect take.
 *
 * d_offsets as bl_batch_select takes them; read i has length L.  A base is VALID where the scans' encoder accepts it (ACGTUacgtu, U as T);
 * an invalid base never matches anything, neither an adapter's base nor a poly base nor a mate's base.  The span starts as
 * [b, e) = d_spans_in[i] clamped to the read as bl_batch_select clamps it, [0, L) without d_spans_in.  An empty input span gives the span
 * (0, 0) and a record without a match and with cut == 0: no step runs.  Otherwise four steps in this order, each off at its zero value:
 *   1  poly tail (poly_before: a mask of bases, bit c = code c, A C G T = 0 1 2 3).  For a base X of the mask walk t = 1, 2, ... from
 *      the span's 3' end with x(t) = the number of the last t bases that are not X.  The walk stops at the first t with
 *      x(t) > poly_max_mismatch, or with t >= poly_min_len and x(t) > floor(t / poly_per) (poly_per 0: x(t) > 0).  n = the bases walked
 *      before the stop, e - b where nothing stops it.  Where n >= poly_min_len and one of those n bases is X, X proposes the position
 *      of the leftmost X among them.  e becomes the smallest proposal (on a tie the lowest code, which gives the same e).
 *   2  read-through between mates (BL_ADAPTERS_PAIRED only; reads 2j and 2j + 1 are mates r1 and r2 of lengths L1 and L2).  The WHOLE
 *      reads are compared, whatever the input spans: for I in [pair_min_overlap, min(L1, L2)], d(I) = the number of i in [0, I) where
 *      r1[i] or r2[I - 1 - i] is invalid or r1[i] != complement(r2[I - 1 - i]).  I qualifies where
 *      d(I) <= min(pair_max_diff, floor(I * pair_error_num / pair_error_den)).  The LARGEST qualifying I is the insert: both mates get
 *      insert = I, pair_mismatches = d(I) and e = max(b, min(e, I)); BL_ADAPT_PAIR is set on a mate whose end moved.  A pair with
 *      min(L1, L2) > BL_ADAPTER_PAIR_MAX_LEN is not tested: BL_ADAPT_PAIR_SKIPPED on both mates.
 *   3  3' adapters (cutadapt -a with --no-indels).  For adapter a of length A, O = min(min_overlap, A); for every p in [b, e - O],
 *      o = min(A, e - p) and m = the number of j < o where read[p + j] is invalid or differs from a[j] (letter case ignored, U = T).
 *      (a, p) is a candidate where m <= floor(o * error_num / error_den).  The match is the candidate with the most matching bases
 *      o - m, then the smaller p, then the lower a.  Then e = p; the record keeps adapter = a, match_pos = p, overlap = o and
 *      mismatches = m.  A match at p = b leaves an empty span.
 *   4  poly tail (poly_after), as step 1, on the span that is left.
 * Then n = e - b: d_spans[i] = (b, e) where n >= min_len and n > 0, else (0, 0); BL_ADAPT_TOO_SHORT where n < min_len.  The record's
 * begin and end are (b, e) before min_len.  Mates are not dropped together here: bl_spans_intersect(..., BL_SPANS_PAIRED) does that.
 * Statistics: n_reads_cut = reads with one of the four step bits; n_reads_kept, n_bases_kept = reads and bases of the spans that are
 * not (0, 0); one count per bit of `cut`; per_adapter[a] = reads matched by adapter a.
 * Outputs, each nullable: d_records[i] (32 bytes, 16-byte aligned), d_spans, *stats (host).  Without stats the call is asynchronous on
 * the context's stream like the scans; with stats it is synchronous.  Results are bit-reproducible: no atomic and no shared memory
 * decides a value or a place.  The bases come from the batch's packed 2-bit copy where it has one, from the ASCII bases where a
 * 16-base chunk holds an invalid base and for a batch without a copy; no byte outside the batch's n_bases, the copy or the outputs is
 * touched.  match_pos saturates at UINT32_MAX - 1 for a position beyond it.
 * BL_ERR_INVALID with a message, nothing launched: a NULL ctx, batch or rule; a batch of another context; d_offsets NULL on a ragged
 * batch; unknown flag bits; BL_ADAPTERS_PAIRED with an odd n_seqs; n_adapters > 8; an adapter length of 0 or above 64; an adapter byte
 * outside ACGTUacgtu; min_overlap 0 with n_adapters > 0; a denominator of 0 or num > den; pair_min_overlap 0 under the flag; a poly mask
 * above 15; poly_min_len 0 with a mask set; reserved != 0; d_records, d_spans or d_spans_in not 16-byte aligned.
 * Knowingly different from cutadapt and fastp: no indels, no wildcards in adapters, 3' adapters only, one match per read, and no
 * fall-back from step 2 to step 3 (both always run). */
#define BL_MAX_ADAPTERS 8
#define BL_ADAPTER_MAX_LEN 64
#define BL_ADAPTER_PAIR_MAX_LEN 512
enum { BL_ADAPT_POLY_BEFORE = 1, BL_ADAPT_PAIR = 2, BL_ADAPT_ADAPTER = 4, BL_ADAPT_POLY_AFTER = 8,
       BL_ADAPT_TOO_SHORT = 16, BL_ADAPT_PAIR_SKIPPED = 32 };
enum { BL_ADAPTERS_PAIRED = 1u << 0 };
typedef struct bl_adapter_rule {
    uint32_t flags;                      /* BL_ADAPTERS_PAIRED: reads 2j and 2j + 1 are mates, step 2 runs */
    uint32_t n_adapters;                 /* 0 .. 8; 0 = step 3 off */
    uint32_t adapter_len[BL_MAX_ADAPTERS];                  /* 1 .. 64 */
    char     adapters[BL_MAX_ADAPTERS][BL_ADAPTER_MAX_LEN]; /* ACGTUacgtu only, no wildcard */
    uint32_t min_overlap;                /* step 3, >= 1 (cutadapt -O) */
    uint32_t error_num, error_den;       /* step 3: mismatches allowed in an overlap of o bases = floor(o * num / den); den >= 1, num <= den */
    uint32_t pair_min_overlap;           /* step 2, >= 1 */
    uint32_t pair_error_num, pair_error_den, pair_max_diff;
    uint32_t poly_before, poly_after;    /* masks of bases, bit c = code c of the scans' encoder; 0 = off */
    uint32_t poly_min_len, poly_per, poly_max_mismatch;   /* poly_per 0 = no mismatch allowed */
    uint32_t reserved;
    uint64_t min_len;                    /* span (0, 0) where the result is shorter */
} bl_adapter_rule;
typedef struct bl_read_adapters {        /* 32 bytes, 16-byte aligned */
    uint64_t begin, end;                 /* the span after the four steps, before min_len */
    uint32_t match_pos;                  /* read-relative start of step 3's match, UINT32_MAX: none */
    uint32_t insert;                     /* step 2's I, 0: none */
    uint16_t adapter;                    /* index of the matched adapter, 0xFFFF: none */
    uint8_t  overlap, mismatches;        /* of step 3's match */
    uint16_t pair_mismatches;
    uint8_t  cut;                        /* BL_ADAPT_*: which steps moved an end, TOO_SHORT, PAIR_SKIPPED */
    uint8_t  reserved;
} bl_read_adapters;
typedef struct bl_adapter_stats {
    uint64_t n_reads, n_reads_cut, n_reads_kept, n_bases, n_bases_kept;
    uint64_t n_poly_before, n_pair, n_adapter, n_poly_after, n_too_short, n_pair_skipped;
    uint64_t per_adapter[BL_MAX_ADAPTERS];
    uint64_t reserved[5];
} bl_adapter_stats;
int bl_scan_read_adapters(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets /* as bl_batch_select */,
                          const uint64_t* d_spans_in /* nullable */, const bl_adapter_rule* rule,
                          bl_read_adapters* d_records /* nullable */, uint64_t* d_spans /* nullable */,
                          bl_adapter_stats* stats /* host, nullable */);

/* Duplicate removal on the device: what fastp --dedup, clumpify dedupe and Picard MarkDuplicates (without coordinates) do in front of a
 * k-mer counter, so that a duplicated fragment's errors do not pass a count filter.  bl_scan_read_duplicates finds the units of a batch
 * that are EXACTLY equal and writes one record per unit and one span per read, in the form bl_batch_select, bl_batch_format and
 * bl_spans_intersect take.
 *
 * Units.  A unit is a read; under BL_DEDUP_PAIRED it is the pair of reads 2u and 2u + 1, and n_seqs must be even.
 * Letters.  A, C, G, T, with U read as T and letter case ignored; any byte the scans' encoder takes as invalid is one fifth letter N.
 *   N equals N and never equals a base.
 * Key of a read.  Its span: d_spans_in[i] clamped to the read as bl_batch_select clamps it, [0, L) without d_spans_in (d_offsets as
 *   bl_batch_select takes them); cut to its first prefix_len bases where prefix_len > 0.  The key is that string of letters; length
 *   counts: ACG is not ACGA.
 * Key of a unit.  For a read its key s; for a pair the ordered pair (s1, s2).
 * Equality.  Two units are equal where their keys are equal.  Under BL_DEDUP_CANONICAL they are also equal where a read's key is the
 *   reverse complement of the other's (rc(N) = N), and where a pair's (s1, s2) is the other's (s2, s1): the same fragment sequenced
 *   from its other strand swaps the mates without reverse-complementing them.
 * Empty units.  A unit with an empty span in any of its reads is empty: BL_DUP_EMPTY, first = kept = itself, copies = 0.  It belongs to
 *   no class, and its reads' clamped spans pass through, an empty one as (0, 0).
 * Classes.  The other units fall into classes of equal units.  first is the lowest unit index of the class.  Without d_scores kept is
 *   first.  With d_scores (one word per READ) a unit's score is the wrapping 64-bit sum of its reads' scores, and kept is the member
 *   with the largest score, the lowest index on a tie (Picard's best sum of base qualities; bl_read_quality's sum is the intended
 *   input).  copies is the class size, on every member.
 * Flags.  BL_DUP_DUPLICATE on every member but kept.  BL_DUP_REVERSED where a member's forward key differs from the kept unit's.
 * Spans.  d_spans of a duplicate's reads are (0, 0); those of a kept unit's reads are the clamped input spans (not cut to prefix_len).
 * Statistics.  n_units; n_empty; n_classes; n_duplicates and n_reversed = the units with that flag; largest_class; n_reads_kept and
 *   n_bases_kept = reads and bases of the spans written that are not (0, 0); class_hist[c - 1] = classes of size c, the last entry
 *   those of 16 or more (fastp's duplication histogram).  n_mixed_groups and rounds describe the work done, not the result, and depend
 *   on hash_bits and seed; nothing else does.
 * Results are exact and bit-identical over reruns: no atomic decides a value or a place.  Outputs, each nullable: d_records[u] (16
 * bytes, 16-byte aligned, one per UNIT), d_spans (one pair per READ), *stats (host).  The call waits for the device once per
 * resolution round (one round unless hash_bits is small) and returns without waiting for its last kernels where stats is NULL; with
 * stats it is synchronous.  No byte outside the batch's n_bases, its packed copy and the outputs is touched.  Temporaries come from
 * the context's scratch, 93 bytes per unit.  With bl_ctx_kernel_timing on, the call sets five markers (bl_ctx_mark): in front of its
 * first phase and behind each of its four phases (DESIGN.md §5.4u names them).
 * BL_ERR_INVALID with a message, nothing launched: a NULL ctx, batch or rule; a batch of another context; d_offsets NULL on a ragged
 * batch; unknown flag bits; BL_DEDUP_PAIRED with an odd n_seqs; hash_bits above 96; reserved != 0; 2^32 units or more; d_records,
 * d_spans or d_spans_in not 16-byte aligned.
 * Not done: duplicates across batches, near-duplicates with mismatches, UMIs, optical coordinates from names, merging of mates. */
enum { BL_DEDUP_PAIRED = 1u << 0, BL_DEDUP_CANONICAL = 1u << 1 };
enum { BL_DUP_DUPLICATE = 1, BL_DUP_EMPTY = 2, BL_DUP_REVERSED = 4 };
typedef struct bl_dedup_rule {
    uint32_t flags;         /* BL_DEDUP_* */
    uint32_t hash_bits;     /* 0 = the default (96); 1 .. 96: how finely the units are grouped before they are compared.  Changes speed only */
    uint64_t prefix_len;    /* 0 = the whole span; P > 0: only the first P bases of every read's span are its key */
    uint64_t seed;          /* changes the grouping only, never a result */
    uint64_t reserved;      /* 0 */
} bl_dedup_rule;
typedef struct bl_read_duplicate {   /* 16 bytes, 16-byte aligned; one per UNIT */
    uint32_t first;   /* lowest unit index of the class */
    uint32_t kept;    /* the unit of the class that stays */
    uint32_t copies;  /* class size, on every member; 0 on an empty unit */
    uint32_t flags;   /* BL_DUP_* */
} bl_read_duplicate;
typedef struct bl_dedup_stats {
    uint64_t n_units, n_empty, n_classes, n_duplicates, n_reversed, largest_class;
    uint64_t n_reads_kept, n_bases_kept;     /* reads and bases of the spans written that are not (0, 0) */
    uint64_t class_hist[16];                 /* classes of size 1 .. 15, and 16 or more */
    uint64_t n_mixed_groups;                 /* groups of units compared together that held more than one class: not part of the result */
    uint64_t rounds;                         /* resolution rounds run: same remark */
    uint64_t reserved[6];
} bl_dedup_stats;
int bl_scan_read_duplicates(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_offsets /* as bl_batch_select */,
                            const uint64_t* d_spans_in /* nullable */, const uint64_t* d_scores /* one per READ, nullable */,
                            const bl_dedup_rule* rule, bl_read_duplicate* d_records /* nullable */, uint64_t* d_spans /* nullable */,
                            bl_dedup_stats* stats /* host, nullable */);

/* Count reduction across the GPUs of one node: ctxs[g] is the context of device g (all distinct devices),
 * counters holds n_gpu rows of n 64-bit counters — row g = GPU g's local counts in, the column sums out (in every row).  One
 * ncclAllReduce(sum, uint64) per GPU over RCCL / xGMI, called on RCCL's C API directly (librccl.so.1 is loaded on first use);
 * communicators are created once per device set and cached.  XOR digests have no RCCL reduction: fold them on the host. */
int bl_count_allreduce(bl_ctx* const* ctxs, int n_gpu, uint64_t* counters, int n);

/* Super-k-mer bucket exchange (record of reference super_kmer_view.hpp:20-24 made self-contained).
 * bl_pack_super_kmers: one 16-byte record per group of bl_scan_super_kmers — d_records[2g] = bases 0..31 of the group's
 *   size + k - 1 bases (2 bits each, first base most significant), d_records[2g+1] = bases 32.. in bits 63..10, mm_pos in
 *   bits 9..5 (d_mm_pos is REQUIRED: bl_count_super_kmers finds a record's minimizer through it), size - 1 in bits 4..0.
 *   Needs 2k - m <= 59.  d_first_pos holds what the scan of THIS batch reported: positions in the caller's whole when the batch
 *   has an origin (bl_batch_set_origin).  A position outside the batch — in front of the origin (by any distance: the difference
 *   is never added to), or at or behind origin + n_bases — packs an EMPTY record: all base bits zero (d_records[2g] == 0 and
 *   bits 63..10 of d_records[2g+1] == 0), while mm_pos and size - 1 in bits 9..0 are kept as given.  A group that starts inside
 *   the batch and runs over its end packs the bases up to the end; those behind it are code 0, bits 9..0 again as given (the
 *   record still claims `size` k-mers).  Neither case reads a byte in front of or behind the batch's n_bases bases.
 * bl_partition_records: reorder 16-byte records into `parts` (<= 64) contiguous buckets by d_hashes[g] % parts (the
 *   minimizer hash the scan returned = the owner rank); counts[b] (host) = records in bucket b.
 * bl_expand_super_kmers: records -> their k-mers (canonical with BL_FLAG_CANONICAL), group after group;
 *   BL_ERR_CAPACITY with *n_kmers = need when d_kmers is too small. */
int bl_pack_super_kmers(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_first_pos, const uint8_t* d_sizes, const uint8_t* d_mm_pos, uint64_t n_groups,
                        uint32_t k, uint32_t m, uint64_t* d_records);
/* bl_scan_super_kmer_records: bl_scan_super_kmers + bl_pack_super_kmers in one scan — the groups leave the scan as packed records
 *   (d_records[2r], d_records[2r+1] as above, with mm_pos) beside the hashes of their minimizers (d_hashes[r]: the owner of the
 *   record), built from the 2-bit codes the scan holds anyway: no position / size arrays written and read back, no second pass
 *   over the bases.  Needs 2k - m <= 59.  result as bl_scan_super_kmers.
 *   Range: the groups are bl_scan_super_kmers' of the same range, clipped to it in the same way: a record packs the size + k - 1 bases of
 *   the clipped piece, from the first k-mer inside the range, with mm_pos counted in that k-mer and size the k-mers inside the range.
 *   Expanding the records of consecutive ranges gives every k-mer of their union exactly once. */
int bl_scan_super_kmer_records(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t m, uint64_t seed, uint32_t flags,
                               uint64_t* d_records, uint64_t* d_hashes, uint64_t capacity, bl_result* result);
/* bl_count_super_kmers: the exact multiplicity of every (canonical) k-mer of the packed records WITHOUT a global sort: records are
 *   grouped by the hash of their minimizer (found again through mm_pos; `m`, `seed` and the canonical flag as given to the scan)
 *   into buckets of a few thousand k-mers, and every bucket is expanded and counted in an LDS hash table by one workgroup (buckets
 *   that do not fit take a sort + run-length path).  All occurrences of a canonical k-mer share their minimizer, so they meet in
 *   one bucket and the count is exact.  d_kmers / d_counts receive the distinct k-mers and their multiplicities in NO particular
 *   order; BL_ERR_CAPACITY with *n_distinct = need when they are too small.  A bucket's table is filled in rounds, so what bounds a
 *   bucket is its DISTINCT k-mers, not their occurrences: reads of high coverage (every minimizer many times over) stay in the tables. */
int bl_count_super_kmers(bl_ctx* ctx, const uint64_t* d_records, uint64_t n_groups, uint32_t k, uint32_t m, uint64_t seed, uint32_t flags, uint64_t* d_kmers,
                         uint32_t* d_counts, uint64_t capacity, uint64_t* n_distinct);
int bl_partition_records(bl_ctx* ctx, const uint64_t* d_hashes, const uint64_t* d_records, uint64_t n, uint32_t parts, uint64_t* d_out, uint64_t* counts);
int bl_expand_super_kmers(bl_ctx* ctx, const uint64_t* d_records, uint64_t n_groups, uint32_t k, uint32_t flags, uint64_t* d_kmers, uint64_t capacity,
                          uint64_t* n_kmers);

/* ---- the same pipeline for k up to 64: 32-byte records, 128-bit k-mers -----------------------------------------------------------
 * bl_scan_super_kmers has no upper limit on k (1 <= m <= 32, w = k - m + 1 <= 64): it is the reference's own super-k-mer driver
 * instantiation, KmerType = __uint128_t, MinimizerType = uint64_t.  These calls take its groups on.  The 64-bit calls above keep
 * their limits and their 16-byte record.
 * THE RECORD: four 64-bit words per group, d_records[4g .. 4g+3], the array 32-byte aligned (BL_ERR_INVALID otherwise):
 *   words 0, 1, 2   bases 0..31, 32..63, 64..95 of the group's size + k - 1 bases
 *   word 3          bases 96..121 in bits 63..12, mm_pos (0..63) in bits 11..6, size - 1 (0..63) in bits 5..0
 *   2 bits per base, first base in the most significant pair (the 16-byte record's packing); base bits beyond the group's own bases are 0.
 * LIMITS: 1 <= m <= 32, m <= k <= 64, k - m + 1 <= 64, 2k - m <= 122 (BL_ERR_INVALID with a message naming them).  k <= 32 is allowed.
 * The minimizer is the m-mer bl_scan_super_kmers reports, hashed as an 8-BYTE key (bl_hash64_u64).  The k-mers are bl_scan_kmers128's:
 * value in 128 bits, reverse complement taken in 2k bits, canonical = numeric minimum.
 * bl_pack_super_kmers128: the arrays of bl_scan_super_kmers -> records.  The clipping contract is bl_pack_super_kmers': the batch's
 *   origin is honoured; a position in front of the origin (by any distance) or at or behind origin + n_bases packs an EMPTY record (all
 *   base bits zero) with bits 11..0 as given; a group that runs over the end packs code 0 behind the end, bits 11..0 as given; no byte
 *   outside the batch's n_bases is read.  d_mm_pos is required.
 * bl_scan_super_kmer_records128: bl_scan_super_kmers + bl_pack_super_kmers128 in one scan — the record is built inside the scan's record
 *   pass from the 2-bit codes the tile holds; no per-group arrays are written and read back and the bases are not read a second time.
 *   The output is exactly what the two calls give for the same arguments: d_records[4r .. 4r+3] as above, d_hashes[r] the minimizer's
 *   hash (8-byte key).  The batch's origin does not change the records.  Either output may be NULL (both NULL: count only); nothing is
 *   written at or beyond `capacity`; the result always carries the full count, with BL_ERR_CAPACITY when it exceeds `capacity`;
 *   `result` is bl_scan_super_kmers'; ranges concatenate as for every scan; no byte outside the batch's n_bases is read.
 * bl_partition_records128: bl_partition_records for 32-byte records (d_out 32-byte aligned too).
 * bl_expand_super_kmers128: records -> their k-mers, group after group, two words per k-mer (low, high; d_kmers 16-byte aligned).
 *   BL_ERR_CAPACITY with *n_kmers = need when d_kmers is too small; nothing is written then.  Only 1 <= k <= 64 is checked (no m).
 * bl_count_super_kmers128: bl_count_super_kmers' contract — exact multiplicities of the (canonical) k-mers, no particular order, two
 *   words per distinct k-mer in d_kmers (low, high; 16-byte aligned); either output pointer NULL = count only; BL_ERR_CAPACITY with
 *   *n_distinct = need when the arrays are too small, and NOTHING is written then.  Buckets by minimizer hash are counted by one wave
 *   each in an LDS table of 16-byte keys whose empty slots are marked by an owner word, not by a key value: every k and strand mode is
 *   taken, k = 64 without the canonical flag (the all-T 64-mer is all ones) included.  Oversized buckets take expand + 128-bit sort +
 *   run-length; bl_ctx_set_option("count128_tables", 0) sends every bucket that way (same result).  Terminates on any record bits.
 *   (bl_sort_u128 / bl_count_sorted_u128 put the distinct k-mers in order; bl_table_build_u128 takes the two arrays as they are and
 *   answers lookups, bl_scan_kmer_counts and the spectrum from them.)
 * NOT provided for k > 32: biolib_amd::read_pool for wide views, and any multi-GPU measurement of this path. */
int bl_scan_super_kmer_records128(bl_ctx* ctx, const bl_batch* batch, uint64_t first, uint64_t n, uint32_t k, uint32_t m, uint64_t seed, uint32_t flags,
                                  uint64_t* d_records /* 4 per group, 32-byte aligned */, uint64_t* d_hashes, uint64_t capacity, bl_result* result);
int bl_pack_super_kmers128(bl_ctx* ctx, const bl_batch* batch, const uint64_t* d_first_pos, const uint8_t* d_sizes, const uint8_t* d_mm_pos, uint64_t n_groups,
                           uint32_t k, uint32_t m, uint64_t* d_records /* 4 per group */);
int bl_partition_records128(bl_ctx* ctx, const uint64_t* d_hashes, const uint64_t* d_records, uint64_t n, uint32_t parts, uint64_t* d_out, uint64_t* counts);
int bl_expand_super_kmers128(bl_ctx* ctx, const uint64_t* d_records, uint64_t n_groups, uint32_t k, uint32_t flags, uint64_t* d_kmers /* 2 per k-mer: lo, hi */,
                             uint64_t capacity, uint64_t* n_kmers);
int bl_count_super_kmers128(bl_ctx* ctx, const uint64_t* d_records, uint64_t n_groups, uint32_t k, uint32_t m, uint64_t seed, uint32_t flags,
                            uint64_t* d_kmers /* 2 per distinct k-mer: lo, hi */, uint32_t* d_counts, uint64_t capacity, uint64_t* n_distinct);

/* ---- BGZF on the device (ingest) -----------------------------------------------------------------------
 * A bgzip'ed file is a chain of gzip members of at most 64 KiB of text each, every one an independent deflate stream: the
 * device inflates a span's members side by side (one wavefront each) and checks their CRC-32, so that the file crosses PCIe
 * compressed.  bl_reader_next_batch_device does this for BGZF input by itself; the two calls below are its building blocks.
 * The reference reads .gz through zlib's gzread (tests/kseq.h:41-42 KSEQ_INIT(gzFile, gzread), tests/test_kmer_view.cpp:23-27):
 * same text, produced here. */
typedef struct {
    uint64_t src_off;  /* the member's deflate data inside the packed buffer */
    uint64_t dst_off;  /* where its text goes inside the text buffer */
    uint32_t src_len;  /* bytes of deflate data */
    uint32_t isize;    /* bytes of text (gzip ISIZE), <= 65536 */
    uint32_t crc;      /* CRC-32 of the text (gzip trailer) */
    uint32_t reserved;
} bl_bgzf_member;
/* Host: walk the member headers in bytes[0 .. n_bytes) and fill members[] (at most `capacity`) with offsets src_base + ... /
 * dst_base + ...; stops in front of a member that is not completely inside the bytes.  *consumed = bytes walked, *text_bytes =
 * the sum of the members' text sizes.  BL_ERR_INVALID for anything that is not a BGZF member header. */
int bl_bgzf_walk(const void* bytes, uint64_t n_bytes, uint64_t src_base, uint64_t dst_base, bl_bgzf_member* members, uint64_t capacity, uint64_t* n_members,
                 uint64_t* consumed, uint64_t* text_bytes);
/* Device, asynchronous on the context's stream: inflate the members described by d_members[0 .. n_members) from d_packed
 * (4-byte aligned, packed_bytes long, its allocation a whole number of dwords) into d_text (text_bytes long).  d_status[i] becomes 0 for a sound member, otherwise a
 * non-zero code (damaged deflate data, text size or CRC-32 that differ from the trailer); a table entry that points outside the
 * two buffers is refused, not followed, and nothing outside a member's own [dst_off, dst_off + isize) is ever written. */
int bl_bgzf_inflate(bl_ctx* ctx, const void* d_packed, uint64_t packed_bytes, const bl_bgzf_member* d_members, uint64_t n_members, void* d_text,
                    uint64_t text_bytes, uint32_t* d_status);

/* ---- BGZF written on the device (the chain's exit compressed) ----------------------------------------------------
 * bl_bgzf_deflate turns the device text d_text[0, n_bytes) into a chain of BGZF members in d_out, one wavefront per member: the text is
 * cut into members of 65,280 bytes (bgzip's 0xff00), the last one holds the rest.  A member is the 18-byte BGZF header (1f 8b 08 04,
 * MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00, BSIZE - 1), ONE deflate block, CRC-32 and ISIZE.  The 28-byte EOF marker (the empty
 * member with the fixed-code data 03 00) follows unless BL_BGZF_NO_EOF is set; n_bytes == 0 gives the marker alone, or nothing.
 * Members are contiguous in d_out; no byte at or behind d_out[*n_out_bytes] is written.
 *   the block     the smallest of three forms in bytes, stored / fixed codes / dynamic codes, ties in that order; the sizes are known
 *                 exactly after the code build, before a bit is written.  Stored keeps every member at or below ISIZE + 31 bytes:
 *                 bl_bgzf_bound = n_bytes + 31 * ceil(n_bytes / 65280) + 28 (without the 28 under BL_BGZF_NO_EOF) is the exact worst case.
 *   the codes     Huffman lengths from the block's own histograms, ties by symbol number, limited to 15 bits by the count-per-length
 *                 adjustment; an alphabet with fewer than two used symbols gets two 1-bit codes.  The dynamic header sends the code
 *                 lengths one by one with 4 bits each (HCLEN 19, no repeat symbols): at most 57 + 4 * (HLIT + HDIST) bits, 0.25 % of a member.
 *   the matches   LZ77 inside the member's own text, distances up to 32,768, lengths 3..258, a deterministic function of the member's
 *                 bytes (bl_deflate_core.hpp; restated in tests/deflate_cases.py); greedy, no lazy evaluation.
 * capacity < bl_bgzf_bound(n_bytes, flags): BL_ERR_CAPACITY, nothing launched, *n_out_bytes = the bound (there is no sizing run: it
 * would compress twice).  d_members (nullable, device, one row per member with text; the EOF marker is not listed) receives exactly what
 * bl_bgzf_inflate takes: src_off / src_len the deflate data inside d_out, dst_off its place in the text, isize and crc.  *n_members
 * (nullable) = ceil(n_bytes / 65280).  Synchronous, behind the work on the context's stream; temporaries come from the context's scratch
 * and are bounded by 1,024 members in flight (334 MB), not by n_bytes.  Reruns are bit-identical: no atomic decides a placement.  No byte at or
 * behind d_text[n_bytes] is read, whatever the alignment of d_text.
 * BL_ERR_INVALID with a message, nothing launched: a NULL ctx; NULL d_text with n_bytes > 0; NULL d_out or n_out_bytes; unknown flags;
 * d_out not 16-byte aligned.
 *
 * bl_text_write_bgzf is bl_text_write with the compressor in front: the text goes in chunks of 1,024 members (66.8 MB: a wave a member,
 * fewer would leave the device idle); a chunk's size is fetched into a pinned word and exactly that many bytes are copied; chunk c + 1
 * is copied and chunk c + 2 compressed while chunk c is written, so only compressed bytes cross the link.  The EOF marker is written
 * once at the end unless BL_BGZF_NO_EOF is set (a file appended to in several calls: set it on all but the last, or finish with a call of
 * n_bytes == 0).  append and BL_ERR_IO as in bl_text_write.  Every call pins its two host buffers and takes its two device buffers anew,
 * each sized by the smaller of the text and a chunk; they are not kept between calls.
 * NOT built: a .gzi index, a run-length block header, matches across members, plain single-stream gzip output, compression levels. */
enum { BL_BGZF_NO_EOF = 1u << 0 };
uint64_t bl_bgzf_bound(uint64_t n_bytes, uint32_t flags);
int bl_bgzf_deflate(bl_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t flags, uint8_t* d_out, uint64_t capacity, uint64_t* n_out_bytes,
                    bl_bgzf_member* d_members /* nullable */, uint64_t* n_members /* nullable */);
int bl_text_write_bgzf(bl_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const char* path, int append, uint32_t flags);

/* Measurement helper: sustained HBM rates of THIS device — a read-only streaming kernel over n_bytes and a
 * device-to-device copy (read + write bytes counted), `iters` repetitions each; bench.py reports them next to the 8 TB/s spec. */
int bl_probe_hbm(bl_ctx* ctx, uint64_t n_bytes, int iters, double* read_gbps, double* copy_gbps);

/* Shader clock held while other work runs: bl_clock_probe_start launches one sleeping wave on its own stream that stamps the
 * shader-cycle and the 100 MHz real-time counters until bl_clock_probe_finish stops it (at the latest duration_ms later, 1..5000);
 * finish returns cycles / time in GHz and releases the probe.  Finish it BEFORE any device-wide synchronise.  Used by bench.py to price the VALU ceiling at the clock of the run. */
typedef struct bl_clock_probe bl_clock_probe;
int bl_clock_probe_start(bl_ctx* ctx, uint32_t duration_ms, bl_clock_probe** out);
int bl_clock_probe_finish(bl_clock_probe* probe, double* shader_ghz);

/* Device-side parser: copy raw FASTA / FASTQ TEXT (already in host memory, e.g. a read()/mmap of the file) to the GPU
 * and build the batch there: newline index, line classification, prefix sums, gather of the sequence lines.  Same
 * sequences as bl_reader_* for the regular layouts it accepts — FASTQ with exactly 4 lines per record, FASTA with any
 * line wrapping, LF or CRLF — and BL_ERR_INVALID for anything else (never a silent mis-parse).  Names are not kept
 * (bl_text_index_build keeps them, and the qualities, on the device). */
int bl_batch_from_text(bl_ctx* ctx, const char* text, uint64_t n_bytes, bl_batch** out, uint64_t* n_seqs, uint64_t* n_bases);

/* ---- spill / wire formats read by biolib's consumers -------------------------------------
 * bl_write_run_u64: a run file of emem::external_memory_vector<uint64_t> (external_memory_vector.hpp:243-262): the
 *   SORTED keys as raw little-endian 8-byte values, no header.  bl_run_file_name builds the reference's file name
 *   <dir>/tmp.run[_<name>]_<id>.bin (:253-262).
 * bl_write_vector_u64: io::basic_store(std::vector<uint64_t>) (io.hpp:104-112): size_t count, then the elements.
 * Both copy the device array to the host and write synchronously. */
int bl_run_file_name(const char* dir, const char* name, uint64_t id, char* out, uint64_t out_len);
int bl_write_run_u64(bl_ctx* ctx, const uint64_t* d_sorted_keys, uint64_t n, const char* path);
int bl_write_vector_u64(bl_ctx* ctx, const uint64_t* d_keys, uint64_t n, const char* path);
/* The read side (reference io::basic_load io.hpp:114-122; external_memory_vector::const_iterator :265-347, a k-way merge over
 * the run files): files biolib wrote feed the device set operations.
 * bl_file_count_u64: elements in a run file (with_count = 0) or a basic_store'd vector (with_count = 1, checked against the size).
 * bl_read_file_u64_host / bl_read_file_u64: its elements into a host / device array of `capacity` elements.
 * bl_merge_runs_u64: the sorted union (duplicates kept) of n_paths run files in one device array — what iterating the
 *   reference's external_memory_vector yields; BL_ERR_CAPACITY with *n_total = need when d_out is too small. */
int bl_file_count_u64(const char* path, int with_count, uint64_t* n);
int bl_read_file_u64_host(const char* path, int with_count, uint64_t* out, uint64_t capacity, uint64_t* n);
int bl_read_file_u64(bl_ctx* ctx, const char* path, int with_count, uint64_t* d_out, uint64_t capacity, uint64_t* n);
int bl_merge_runs_u64(bl_ctx* ctx, const char* const* paths, uint32_t n_paths, uint64_t* d_out, uint64_t capacity, uint64_t* n_total);

/* The same files for 16-byte keys: emem::external_memory_vector<__uint128_t> and io::basic_store(std::vector<__uint128_t>).  A run
 * file holds the sorted keys as raw 16-byte little-endian elements (low word first), no header; a stored vector is a size_t count
 * followed by the elements.  This is what the reference writes when it is built the way its own CMake builds it — the GNU dialect
 * gnu++17, under which std::is_fundamental<__uint128_t> holds, which io::basic_store asserts before it writes the raw bytes; a strict
 * -std=c++17 build of the reference does not compile such a vector.  Arguments, capacities (in KEYS, two words each) and error codes as
 * their u64 namesakes; the device arrays are 16-byte aligned. */
int bl_write_run_u128(bl_ctx* ctx, const uint64_t* d_sorted_keys, uint64_t n, const char* path);
int bl_write_vector_u128(bl_ctx* ctx, const uint64_t* d_keys, uint64_t n, const char* path);
int bl_file_count_u128(const char* path, int with_count, uint64_t* n);
int bl_read_file_u128_host(const char* path, int with_count, uint64_t* out /* 2 per key */, uint64_t capacity, uint64_t* n);
int bl_read_file_u128(bl_ctx* ctx, const char* path, int with_count, uint64_t* d_out, uint64_t capacity, uint64_t* n);
int bl_merge_runs_u128(bl_ctx* ctx, const char* const* paths, uint32_t n_paths, uint64_t* d_out, uint64_t capacity, uint64_t* n_total);

/* ---- device memory helpers (for callers without their own allocator) ----------------------------- */
int bl_device_alloc(bl_ctx* ctx, uint64_t bytes, void** d_ptr);
int bl_device_free(bl_ctx* ctx, void* d_ptr);
/* Page-locked host memory (copies to and from it are single DMA transfers; its pages are mapped once, at allocation): what a
 * caller that downloads results batch after batch should copy into (include/compat/read_pool.hpp does). */
int bl_host_alloc(bl_ctx* ctx, uint64_t bytes, void** ptr);
int bl_host_free(bl_ctx* ctx, void* ptr);
int bl_copy_to_host(bl_ctx* ctx, void* dst, const void* d_src, uint64_t bytes); /* synchronous */
int bl_copy_to_device(bl_ctx* ctx, void* d_dst, const void* src, uint64_t bytes); /* synchronous */

/* ---- host-side scalar helper (bit-exact with the device hash) ------------------------------------- */
uint64_t bl_hash64_u64(uint64_t value, uint64_t seed);
/* hash::hash64::hash<__uint128_t>(value, seed), value = hi << 64 | lo: the 16 bytes hashed are lo's then hi's */
uint64_t bl_hash64_u128(uint64_t lo, uint64_t hi, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* BIOLIB_AMD_H */
