// bl_host.hpp — what the translation units of the library share on the HOST side: the functions bl_capi.hip defines for the other units,
// declared once, and the few helpers every entry point repeats (namespace blh).  Internal; never included from a *_core.hpp (those
// compile without HIP in tests/emu).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "../../include/biolib_amd.h"

// ------------------------------------------------------------------------------------------------ defined in bl_capi.hip
int bl_set_error(int code, const char* msg);  // the thread's bl_last_error(); returns code
// The stream every non-scan entry point enqueues on: the borrowed one or lane 0's, made to wait for a scan still running on lane 1.
hipStream_t bl_ctx_stream(bl_ctx* ctx);
int bl_ctx_device(bl_ctx* ctx);
// With bl_ctx_kernel_timing on: an event pair on `stream` around what the caller enqueues between start = 1 and start = 0, added to
// bl_ctx_kernel_time's sum as one launch.  Nothing otherwise.
int bl_ctx_kernel_event(bl_ctx* ctx, hipStream_t stream, int start);
int bl_ctx_kernel_timing_on(bl_ctx* ctx);   // bl_ctx_kernel_timing is on: a call of several phases may set bl_ctx_mark markers between them
int bl_ctx_count128_tables(bl_ctx* ctx);    // the "count128_tables" option
int bl_ctx_jaccard128_path(bl_ctx* ctx);    // the "jaccard128_path" option
int bl_ctx_table_prefix_bits(bl_ctx* ctx);  // the "table_prefix_bits" option

// Grow-only device scratch that lives with the context; NULL on failure.  The caller has synchronised the slot's previous use (the entry
// points that use it are synchronous).
//   slot   holds                                       used by
//   0      candidates; heads and tails of the steps    bl_correct; bl_steps
//   0-3    arenas, library workspace, keys, counts,    the k-mer counters (bl_superkmer*.hip; the 128-bit one keeps its run count in 7) and
//          the text (3)                                the text parser, which call the set operations while they hold them
//   4      data; blpart::partition's histogram,        the set operations (bl_keylist.hpp), the owner splits, the table build and algebra, the
//          offsets and bucket starts                   quantiles, select, format, the corrector, the graph (about 133 bytes per key in slot 4),
//   5      library workspace (rocPRIM):                links, clean, the BGZF writer (slots, token areas and sizes of the members in flight)
//          blh::exclusive_sum(_total) take it          and the steps (8 bytes per position; 88 per step for the GAF text): none of them calls
//                                                      another while it holds 4-6
//   6      counters, flags, statistics                 (bl_dedup.hip: 93 bytes per unit in slot 4, rocPRIM's workspace in 5, counters and flags in 6)
void* bl_ctx_scratch(bl_ctx* ctx, int slot, size_t bytes);

// Device memory of short-lived batch buffers, recycled between batches.  bl_ctx_pool_free takes NULL, and hipFree()s what is not the pool's.
void* bl_ctx_pool_alloc(bl_ctx* ctx, size_t bytes);
void bl_ctx_pool_free(bl_ctx* ctx, void* p);

// New batches around pool buffers the caller filled on bl_ctx_stream (bases: >= n_bases + 64 bytes, zero padded).  Ownership: both calls
// take their buffers whatever they return — on success the batch owns them (adopt_device frees the offsets once the start bits are built),
// on failure they have been freed.  The caller release()s its blh::Pooled holders into the call and never frees afterwards.
//   adopt_device   DEVICE offsets[n_seqs + 1]; fixed_len != 0: every sequence is that long, the batch is a fixed-length one
//   adopt_like     the geometry of `like` (n_bases, n_seqs, read length, origin); d_start_bits: a pool copy of like's, or NULL
int bl_batch_adopt_device(bl_ctx* ctx, void* d_bases, uint64_t n_bases, uint64_t* d_offsets, uint64_t n_seqs, uint64_t fixed_len, bl_batch** out);
int bl_batch_adopt_like(bl_ctx* ctx, const bl_batch* like, void* d_bases, uint32_t* d_start_bits, bl_batch** out);
int bl_batch_describe(const bl_batch* batch, bl_ctx** ctx, uint64_t* n_bases, uint64_t* n_seqs, uint64_t* read_len);
// the start-bit vector the position-tiled scans read (NULL: one sequence).  ensure: build it where a fixed-length batch has not needed it yet
int bl_batch_scan_view(bl_ctx* ctx, const bl_batch* batch, int ensure, const uint32_t** start_bits);
// the batch's packed copy (bl_scan_core.hpp: ScanParams::codes_packed, chunk_bad), NULL where it has none or the context's "packed_codes" is 0
int bl_batch_packed_view(bl_ctx* ctx, const bl_batch* batch, const uint32_t** codes, const uint32_t** chunk_bad);
// (bl_batch_device_bases is public: include/biolib_amd.h)
// what bl_text_index_info does not tell (bl_format.hip): the index's context and the n_bases of the batch it was built with
int bl_text_index_describe(const bl_text_index* index, bl_ctx** ctx, uint64_t* n_bases);

// ------------------------------------------------------------------------------------------------ helpers
namespace blh {

inline int hip_rc(hipError_t e) { return bl_set_error(e == hipErrorOutOfMemory ? BL_ERR_OOM : BL_ERR_HIP, hipGetErrorString(e)); }
inline int invalid(const char* msg) { return bl_set_error(BL_ERR_INVALID, msg); }

// One bl_ctx_pool_alloc buffer, freed on scope exit unless release()d (into bl_batch_adopt_*, or to a caller that frees it itself).
template <typename T>
class Pooled {
public:
    Pooled() = default;
    Pooled(bl_ctx* ctx, size_t bytes) : ctx_(ctx), p_(static_cast<T*>(bl_ctx_pool_alloc(ctx, bytes))) {}
    Pooled(Pooled&& o) noexcept : ctx_(o.ctx_), p_(o.release()) {}
    Pooled& operator=(Pooled&& o) noexcept
    {
        if (this != &o) {
            bl_ctx_pool_free(ctx_, p_);
            ctx_ = o.ctx_;
            p_ = o.release();
        }
        return *this;
    }
    Pooled(const Pooled&) = delete;
    Pooled& operator=(const Pooled&) = delete;
    ~Pooled() { bl_ctx_pool_free(ctx_, p_); }

    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    T* release()
    {
        T* p = p_;
        p_ = nullptr;
        return p;
    }

private:
    bl_ctx* ctx_ = nullptr;
    T* p_ = nullptr;
};

// The two calls of a rocPRIM device primitive: call(nullptr, bytes) asks for the size; the workspace is scratch `slot`; call(ws, bytes)
// runs.  hipErrorOutOfMemory if the slot cannot grow.  Two primitives of one entry point may take the same slot one after the other
// without a wait in between: a slot only grows, and bl_ctx_scratch synchronises the device before it replaces the block.
template <typename F>
hipError_t with_workspace(bl_ctx* ctx, int slot, F&& call)
{
    size_t bytes = 0;
    const hipError_t e = call(static_cast<void*>(nullptr), bytes);
    if (e != hipSuccess) return e;
    void* ws = bl_ctx_scratch(ctx, slot, bytes ? bytes : 16);
    return ws ? call(ws, bytes) : hipErrorOutOfMemory;
}

// Exclusive sum of n 8-byte words on `stream` (rocPRIM; its workspace is scratch slot 5, which a second sum on the same stream may take
// again at once).  Defined in bl_host.hip: the library's one instantiation of that scan.
int exclusive_sum(bl_ctx* ctx, const uint64_t* in, uint64_t* out, size_t n, hipStream_t stream);
// The same, then out[n - 1] copied to *total and the stream waited for (n >= 1; callers end `in` with a word of 0: the sum of the rest).
int exclusive_sum_total(bl_ctx* ctx, const uint64_t* in, uint64_t* out, size_t n, hipStream_t stream, uint64_t* total);

inline unsigned blocks_for(uint64_t threads, unsigned tpb) { return (unsigned)((threads + tpb - 1) / tpb); }
inline size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
// the 16 bytes of a rule's name: the length up to the NUL inside them, -1 without one; the first len bytes as two little-endian words
inline int terminated_length(const char* s)
{
    for (int i = 0; i < 16; ++i)
        if (!s[i]) return i;
    return -1;
}
inline void pack_prefix(const char* s, int len, uint64_t w[2])
{
    w[0] = w[1] = 0;
    for (int i = 0; i < len; ++i) w[i >> 3] |= (uint64_t)(uint8_t)s[i] << (8 * (i & 7));
}

// ---- The argument checks the entry points share: BL_OK, or BL_ERR_INVALID with the one text each has.  They stand between a caller's
// mistake and a kernel that reads outside an array.  Separate functions, because the entry points differ in what they check in between,
// and the order in which a call refuses is part of its behaviour.  (Defined in bl_host.hip.)
struct BatchView {
    const uint8_t* bases;
    uint64_t n_bases, n_seqs, read_len;  // read_len: 0 unless the batch is one of fixed-length reads
};
int batch_view(bl_ctx* ctx, const bl_batch* batch, BatchView& v);  // "the batch belongs to another context"; neither pointer is NULL
// end: n == 0 or a range past the batch ends with it.  Refuses first > n_bases, and more than 2^31 positions: "<noun> may hold at most ..."
int range_end(uint64_t n_bases, uint64_t first, uint64_t n, const char* noun, uint64_t& end);
int offsets_needed(const uint64_t* d_offsets, uint64_t n_seqs, uint64_t read_len);  // NULL offsets on a batch of ragged sequences
int table_owner(const bl_ctx* owner, const bl_ctx* ctx);                           // "the table belongs to another context"
int table_takes_k(uint32_t key_words, uint32_t key_bits, uint32_t k);             // one-word keys hold k <= 32; 2k <= key_bits

}  // namespace blh

#define BLH_TRY(call)                                 \
    do {                                              \
        hipError_t e_ = (call);                       \
        if (e_ != hipSuccess) return blh::hip_rc(e_); \
    } while (0)
// the same for a call that answers a status of the library (the error text is set)
#define BLH_OK(call)                    \
    do {                                \
        const int rc_ = (call);         \
        if (rc_ != BL_OK) return rc_;   \
    } while (0)
