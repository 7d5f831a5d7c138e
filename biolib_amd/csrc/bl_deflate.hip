// bl_deflate.hip — BGZF written on the device: bl_bgzf_bound, bl_bgzf_deflate (a device text as a chain of BGZF members, one wave per
// member; the encoder is bl_deflate_core.hpp) and bl_text_write_bgzf (bl_text_write's pipeline with the compressor in front: only
// compressed bytes cross the link).  Kernels:
//   deflate_members_kernel   one wave per member of a group: the whole member (header, one deflate block, CRC-32, ISIZE) into the member's
//                            fixed-stride slot of context scratch, its size and CRC-32 into two arrays
//   (rocPRIM)                exclusive sum of the group's sizes
//   gather_members_kernel    one workgroup per member: the slot's bytes to their place in d_out, the member's row of d_members
//   advance_kernel           the running end of the output (a device word) moves behind the group
//   eof_kernel               the 28-byte EOF marker
// Temporaries are bounded by GROUP_MEMBERS members in flight, not by the text: a text of more members goes group by group on the stream,
// without a host wait in between.
//
// Formats: RFC 1951 (deflate), RFC 1952 (gzip member), SAM specification §4.1 (BGZF: extra field 'B','C', 2, BSIZE = member size - 1;
// the EOF marker is the empty member with the fixed-code data 03 00).
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/biolib_amd.h"
#include "bl_deflate_core.hpp"
#include "bl_host.hpp"

namespace bl_deflate {

constexpr uint32_t GROUP_MEMBERS = 1024;    // members compressed side by side (334 MB of slots and token areas)
constexpr uint32_t CHUNK_MEMBERS = 1024;    // bl_text_write_bgzf: members per chunk (66.8 MB of text): a group, so that a chunk fills the device
constexpr uint32_t TOKEN_STRIDE = MAX_TOKENS + 1;
constexpr uint32_t GATHER_THREADS = 256;

__constant__ uint8_t g_eof_marker[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
const uint8_t h_eof_marker[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// what one group needs of scratch slot 4, every part 64-byte aligned
struct Arena {
    uint8_t* slots;    // [g][SLOT_BYTES]
    uint32_t* tokens;  // [g][TOKEN_STRIDE]
    uint64_t* sizes;   // [g + 1], the last one 0
    uint64_t* starts;  // [g + 1]: the exclusive sum, the last one the group's bytes
    uint32_t* crcs;    // [g]
    uint64_t* end;     // the output's running end
    uint32_t* err;     // != 0: a member did not come out at the size computed beforehand (never)
};
size_t round64(size_t x) { return (x + 63) & ~(size_t)63; }
size_t arena_bytes(uint32_t g)
{
    return round64((size_t)g * SLOT_BYTES) + round64((size_t)g * TOKEN_STRIDE * 4) + 2 * round64((size_t)(g + 1) * 8) + round64((size_t)g * 4) + 128;
}
Arena carve(void* base, uint32_t g)
{
    Arena a;
    uint8_t* p = static_cast<uint8_t*>(base);
    a.slots = p;
    p += round64((size_t)g * SLOT_BYTES);
    a.tokens = reinterpret_cast<uint32_t*>(p);
    p += round64((size_t)g * TOKEN_STRIDE * 4);
    a.sizes = reinterpret_cast<uint64_t*>(p);
    p += round64((size_t)(g + 1) * 8);
    a.starts = reinterpret_cast<uint64_t*>(p);
    p += round64((size_t)(g + 1) * 8);
    a.crcs = reinterpret_cast<uint32_t*>(p);
    p += round64((size_t)g * 4);
    a.end = reinterpret_cast<uint64_t*>(p);
    a.err = reinterpret_cast<uint32_t*>(p + 64);
    return a;
}

__global__ __launch_bounds__(64) void deflate_members_kernel(const uint8_t* text, uint64_t n_bytes, uint64_t first_member, uint32_t count, Arena a)
{
    __shared__ Shared sh;
    const uint32_t mi = blockIdx.x;
    if (mi >= count) return;
    const uint64_t off = (first_member + mi) * (uint64_t)MEMBER_TEXT;
    const uint32_t len = n_bytes - off < MEMBER_TEXT ? (uint32_t)(n_bytes - off) : MEMBER_TEXT;
    uint32_t crc;
    const uint32_t size = deflate_member(sh, text + off, len, a.tokens + (size_t)mi * TOKEN_STRIDE, a.slots + (size_t)mi * SLOT_BYTES, crc);
    if ((threadIdx.x & 63u) == 0) {
        a.sizes[mi] = size;
        a.crcs[mi] = crc;
        if (mi == 0) a.sizes[count] = 0;
        if (size == 0) *a.err = 1;
    }
}

__global__ __launch_bounds__(GATHER_THREADS) void gather_members_kernel(uint64_t n_bytes, uint64_t first_member, uint32_t count, Arena a, uint8_t* out,
                                                                        bl_bgzf_member* members)
{
    const uint32_t mi = blockIdx.x;
    if (mi >= count) return;
    const uint64_t at = *a.end + a.starts[mi];
    const uint32_t size = (uint32_t)a.sizes[mi];
    gather_member(a.slots + (size_t)mi * SLOT_BYTES, out + at, size, threadIdx.x, GATHER_THREADS);
    if (members && threadIdx.x == 0 && size >= 26) {
        const uint64_t off = (first_member + mi) * (uint64_t)MEMBER_TEXT;
        bl_bgzf_member m;
        m.src_off = at + 18;
        m.dst_off = off;
        m.src_len = size - 26;
        m.isize = n_bytes - off < MEMBER_TEXT ? (uint32_t)(n_bytes - off) : MEMBER_TEXT;
        m.crc = a.crcs[mi];
        m.reserved = 0;
        members[first_member + mi] = m;
    }
}

__global__ void advance_kernel(uint32_t count, Arena a) { *a.end += a.starts[count]; }

__global__ __launch_bounds__(64) void eof_kernel(Arena a, uint8_t* out)
{
    const uint64_t at = *a.end;
    if (threadIdx.x < 28) out[at + threadIdx.x] = g_eof_marker[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) *a.end = at + 28;
}

namespace {

using blh::hip_rc;
using blh::invalid;

uint64_t members_of(uint64_t n_bytes) { return (n_bytes + MEMBER_TEXT - 1) / MEMBER_TEXT; }

// Everything of one text on the stream, nothing waited for: a.end becomes the byte count of the output.  The arena holds `group` members.
int enqueue(bl_ctx* ctx, hipStream_t s, const Arena& a, uint32_t group, const uint8_t* d_text, uint64_t n_bytes, bool eof, uint8_t* d_out, bl_bgzf_member* d_members)
{
    BLH_TRY(hipMemsetAsync(a.end, 0, 128, s));  // (the end and the error word)
    const uint64_t n_members = members_of(n_bytes);
    for (uint64_t first = 0; first < n_members; first += group) {
        const uint32_t count = n_members - first < group ? (uint32_t)(n_members - first) : group;
        hipLaunchKernelGGL(deflate_members_kernel, dim3(count), dim3(64), 0, s, d_text, n_bytes, first, count, a);
        BLH_TRY(hipGetLastError());
        BLH_OK(blh::exclusive_sum(ctx, a.sizes, a.starts, (size_t)count + 1, s));
        hipLaunchKernelGGL(gather_members_kernel, dim3(count), dim3(GATHER_THREADS), 0, s, n_bytes, first, count, a, d_out, d_members);
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, s, count, a);
        BLH_TRY(hipGetLastError());
    }
    if (eof) {
        hipLaunchKernelGGL(eof_kernel, dim3(1), dim3(64), 0, s, a, d_out);
        BLH_TRY(hipGetLastError());
    }
    return BL_OK;
}

bool arena_for(bl_ctx* ctx, uint64_t n_members, uint32_t& group, Arena& a)
{
    group = n_members < GROUP_MEMBERS ? (uint32_t)(n_members ? n_members : 1) : GROUP_MEMBERS;
    void* base = bl_ctx_scratch(ctx, 4, arena_bytes(group));
    if (!base) return false;
    a = carve(base, group);
    return true;
}

int io_error(const char* what, const char* path) { return bl_set_error(BL_ERR_IO, (std::string(what) + path + ": " + std::strerror(errno)).c_str()); }

}  // namespace

}  // namespace bl_deflate

extern "C" uint64_t bl_bgzf_bound(uint64_t n_bytes, uint32_t flags)
{
    return n_bytes + (uint64_t)bl_deflate::MEMBER_OVERHEAD * bl_deflate::members_of(n_bytes) + ((flags & BL_BGZF_NO_EOF) ? 0u : 28u);
}

extern "C" int bl_bgzf_deflate(bl_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, uint32_t flags, uint8_t* d_out, uint64_t capacity, uint64_t* n_out_bytes,
                               bl_bgzf_member* d_members, uint64_t* n_members)
{
    using namespace bl_deflate;
    if (!ctx) return invalid("bl_bgzf_deflate: ctx is NULL");
    if (!d_text && n_bytes) return invalid("bl_bgzf_deflate: d_text is NULL");
    if (!d_out || !n_out_bytes) return invalid("bl_bgzf_deflate: d_out or n_out_bytes is NULL");
    if (flags & ~(uint32_t)BL_BGZF_NO_EOF) return invalid("bl_bgzf_deflate: unknown flag bits");
    if (blh::misaligned16(d_out)) return invalid("bl_bgzf_deflate: d_out must be 16-byte aligned");
    const uint64_t bound = bl_bgzf_bound(n_bytes, flags), total_members = members_of(n_bytes);
    if (n_members) *n_members = total_members;
    if (capacity < bound) {
        *n_out_bytes = bound;
        return bl_set_error(BL_ERR_CAPACITY, "bl_bgzf_deflate: d_out is smaller than bl_bgzf_bound (*n_out_bytes says how large that is)");
    }
    *n_out_bytes = 0;
    if (bound == 0) return BL_OK;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);  // behind the context's work in flight
    uint32_t group;
    Arena a;
    if (!arena_for(ctx, total_members, group, a)) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    const int rc = enqueue(ctx, s, a, group, d_text, n_bytes, !(flags & BL_BGZF_NO_EOF), d_out, d_members);
    if (rc != BL_OK) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    unsigned long long end = 0;
    unsigned int err = 0;
    BLH_TRY(hipMemcpyAsync(&end, a.end, sizeof(end), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipMemcpyAsync(&err, a.err, sizeof(err), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    if (err || end > bound) return bl_set_error(BL_ERR_INTERNAL, "bl_bgzf_deflate: a member did not come out at the size computed for it");
    *n_out_bytes = end;
    return BL_OK;
}

// Device text to a BGZF file: chunks of CHUNK_MEMBERS members; a chunk's size is fetched into a pinned word, then exactly that many
// compressed bytes are copied; chunk c + 1 is copied and chunk c + 2 compressed while chunk c is written.
extern "C" int bl_text_write_bgzf(bl_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const char* path, int append, uint32_t flags)
{
    using namespace bl_deflate;
    if (!ctx || !path || (n_bytes && !d_text)) return invalid("NULL argument");
    if (flags & ~(uint32_t)BL_BGZF_NO_EOF) return invalid("bl_text_write_bgzf: unknown flag bits");
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    FILE* f = std::fopen(path, append ? "ab" : "wb");
    if (!f) return io_error("cannot open ", path);
    hipStream_t s = bl_ctx_stream(ctx);
    const uint64_t chunk_text = (uint64_t)CHUNK_MEMBERS * MEMBER_TEXT;
    const uint64_t n_chunks = (n_bytes + chunk_text - 1) / chunk_text;
    const uint64_t first_text = n_bytes < chunk_text ? n_bytes : chunk_text;
    const size_t packed_cap = (size_t)bl_bgzf_bound(first_text, BL_BGZF_NO_EOF) + 64;
    uint8_t* h_buf[2] = {nullptr, nullptr};
    unsigned long long* h_size = nullptr;  // two pinned words
    blh::Pooled<uint8_t> d_packed[2];
    hipEvent_t sized[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    unsigned long long size[2] = {0, 0};
    int rc = BL_OK;
    uint32_t group = 0;
    Arena a{};
    if (n_chunks) {
        if (!arena_for(ctx, members_of(first_text), group, a)) rc = bl_set_error(BL_ERR_OOM, "scratch allocation failed");
        hipError_t e = rc == BL_OK ? hipHostMalloc(reinterpret_cast<void**>(&h_size), 2 * sizeof(unsigned long long), hipHostMallocDefault) : hipSuccess;
        for (int i = 0; i < 2 && rc == BL_OK && e == hipSuccess; ++i) {
            d_packed[i] = blh::Pooled<uint8_t>(ctx, packed_cap);
            if (!d_packed[i]) rc = bl_set_error(BL_ERR_OOM, "device allocation failed (compressed chunk)");
            if (rc == BL_OK) e = hipHostMalloc(reinterpret_cast<void**>(&h_buf[i]), packed_cap, hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&sized[i], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&copied[i], hipEventDisableTiming);
        }
        if (rc == BL_OK && e != hipSuccess) rc = hip_rc(e);
    }
    auto text_of = [&](uint64_t c) { return n_bytes - c * chunk_text < chunk_text ? n_bytes - c * chunk_text : chunk_text; };
    // chunk c compressed into its device buffer, its size on the way into the pinned word
    auto compress = [&](uint64_t c) {
        int r = enqueue(ctx, s, a, group, d_text + c * chunk_text, text_of(c), false, d_packed[c & 1].get(), nullptr);
        if (r != BL_OK) return r;
        BLH_TRY(hipMemcpyAsync(&h_size[c & 1], a.end, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        BLH_TRY(hipEventRecord(sized[c & 1], s));
        return (int)BL_OK;
    };
    // its size is here: the copy of exactly that many bytes
    auto download = [&](uint64_t c) {
        BLH_TRY(hipEventSynchronize(sized[c & 1]));
        size[c & 1] = h_size[c & 1];
        if (size[c & 1] > packed_cap) return bl_set_error(BL_ERR_INTERNAL, "bl_text_write_bgzf: a chunk came out larger than its bound");
        BLH_TRY(hipMemcpyAsync(h_buf[c & 1], d_packed[c & 1].get(), size[c & 1], hipMemcpyDeviceToHost, s));
        BLH_TRY(hipEventRecord(copied[c & 1], s));
        return (int)BL_OK;
    };
    // Chunk c is written while the copy of chunk c + 1 and the compression of chunk c + 2 run, in that order on the stream: a copy needs
    // its size on the host, which is there once the chunk's compression is over — one step earlier.  Chunk c + 2 takes the device buffer
    // of chunk c (copied: waited for below) and chunk c + 1 the pinned buffer of chunk c - 1 (written in the step before).
    if (rc == BL_OK && n_chunks) {
        rc = compress(0);
        if (rc == BL_OK) rc = download(0);
        if (rc == BL_OK && n_chunks > 1) rc = compress(1);
    }
    for (uint64_t c = 0; c < n_chunks && rc == BL_OK; ++c) {
        const hipError_t e = hipEventSynchronize(copied[c & 1]);
        if (e != hipSuccess) { rc = hip_rc(e); break; }
        if (c + 1 < n_chunks) rc = download(c + 1);
        if (rc == BL_OK && c + 2 < n_chunks) rc = compress(c + 2);
        if (rc != BL_OK) break;
        if (std::fwrite(h_buf[c & 1], 1, size[c & 1], f) != size[c & 1]) rc = io_error("short write to ", path);
    }
    (void)hipStreamSynchronize(s);  // nothing copies into the buffers when they go
    if (rc == BL_OK && !(flags & BL_BGZF_NO_EOF) && std::fwrite(h_eof_marker, 1, 28, f) != 28) rc = io_error("short write to ", path);
    if (std::fclose(f) != 0 && rc == BL_OK) rc = io_error("closing ", path);
    for (int i = 0; i < 2; ++i) {
        if (sized[i]) (void)hipEventDestroy(sized[i]);
        if (copied[i]) (void)hipEventDestroy(copied[i]);
        if (h_buf[i]) (void)hipHostFree(h_buf[i]);
    }
    if (h_size) (void)hipHostFree(h_size);
    return rc;
}
