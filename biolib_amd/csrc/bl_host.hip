// bl_host.hip — the host helpers of bl_host.hpp that need a definition: blh::exclusive_sum, so that rocPRIM's scan of 8-byte words is
// compiled once for the library and not once per unit that sums tile totals, and the argument checks the entry points share.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <string>

#include "bl_host.hpp"

namespace blh {

int exclusive_sum(bl_ctx* ctx, const uint64_t* in, uint64_t* out, size_t n, hipStream_t s)
{
    const hipError_t e = with_workspace(ctx, 5, [&](void* ws, size_t& bytes) { return rocprim::exclusive_scan(ws, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), s); });
    if (e == hipErrorOutOfMemory) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    return e == hipSuccess ? BL_OK : hip_rc(e);
}

int exclusive_sum_total(bl_ctx* ctx, const uint64_t* in, uint64_t* out, size_t n, hipStream_t s, uint64_t* total)
{
    BLH_OK(exclusive_sum(ctx, in, out, n, s));
    BLH_TRY(hipMemcpyAsync(total, out + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    BLH_TRY(hipStreamSynchronize(s));
    return BL_OK;
}

int batch_view(bl_ctx* ctx, const bl_batch* batch, BatchView& v)
{
    bl_ctx* owner = nullptr;
    bl_batch_describe(batch, &owner, &v.n_bases, &v.n_seqs, &v.read_len);
    if (owner != ctx) return invalid("the batch belongs to another context");
    v.bases = static_cast<const uint8_t*>(bl_batch_device_bases(batch));
    return BL_OK;
}

int range_end(uint64_t n_bases, uint64_t first, uint64_t n, const char* noun, uint64_t& end)
{
    if (first > n_bases) return invalid("range starts beyond the batch");
    end = (n == 0 || n > n_bases - first) ? n_bases : first + n;  // first + n cannot wrap here
    if (end - first > (1ull << 31)) return invalid((std::string(noun) + " may hold at most 2^31 positions; split it").c_str());
    return BL_OK;
}

int offsets_needed(const uint64_t* d_offsets, uint64_t n_seqs, uint64_t read_len)
{
    if (!d_offsets && n_seqs > 1 && read_len == 0)
        return invalid("d_offsets is NULL: only a single-sequence or a fixed-read-length batch finds its sequences without the offsets");
    return BL_OK;
}

int table_owner(const bl_ctx* owner, const bl_ctx* ctx) { return owner == ctx ? BL_OK : invalid("the table belongs to another context"); }

int table_takes_k(uint32_t key_words, uint32_t key_bits, uint32_t k)
{
    if (key_words == 1 && k > 32) return invalid("a table of one-word keys takes k <= 32");
    if (k >= 1 && 2 * k > key_bits) return invalid(("2k = " + std::to_string(2 * k) + " exceeds the table's key_bits = " + std::to_string(key_bits)).c_str());
    return BL_OK;
}

}  // namespace blh
