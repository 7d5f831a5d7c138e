// bl_host.hip — the host helpers of bl_host.hpp that instantiate device code: blh::exclusive_sum, so that rocPRIM's scan of 8-byte words
// is compiled once for the library and not once per unit that sums tile totals.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "bl_host.hpp"

namespace blh {

int exclusive_sum(bl_ctx* ctx, const uint64_t* in, uint64_t* out, size_t n, hipStream_t s)
{
    const hipError_t e = with_workspace(ctx, 5, [&](void* ws, size_t& bytes) { return rocprim::exclusive_scan(ws, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), s); });
    if (e == hipErrorOutOfMemory) return bl_set_error(BL_ERR_OOM, "scratch allocation failed");
    return e == hipSuccess ? BL_OK : hip_rc(e);
}

}  // namespace blh
