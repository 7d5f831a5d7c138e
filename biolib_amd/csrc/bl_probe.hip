// bl_probe.hip — two measurements of the device the benchmark reports next to its rates: the HBM bandwidth a streaming kernel and a
// device-to-device copy reach (bl_probe_hbm), and the shader clock the chip holds while other kernels run (bl_clock_probe_*).
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/biolib_amd.h"
#include "bl_host.hpp"

// ---------------------------------------------------------------------------------------------------------
// Measured HBM peaks (SURVEY.md §8d "confirm on the box ... report the measured peak next to the spec"): a read-only
// streaming kernel (16 B per lane, grid-stride, XOR-folded so nothing is elided) and a device-to-device copy.
namespace {

struct Quad {
    unsigned int x, y, z, w;
};

__global__ __launch_bounds__(256) void stream_read_kernel(const Quad* __restrict__ src, unsigned long long n16, unsigned int* sink)
{
    unsigned int acc = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {  // four independent loads in flight per lane
        const Quad a = src[i], b = src[i + stride], c = src[i + 2 * stride], d = src[i + 3 * stride];
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
    }
    for (; i < n16; i += stride) {
        const Quad a = src[i];
        acc ^= a.x ^ a.y ^ a.z ^ a.w;
    }
    if (acc == 0x9e3779b9u) *sink = acc;  // practically never: keeps the loads alive
}

}  // namespace

extern "C" int bl_probe_hbm(bl_ctx* ctx, uint64_t n_bytes, int iters, double* read_gbps, double* copy_gbps)
{
    if (!ctx || !read_gbps || !copy_gbps || iters < 1 || n_bytes < (1u << 20)) return bl_set_error(BL_ERR_INVALID, "bad argument (>= 1 MiB, >= 1 iteration)");
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    hipStream_t s = bl_ctx_stream(ctx);
    n_bytes &= ~(uint64_t)15;
    void *a = nullptr, *b = nullptr;
    unsigned int* sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMalloc(&a, n_bytes);
    if (e == hipSuccess) e = hipMalloc(&b, n_bytes);
    if (e == hipSuccess) e = hipMalloc(&sink, 4);
    if (e == hipSuccess) e = hipMemsetAsync(a, 0x5a, n_bytes, s);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float ms_read = 0, ms_copy = 0;
    if (e == hipSuccess) {
        const unsigned blocks = 256 * 16;  // 16 workgroups per CU
        hipLaunchKernelGGL(stream_read_kernel, dim3(blocks), dim3(256), 0, s, static_cast<const Quad*>(a), n_bytes / 16, sink);  // warm-up
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters; ++i)
            hipLaunchKernelGGL(stream_read_kernel, dim3(blocks), dim3(256), 0, s, static_cast<const Quad*>(a), n_bytes / 16, sink);
        (void)hipEventRecord(e1, s);
        e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_read, e0, e1);
    }
    if (e == hipSuccess) {
        e = hipMemcpyAsync(b, a, n_bytes, hipMemcpyDeviceToDevice, s);  // warm-up
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters && e == hipSuccess; ++i) e = hipMemcpyAsync(b, a, n_bytes, hipMemcpyDeviceToDevice, s);
        (void)hipEventRecord(e1, s);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_copy, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (sink) (void)hipFree(sink);
    if (e != hipSuccess) return blh::hip_rc(e);
    *read_gbps = (double)n_bytes * iters / (ms_read * 1e-3) / 1e9;
    *copy_gbps = 2.0 * (double)n_bytes * iters / (ms_copy * 1e-3) / 1e9;  // read + write
    return BL_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Shader clock held by the chip WHILE other kernels run (MI355X_MICROARCH.md, DVFS item 6): one wave on its own stream
// sleeps for duration_ms and stamps s_memtime (shader cycles) and s_memrealtime (100 MHz) at both ends.  bench.py starts
// it at the head of the timed region, so the VALU ceiling is priced at the clock of the run, not at the nominal 2.4 GHz.
namespace {

__global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long* out, unsigned long long ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    unsigned long long t = t0;
    // ends when the host raises out[2] (bl_clock_probe_finish) or, at the latest, after `ticks` x 10 ns: a wall-clock bound that
    // holds whatever else happens
    while (t - t0 < ticks && __hip_atomic_load(&out[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
        __builtin_amdgcn_s_sleep(127);
        t = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) {
        out[0] = c1 - c0;
        out[1] = t - t0;
    }
}

}  // namespace

struct bl_clock_probe {
    int device;
    hipStream_t stream;
    unsigned long long* pinned;  // [0] cycles, [1] 10-ns ticks, [2] stop request (host -> device)
};

extern "C" int bl_clock_probe_start(bl_ctx* ctx, uint32_t duration_ms, bl_clock_probe** out)
{
    if (!ctx || !out || duration_ms == 0 || duration_ms > 5000) return bl_set_error(BL_ERR_INVALID, "clock probe: need a context and 1..5000 ms");
    *out = nullptr;
    BLH_TRY(hipSetDevice(bl_ctx_device(ctx)));
    bl_clock_probe* p = new (std::nothrow) bl_clock_probe{bl_ctx_device(ctx), nullptr, nullptr};
    if (!p) return bl_set_error(BL_ERR_OOM, "host allocation failed");
    hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&p->pinned), 4 * sizeof(unsigned long long), hipHostMallocDefault);
    if (e == hipSuccess) {
        p->pinned[0] = p->pinned[1] = p->pinned[2] = 0;
        hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, p->stream, p->pinned, (unsigned long long)duration_ms * 100000ull);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        if (p->pinned) (void)hipHostFree(p->pinned);
        if (p->stream) (void)hipStreamDestroy(p->stream);
        delete p;
        return bl_set_error(BL_ERR_HIP, hipGetErrorString(e));
    }
    *out = p;
    return BL_OK;
}

extern "C" int bl_clock_probe_finish(bl_clock_probe* p, double* shader_ghz)
{
    if (!p) return bl_set_error(BL_ERR_INVALID, "probe is NULL");
    (void)hipSetDevice(p->device);
    __atomic_store_n(&p->pinned[2], 1ull, __ATOMIC_RELEASE);  // stop now: the probe must never outlive what it measures (a device-wide
                                                              // synchronise would otherwise wait for it)
    hipError_t e = hipStreamSynchronize(p->stream);
    const double cycles = (double)p->pinned[0], ticks = (double)p->pinned[1];
    (void)hipHostFree(p->pinned);
    (void)hipStreamDestroy(p->stream);
    delete p;
    if (e != hipSuccess) return bl_set_error(BL_ERR_HIP, hipGetErrorString(e));
    if (shader_ghz) *shader_ghz = ticks > 0 ? cycles / ticks * 0.1 : 0.0;
    return BL_OK;
}
