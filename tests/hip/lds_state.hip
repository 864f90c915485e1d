// Diagnostics for tests/lds_state.py (liblanemap_diag.so, never part of the product library): set and read back the contents of every
// CU's LDS, and a deliberately leaky kernel as the negative control of the LDS-state tests.  gfx950: 160 KB of LDS per CU, so a
// workgroup that asks for all of it has a CU's LDS to itself and the dispatcher has to spread a grid of them over the CUs.
#include "common.h"

static constexpr int LDS_WORDS = 163840 / 4;
static constexpr int LDS_THREADS = 256;
static constexpr int FILL_PASSES = 4;

// Volatile accesses through a generic pointer compile to flat_load / flat_store (address-space inference leaves volatile alone), and
// non-volatile loads from LDS that the kernel never stored may be folded away: the pointers carry the LDS address space themselves.
typedef volatile __attribute__((address_space(3))) unsigned* lds_u32_ptr;
typedef volatile __attribute__((address_space(3))) float* lds_f32_ptr;

__global__ __launch_bounds__(LDS_THREADS) void lds_fill_kernel(unsigned word) {
    extern __shared__ unsigned lds_raw[];
    const lds_u32_ptr lds_all = (lds_u32_ptr)lds_raw;
    for (int pass = 0; pass < FILL_PASSES; ++pass) {
        for (int i = threadIdx.x; i < LDS_WORDS; i += LDS_THREADS) lds_all[i] = word;
        __syncthreads();
    }
}

__global__ __launch_bounds__(LDS_THREADS) void lds_probe_kernel(unsigned word, unsigned long long* mismatches) {
    extern __shared__ unsigned lds_raw[];
    const lds_u32_ptr lds_all = (lds_u32_ptr)lds_raw;
    unsigned bad = 0;
    for (int i = threadIdx.x; i < LDS_WORDS; i += LDS_THREADS) bad += (lds_all[i] != word) ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off);
    // the 160 KB leave no room for a counter of its own: the four wave sums meet in word 0, which gets its old value back at the end so
    // that a probe leaves LDS as it found it
    const unsigned keep = lds_all[0];
    __syncthreads();                       // every read of the old contents is done before word 0 is borrowed
    if (threadIdx.x == 0) lds_all[0] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&lds_raw[0], bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = lds_all[0];
        lds_all[0] = keep;
        if (total) atomicAdd(mismatches, (unsigned long long)total);
    }
}

// y[i] = x[i] + 0 * pad, where pad is column 32 of a [8][33] staging tile that nothing writes: exact after finite LDS, NaN after NaN / Inf
__global__ __launch_bounds__(LDS_THREADS) void lds_leaky_kernel(const float* __restrict__ x, float* __restrict__ y, int n) {
    __shared__ float tile[8 * 33];
    const lds_f32_ptr t = (lds_f32_ptr)tile;
    const int r = threadIdx.x >> 5, c = threadIdx.x & 31;
    const long i = (long)blockIdx.x * LDS_THREADS + threadIdx.x;
    if (i < n) t[r * 33 + c] = x[i];
    __syncthreads();
    if (i < n) y[i] = t[r * 33 + c] + 0.f * t[r * 33 + 32];
}

static int lds_grid(int workgroups, int* grid) {
    if (workgroups <= 0) {
        int dev = 0, cus = 0;
        LM_HIP(hipGetDevice(&dev));
        LM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        workgroups = 4 * cus;
    }
    *grid = workgroups;
    return LM_OK;
}

LM_API int lmd_lds_fill(void* stream, unsigned word, int workgroups) {
    int grid = 0;
    if (int rc = lds_grid(workgroups, &grid)) return rc;
    const size_t bytes = (size_t)LDS_WORDS * 4;
    if (int rc = lm_ensure_dynamic_lds((const void*)lds_fill_kernel, bytes)) return rc;
    hipLaunchKernelGGL(lds_fill_kernel, dim3(grid), dim3(LDS_THREADS), bytes, (hipStream_t)stream, word);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

LM_API int lmd_lds_probe(void* stream, unsigned word, unsigned long long* mismatches, int workgroups) {
    LM_REQUIRE(mismatches, "lmd_lds_probe: null counter");
    int grid = 0;
    if (int rc = lds_grid(workgroups, &grid)) return rc;
    const size_t bytes = (size_t)LDS_WORDS * 4;
    if (int rc = lm_ensure_dynamic_lds((const void*)lds_probe_kernel, bytes)) return rc;
    hipLaunchKernelGGL(lds_probe_kernel, dim3(grid), dim3(LDS_THREADS), bytes, (hipStream_t)stream, word, mismatches);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

LM_API int lmd_lds_leaky(void* stream, const float* x, float* y, int n) {
    LM_REQUIRE(x && y && n >= 0, "lmd_lds_leaky: null buffer or negative n");
    if (n == 0) return LM_OK;
    hipLaunchKernelGGL(lds_leaky_kernel, dim3(lm_cdiv(n, LDS_THREADS)), dim3(LDS_THREADS), 0, (hipStream_t)stream, x, y, n);
    LM_LAUNCH_CHECK();
    return LM_OK;
}
