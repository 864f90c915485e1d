// Shared helpers for the lanemap_hip C-ABI library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

// The C ABI - every entry's prototype, the structs that cross it, the LM_OK .. and LM_ACT_.. codes - has one definition, the public
// header.  A definition below that disagrees with its prototype does not compile.
#include "../../include/lanemap_hip.h"

#define LM_API extern "C" __attribute__((visibility("default")))   // on the definition: exported; the prototype is the header's

void lm_set_error(const char* fmt, ...);
int lm_ensure_dynamic_lds(const void* kernel, size_t bytes);   // per device and kernel, thread-safe (errors.cpp)

#define LM_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            lm_set_error(__VA_ARGS__);   \
            return LM_ERR_ARG;           \
        }                                \
    } while (0)

#define LM_HIP(expr)                                                                  \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            lm_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return LM_ERR_HIP;                                                        \
        }                                                                             \
    } while (0)

#define LM_LAUNCH_CHECK() LM_HIP(hipGetLastError())

// Streams and graphs.  An entry enqueues on the stream it is given and on nothing else.  One that only launches kernels and enqueues
// device-to-device copies may be captured into a HIP graph; it zeroes with lm_zero_async below, never with hipMemsetAsync (captured
// memset nodes replay wrongly).  One that copies call-local HOST memory to the device
// (a captured copy node would keep the address of memory that the next call overwrites) or synchronises the stream (which invalidates
// a capture) must not be: LM_NO_CAPTURE is its FIRST statement, before anything touches the stream.  Anything but "not capturing" - a
// failed query included - is LM_ERR_ARG with the entry's name and the reason; the capture itself stays valid.
static inline int lm_refuse_capture(void* stream, const char* who, const char* why) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusActive;
    const hipError_t e = hipStreamIsCapturing((hipStream_t)stream, &st);
    if (e == hipSuccess && st == hipStreamCaptureStatusNone) return LM_OK;
    (void)hipGetLastError();                 // the failed query must not surface at a later launch check
    if (e != hipSuccess)
        lm_set_error("%s: must not be called while a stream is being captured (%s); the capture status of its stream could not be queried: %s",
                     who, why, hipGetErrorString(e));
    else
        lm_set_error("%s: must not be called on a stream that is being captured into a graph: %s", who, why);
    return LM_ERR_ARG;
}
#define LM_NO_CAPTURE(stream, who, why)                                  \
    do {                                                                 \
        if (int nc_ = lm_refuse_capture((stream), (who), (why))) return nc_; \
    } while (0)
#define LM_WHY_HOST_COPY "it copies call-local host memory to the device"
#define LM_WHY_HOST_COPY_SYNC "it copies call-local host memory to the device and synchronises the stream"

static inline int lm_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline long lm_cdivl(long a, long b) { return (a + b - 1) / b; }
static inline size_t lm_align256(size_t v) { return (v + 255) / 256 * 256; }   // workspace segments start on 256 bytes

#ifdef __HIPCC__
// Zeroing inside an entry that may be captured: a kernel, never hipMemsetAsync.  Replays of a captured memset node were seen to leave
// what the previous replay had put there, or to write other bytes than zeros (tests/test_gpu_streams.py: the replays of
// lm_rowref_decode, lm_tile_gap_hist, lm_sparse_conv_outputs, lm_sparse_to_dense_nhwc and lm_las_label_records over outputs
// pre-filled with 0xFF); a kernel node replays like every other launch.  Any address, any byte count: 16-byte stores over the
// aligned middle, single bytes before and behind it.
namespace {
__global__ __launch_bounds__(256) __attribute__((unused)) void lm_zero_kernel(unsigned char* __restrict__ p, size_t head, size_t n16,
                                                                               size_t tail) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) reinterpret_cast<uint4*>(p + head)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (i < head) p[i] = 0;
    if (i < tail) p[head + 16 * n16 + i] = 0;
}
}  // namespace
static inline __attribute__((unused)) hipError_t lm_zero_async(void* ptr, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    unsigned char* p = (unsigned char*)ptr;
    size_t head = (16 - ((uintptr_t)p & 15)) & 15;
    if (head > bytes) head = bytes;
    const size_t n16 = (bytes - head) / 16, tail = bytes - head - 16 * n16;         // head + 16 n16 + tail == bytes, head, tail < 16
    const size_t threads = n16 > 16 ? n16 : 16;
    hipLaunchKernelGGL(lm_zero_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, p, head, n16, tail);
    return hipGetLastError();
}
// GroupNorm(C,C) + ReLU + bilinear (align_corners=True) building blocks with a FIXED operation order: `#pragma clang fp contract(off)`
// keeps the compiler from fusing their multiplies and adds differently in different kernels (HIP's __fmul_rn / __fadd_rn are plain
// operators and do not prevent that), explicit fmaf where a fused multiply-add is wanted.  The same bits in every kernel that uses
// them (norm_resize.hip, the fused Winograd input transform, the bilinear residual of the convolution epilogue).
// Source index follows ATen: scale = (in-1)/(out-1) in fp32, src = scale*dst, i0 = floor(src), i1 = min(i0+1, in-1), w1 = src - i0.
// (lm_bilin_axis_scaled: the same with the scale computed once by the caller - on the host the IEEE single-precision quotient is the
// same float, hipcc divides correctly rounded by default)
__device__ __forceinline__ void lm_bilin_axis_scaled(int o, int in, float scale, int& i0, int& i1, float& w0, float& w1) {
#pragma clang fp contract(off)
    const float src = scale * (float)o;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    w1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    w0 = 1.f - w1;
}
__device__ __forceinline__ void lm_bilin_axis(int o, int in, int out, int& i0, int& i1, float& w0, float& w1) {
#pragma clang fp contract(off)
    const float scale = (out > 1) ? (float)(in - 1) / (float)(out - 1) : 0.f;
    lm_bilin_axis_scaled(o, in, scale, i0, i1, w0, w1);
}
#endif
// Division of n < 2^31 by an invariant divisor d >= 1 (Granlund & Montgomery, round-up variant): q = (mulhi(n, mul) + n) >> sh with
// sh = ceil(log2 d), mul = floor(2^32 (2^sh - d) / d) + 1; the sum stays below 2^32 for n < 2^31.  3 VALU instructions instead of the
// ~25 of a 32-bit (or ~60 of a 64-bit) division by a run-time value.
struct LmFastDiv {
    unsigned d, mul, sh;
};
static inline LmFastDiv lm_fastdiv_make(unsigned d) {
    LmFastDiv f;
    f.d = d;
    f.sh = 0;
    while ((1ull << f.sh) < d) ++f.sh;
    f.mul = (unsigned)((((1ull << f.sh) - d) << 32) / d + 1);
    return f;
}
#ifdef __HIPCC__
__device__ __forceinline__ unsigned lm_fastdiv(unsigned n, const LmFastDiv& f) { return (__umulhi(n, f.mul) + n) >> f.sh; }
__device__ __forceinline__ void lm_gn_affine(float mean, float rstd, float gamma, float beta, float& a, float& g) {
#pragma clang fp contract(off)
    a = rstd * gamma;                        // gn(v) = v * a + g
    g = __builtin_fmaf(-mean, a, beta);
}
__device__ __forceinline__ float lm_gn_relu(float v, float a, float g) { return fmaxf(__builtin_fmaf(v, a, g), 0.f); }
__device__ __forceinline__ float lm_bilerp(float v00, float v01, float v10, float v11, float wy0, float wy1, float wx0, float wx1) {
#pragma clang fp contract(off)
    const float top = wx0 * v00 + wx1 * v01;
    const float bot = wx0 * v10 + wx1 * v11;
    return wy0 * top + wy1 * bot;
}
#endif
