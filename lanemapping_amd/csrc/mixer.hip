// MLP-Mixer token mixing on the CDNA4 matrix cores, exact fp32.
//
//   Y[b][m][n] = act( sum_k W[m][k] * X[b][k][n] + bias[m] ) (+ R[b][m][n])
//
// The weight is the LEFT operand: one Conv1d(K -> M, kernel 1) over the token axis, applied to every channel n of every batch
// element b (the token-mixing FeedForward of MixSegNet, baseline/models/backbone/mixsegnet.py:24-31,55-58: K, M = 324 -> 1296 and
// 1296 -> 324 over the 512 channels).  X[b] is read in the layout the rest of the backbone keeps, [B*K][N] row-major (token rows,
// channel vectors contiguous): no transpose pass, no padded copy.  The weight is packed once at load as Wt[Kp][ldw] = W^T, zero
// padded to Kp = K rounded up to BK and ldw >= M rounded up to 128, so its tile loads never need a mask.  The K tail of X (K % BK)
// is masked at load: a workgroup never reads past its batch element.
//
// Design (gfx950): 256 threads = 4 waves, each wave owns a WM x WN output tile of 32 x 32 accumulators driven by
// v_mfma_f32_32x32x2_f32 (exact f32: each output is the k-ascending fmaf chain, whatever the tile shape or batch size).  Both
// operands sit in LDS k-major ([BK][BM] of Wt, [BK][BN] of X), so an MFMA operand is one ds_read_b32 per lane with the 32 lanes of
// a half-wave on 32 consecutive floats (conflict-free; lanes l and l + 32 are serviced apart).  The next k-slab is loaded to
// registers (16-byte global loads, coalesced along n and m) under the MFMAs of the current one and written to the other LDS buffer:
// one barrier per slab.  Epilogue straight from the accumulator layout: a half-wave stores 32 consecutive channels of one row.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int BK = 16;          // k-slab (tokens): 324 = 20.25 slabs, 1296 = 81
constexpr int NT = 256;         // threads per workgroup
constexpr int MPAD = 128;       // the packed weight's M padding: a multiple of every BM

struct MixParams {
    const float* x; const float* wt; const float* bias; const float* res; float* y;
    int B, M, K, N, ldw, act;
};

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(NT) void token_mix_kernel(MixParams p) {
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    static_assert((BM / WM) * (BN / WN) * 64 == NT, "four waves per workgroup");
    constexpr int A_LOADS = BK * BM / 4 / NT;    // float4 per thread per slab
    constexpr int B_LOADS = BK * BN / 4 / NT;
    static_assert(A_LOADS >= 1 && B_LOADS >= 1 && BM % 4 == 0 && BN % 4 == 0, "whole float4 loads");
    __shared__ __attribute__((aligned(16))) float As[2][BK][BM];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm0 = (wave / WAVES_N) * WM;
    const int wn0 = (wave % WAVES_N) * WN;
    const int n0 = blockIdx.x * BN;
    const int m0 = blockIdx.y * BM;
    const int b = blockIdx.z;
    const float* xb = p.x + (long)b * p.K * p.N;

    // load slots: thread tid moves float4 number tid + i * NT of the slab ([BK][BM] resp. [BK][BN], row-major)
    float* const Af = &As[0][0][0];
    float* const Bf = &Bs[0][0][0];
    f32x4 ra[A_LOADS], rb[B_LOADS];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            const int e = (tid + i * NT) * 4, r = e / BM, c = e % BM;
            ra[i] = *reinterpret_cast<const f32x4*>(p.wt + (long)(k0 + r) * p.ldw + m0 + c);    // zero padded: always in bounds
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const int e = (tid + i * NT) * 4, r = e / BN, c = e % BN;
            const int k = k0 + r, n = n0 + c;
            rb[i] = (k < p.K && n < p.N) ? *reinterpret_cast<const f32x4*>(xb + (long)k * p.N + n) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) *reinterpret_cast<f32x4*>(Af + buf * BK * BM + (tid + i * NT) * 4) = ra[i];
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) *reinterpret_cast<f32x4*>(Bf + buf * BK * BN + (tid + i * NT) * 4) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int KT = (p.K + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    const int frow = lane & 31, fk = lane >> 5;        // operand lane map of 32x32x2: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
    for (int kt = 0; kt < KT; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < KT) gload((kt + 1) * BK);         // next slab in flight under this slab's MFMAs
        const float* Ab = Af + buf * BK * BM + fk * BM + wm0 + frow;
        const float* Bb = Bf + buf * BK * BN + fk * BN + wn0 + frow;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = Ab[kk * BM + i * 32];
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = Bb[kk * BN + j * 32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < KT) lstore(buf ^ 1);              // the other buffer was last read before the previous barrier
        __syncthreads();
    }

    // epilogue: accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 block
    const int half = lane >> 5;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn0 + j * 32 + frow;
        if (n >= p.N) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m >= p.M) continue;
                const long o = ((long)b * p.M + m) * p.N + n;
                float v = acc[i][j][r] + p.bias[m];
                if (p.act == LM_ACT_GELU) v = gelu_erf(v);
                if (p.res) v += p.res[o];
                p.y[o] = v;
            }
    }
}

template <int BM, int BN, int WM, int WN>
int launch(const MixParams& p, hipStream_t s) {
    const dim3 grid(lm_cdiv(p.N, BN), lm_cdiv(p.M, BM), p.B);
    hipLaunchKernelGGL((token_mix_kernel<BM, BN, WM, WN>), grid, dim3(NT), 0, s, p);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

}  // namespace

// y[b] = act(W x[b] + bias) (+ res[b]) for b < B: x [B*K][N], res / y [B*M][N] row-major (N % 4 == 0, 16-byte aligned);
// wt = W^T zero padded to [ceil(K / 16) * 16][ldw], ldw >= ceil(M / 128) * 128; bias [M]; act LM_ACT_NONE or LM_ACT_GELU.
LM_API int lm_token_mix_mfma_f32(void* stream, const float* x, const float* wt, int ldw, const float* bias, const float* res, float* y,
                                 int B, int M, int K, int N, int act) {
    LM_REQUIRE(x && wt && bias && y, "token_mix: null pointer");
    LM_REQUIRE(B >= 1 && M >= 1 && K >= 1 && N >= 4 && B <= 65535, "token_mix: bad shape B=%d M=%d K=%d N=%d", B, M, K, N);
    LM_REQUIRE(N % 4 == 0, "token_mix: N=%d must be a multiple of 4", N);
    LM_REQUIRE(ldw % MPAD == 0 && ldw >= M, "token_mix: ldw=%d must be M=%d rounded up to a multiple of %d", ldw, M, MPAD);
    LM_REQUIRE(act == LM_ACT_NONE || act == LM_ACT_GELU, "token_mix: act=%d (none or gelu)", act);
    LM_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)wt & 15) == 0, "token_mix: x and wt must be 16-byte aligned");
    LM_REQUIRE((long)B * (M > K ? M : K) * N < (1L << 31) && (long)(K + BK) * ldw < (1L << 31), "token_mix: problem too large");
    MixParams p;
    p.x = x; p.wt = wt; p.bias = bias; p.res = res; p.y = y;
    p.B = B; p.M = M; p.K = K; p.N = N; p.ldw = ldw; p.act = act;
    hipStream_t s = (hipStream_t)stream;
    // under two rounds of 128 x 128 tiles on the 256 CUs (the 324-row GEMM: 192 tiles at B = 16) -> 64 x 64 tiles, 4x the workgroups
    // (the k order of an output does not depend on the tile: same bits either way)
    const long big_blocks = (long)lm_cdiv(M, 128) * lm_cdiv(N, 128) * B;
    if (big_blocks < 512) return launch<64, 64, 32, 32>(p, s);
    return launch<128, 128, 64, 64>(p, s);
}
