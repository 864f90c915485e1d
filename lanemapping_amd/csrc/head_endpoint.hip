// ColumnProposal2 with heads.endp_mode = 'endpoint' (heads/polyline_fpn_vit_vertex_2.py:254-260, :371-373): the head's own endpoint map
//
//   endpoint = conv3x3(bn(relu(conv3x3(relu(cat(up(col), x_endp)); W1) + b1)); W2) + b2        at H x W (1152 x 1152)
//
// in ONE kernel.  The reference builds cat(up(col), x_endp) as a [B,17,H,W] tensor (90 MB per tile, twice with the ReLU); here a
// workgroup of 256 threads owns one EP_T x EP_T output tile and keeps everything between the low-resolution `col` and the final map in
// LDS and registers:
//   1. the low-resolution patch of the 16 col channels that the tile and its 2-pixel halo interpolate from -> LDS (EP_PATCH^2 pixels; a
//      tile whose patch is larger - a down-sampling call - reads col from global memory instead, same arithmetic);
//   2. per chunk of 4 input channels (then x_endp alone): a = relu(bilinear(col)) on the (EP_T + 4)^2 region -> LDS, zero outside the
//      image (the padding of conv 1); conv 1 accumulates its 4 output channels for a 1 x 5 strip of the (EP_T + 2)^2 region per thread;
//   3. t = s * relu(acc + b1) + beta, ZERO outside the image (the padding of conv 2: the BatchNorm shift must not leak into it, which
//      is why it is folded into neither convolution) -> LDS, over the buffer of step 2;
//   4. conv 2 -> 1 x 4 outputs per thread, the only global write.
// Exact fp32 FMAs in a fixed order (channel, ky, kx): every output is the same sequence of operations wherever its tile lies and
// whatever B is.  The interpolation is lm_bilin_axis / lm_bilerp of common.h: the bits of lm_upsample_bilinear_nhwc.
#include "common.h"

namespace {

constexpr int EP_T = 32;                 // output tile edge
constexpr int EP_A = EP_T + 4;           // rows of the conv-1 input region (2-pixel halo)
constexpr int EP_AS = EP_A + 1;          // its columns and row stride: one more column feeds the junk end of the last 1 x 5 strip
constexpr int EP_R = EP_T + 2;           // conv-1 output region (1-pixel halo)
constexpr int EP_RS = EP_R + 1;          // its row stride
constexpr int EP_STRIPS = 7;             // 1 x 5 strips per conv-1 row (35 >= EP_R columns)
constexpr int EP_PATCH = 12;             // low-resolution patch edge held in LDS: 36 outputs at scale 287 / 1151 span 10 source rows
constexpr int EP_CIN = 16;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct EpAxis {            // per row / column of the conv-1 input region: source indices (i0 < 0: outside the image) and weights
    int i0[EP_AS], i1[EP_AS];
    float w0[EP_AS], w1[EP_AS];
};

// conv 1 over NCH channels of the materialised region `a` [NCH][EP_A][EP_AS] for the strip (row, col0 .. col0 + 4);
// w1p = [c][ky][kx][4 outputs] of these channels
template <int NCH>
__device__ __forceinline__ void ep_conv1_chunk(const float* a, const float* __restrict__ w1p, int row, int col0, f32x2 (&acc)[5][2]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const float* ar = a + (c * EP_A + row + ky) * EP_AS + col0;
            float v[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) v[j] = ar[j];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float* wq = w1p + ((c * 3 + ky) * 3 + kx) * 4;
                const f32x2 w01 = {wq[0], wq[1]}, w23 = {wq[2], wq[3]};
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const f32x2 vv = {v[j + kx], v[j + kx]};
                    acc[j][0] = __builtin_elementwise_fma(vv, w01, acc[j][0]);
                    acc[j][1] = __builtin_elementwise_fma(vv, w23, acc[j][1]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void head_endpoint_kernel(const float* __restrict__ col, int ldc, const float* __restrict__ x_endp,
                                                            const float* __restrict__ w1p, const float* __restrict__ b1,
                                                            const float* __restrict__ bn_s, const float* __restrict__ bn_b,
                                                            const float* __restrict__ w2, const float* __restrict__ b2,
                                                            float* __restrict__ out, int h, int w, int H, int W) {
    __shared__ __attribute__((aligned(16))) float patch[EP_PATCH * EP_PATCH * EP_CIN];
    __shared__ float abuf[4 * EP_A * EP_AS];          // step 2: a [4][EP_A][EP_AS]; step 3: t [4][EP_R][EP_RS]
    __shared__ EpAxis ay, ax;
    static_assert(4 * EP_R * EP_RS <= 4 * EP_A * EP_AS, "t must fit the buffer of a");

    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int oy0 = blockIdx.y * EP_T, ox0 = blockIdx.x * EP_T;

    // interpolation tables of the region's rows and columns (image row oy0 - 2 + r, column ox0 - 2 + q)
    if (tid < EP_AS) {
        const int g = oy0 - 2 + tid;
        int i0 = -1, i1 = -1;
        float f0 = 0.f, f1 = 0.f;
        if (g >= 0 && g < H) lm_bilin_axis(g, h, H, i0, i1, f0, f1);
        ay.i0[tid] = i0, ay.i1[tid] = i1, ay.w0[tid] = f0, ay.w1[tid] = f1;
    } else if (tid >= 64 && tid < 64 + EP_AS) {
        const int q = tid - 64, g = ox0 - 2 + q;
        int i0 = -1, i1 = -1;
        float f0 = 0.f, f1 = 0.f;
        if (g >= 0 && g < W) lm_bilin_axis(g, w, W, i0, i1, f0, f1);
        ax.i0[q] = i0, ax.i1[q] = i1, ax.w0[q] = f0, ax.w1[q] = f1;
    }
    // low-resolution extent of the region (the source index grows with the destination index): every thread computes the same values
    int sy_lo, sy_hi, sx_lo, sx_hi;
    {
        int i0, i1;
        float f0, f1;
        lm_bilin_axis(max(oy0 - 2, 0), h, H, i0, i1, f0, f1);
        sy_lo = i0;
        lm_bilin_axis(min(oy0 - 2 + EP_AS - 1, H - 1), h, H, i0, i1, f0, f1);
        sy_hi = i1;
        lm_bilin_axis(max(ox0 - 2, 0), w, W, i0, i1, f0, f1);
        sx_lo = i0;
        lm_bilin_axis(min(ox0 - 2 + EP_AS - 1, W - 1), w, W, i0, i1, f0, f1);
        sx_hi = i1;
    }
    const int pr = sy_hi - sy_lo + 1, pc = sx_hi - sx_lo + 1;
    const bool staged = pr <= EP_PATCH && pc <= EP_PATCH;
    const float* colb = col + (long)b * h * w * ldc;
    if (staged) {
        for (int i = tid; i < pr * pc * EP_CIN; i += 256) {
            const int c = i % EP_CIN, p = i / EP_CIN;
            const int px = p % pc, py = p / pc;
            patch[(py * EP_PATCH + px) * EP_CIN + c] = colb[((long)(sy_lo + py) * w + (sx_lo + px)) * ldc + c];
        }
    }

    // the strip of conv-1 outputs this thread accumulates: region row `row`, columns col0 .. col0 + 4
    const int row = tid / EP_STRIPS, col0 = (tid % EP_STRIPS) * 5;
    const bool conv1_on = row < EP_R;
    f32x2 acc[5][2];
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[j][0] = acc[j][1] = f32x2{0.f, 0.f};

    for (int chunk = 0; chunk < 5; ++chunk) {
        __syncthreads();              // tables and patch written (chunk 0); conv 1 of the previous chunk has read abuf
        if (chunk < 4) {
            const int c0 = chunk * 4;
            for (int i = tid; i < EP_A * EP_AS; i += 256) {
                const int r = i / EP_AS, q = i % EP_AS;
                const int y0 = ay.i0[r], x0 = ax.i0[q];
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if (y0 >= 0 && x0 >= 0) {
                    const int y1 = ay.i1[r], x1 = ax.i1[q];
                    const float wy0 = ay.w0[r], wy1 = ay.w1[r], wx0 = ax.w0[q], wx1 = ax.w1[q];
                    f32x4 v00, v01, v10, v11;
                    if (staged) {
                        const float* pp = patch + c0;
                        v00 = *reinterpret_cast<const f32x4*>(pp + ((y0 - sy_lo) * EP_PATCH + (x0 - sx_lo)) * EP_CIN);
                        v01 = *reinterpret_cast<const f32x4*>(pp + ((y0 - sy_lo) * EP_PATCH + (x1 - sx_lo)) * EP_CIN);
                        v10 = *reinterpret_cast<const f32x4*>(pp + ((y1 - sy_lo) * EP_PATCH + (x0 - sx_lo)) * EP_CIN);
                        v11 = *reinterpret_cast<const f32x4*>(pp + ((y1 - sy_lo) * EP_PATCH + (x1 - sx_lo)) * EP_CIN);
                    } else {
                        const float* p00 = colb + ((long)y0 * w + x0) * ldc + c0;
                        const float* p01 = colb + ((long)y0 * w + x1) * ldc + c0;
                        const float* p10 = colb + ((long)y1 * w + x0) * ldc + c0;
                        const float* p11 = colb + ((long)y1 * w + x1) * ldc + c0;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v00[e] = p00[e], v01[e] = p01[e], v10[e] = p10[e], v11[e] = p11[e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = fmaxf(lm_bilerp(v00[e], v01[e], v10[e], v11[e], wy0, wy1, wx0, wx1), 0.f);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) abuf[e * EP_A * EP_AS + i] = o[e];
            }
        } else {
            const float* xb = x_endp + (long)b * H * W;
            for (int i = tid; i < EP_A * EP_AS; i += 256) {
                const int r = i / EP_AS, q = i % EP_AS;
                const int gy = oy0 - 2 + r, gx = ox0 - 2 + q;
                float o = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) o = fmaxf(xb[(long)gy * W + gx], 0.f);
                abuf[i] = o;
            }
        }
        __syncthreads();
        if (conv1_on) {
            if (chunk < 4)
                ep_conv1_chunk<4>(abuf, w1p + chunk * 4 * 36, row, col0, acc);
            else
                ep_conv1_chunk<1>(abuf, w1p + 16 * 36, row, col0, acc);
        }
    }
    __syncthreads();                  // every strip has read the last a: abuf becomes t
    if (conv1_on) {
        const int gy = oy0 - 1 + row;
        const f32x2 bb[2] = {{b1[0], b1[1]}, {b1[2], b1[3]}};
        const f32x2 ss[2] = {{bn_s[0], bn_s[1]}, {bn_s[2], bn_s[3]}};
        const f32x2 sh[2] = {{bn_b[0], bn_b[1]}, {bn_b[2], bn_b[3]}};
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int q = col0 + j, gx = ox0 - 1 + q;
            if (q >= EP_R) continue;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const float r = fmaxf(acc[j][p][e] + bb[p][e], 0.f);
                    abuf[((2 * p + e) * EP_R + row) * EP_RS + q] = in ? __builtin_fmaf(ss[p][e], r, sh[p][e]) : 0.f;
                }
            }
        }
    }
    __syncthreads();
    // conv 2: output row orow, columns oc0 .. oc0 + 3 of the tile
    const int orow = tid / (EP_T / 4), oc0 = (tid % (EP_T / 4)) * 4;
    const int gy = oy0 + orow;
    if (gy >= H) return;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const float* tr = abuf + (c * EP_R + orow + ky) * EP_RS + oc0;
            float v[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = tr[j];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float wk = w2[(c * 3 + ky) * 3 + kx];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = __builtin_fmaf(v[j + kx], wk, o[j]);
            }
        }
    }
    const float bias = b2[0];
    float* orow_p = out + ((long)b * H + gy) * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gx = ox0 + oc0 + j;
        if (gx < W) orow_p[gx] = o[j] + bias;
    }
}

}  // namespace

LM_API int lm_head_endpoint_tile() { return EP_T; }

LM_API int lm_head_endpoint(void* hip_stream, const float* col, int ldc, const float* x_endp, const float* w1p, const float* b1,
                            const float* bn_scale, const float* bn_shift, const float* w2, const float* b2, float* out, int B, int h,
                            int w, int H, int W) {
    LM_REQUIRE(col && x_endp && w1p && b1 && bn_scale && bn_shift && w2 && b2 && out, "head_endpoint: null pointer");
    LM_REQUIRE(ldc >= EP_CIN, "head_endpoint: ldc=%d is below the %d channels of col", ldc, EP_CIN);
    LM_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "head_endpoint: bad sizes B=%d h=%d w=%d H=%d W=%d", B, h, w, H, W);
    LM_REQUIRE(B <= 65535 && lm_cdiv(H, EP_T) <= 65535, "head_endpoint: grid too large (B=%d, H=%d)", B, H);
    hipLaunchKernelGGL(head_endpoint_kernel, dim3(lm_cdiv(W, EP_T), lm_cdiv(H, EP_T), B), dim3(256), 0, (hipStream_t)hip_stream,
                       col, ldc, x_endp, w1p, b1, bn_scale, bn_shift, w2, b2, out, h, w, H, W);
    LM_LAUNCH_CHECK();
    return LM_OK;
}
