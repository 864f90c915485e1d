// Normalisation and resampling kernels (HBM-bound, NHWC fp32, float4 per lane).
//
//  lm_gn_stats                : per-(b,c) mean / rstd of GroupNorm(C groups == C channels)
//                               (postprojector.py:512-515), deterministic two-level fp64 reduction
//  lm_gn_relu_upsample        : y (=|+=) bilinear_align_corners(relu(gn(x)))  -> fuses the
//                               `_upsample(F.relu(gn(conv(..))))` and `s2+s3+s4` steps (postprojector.py:615-651)
//  lm_gn_relu_upsample_sum    : y = ((t0 + t1) + t2) of up to three such terms in one pass (the `s2 + s3 + s4` sum)
//  lm_upsample_bilinear_nhwc  : F.interpolate(mode='bilinear', align_corners=True) (+ optional add)
//                               (postprojector.py:541-561; heads/polyline_fpn_vit_vertex_2.py:298-300)
//  lm_upsample_bilinear_to_chw: same, NHWC source -> planar [B,C,Ho,Wo] destination (bi_seg / endp maps)
//  lm_layernorm_rows          : nn.LayerNorm(dim) eps 1e-5 over rows (vitsegnet.py:20-26), D % 32 == 0 up to 4096 but 768
//  lm_unpatchify              : 'b (h w) (p1 p2 c) -> b c (h p1) (w p2)' into NHWC (vitsegnet.py:180)
//
// Bilinear source index follows ATen: scale = (in-1)/(out-1) in fp32, src = scale*dst,
// i0 = floor(src), i1 = min(i0+1, in-1), w1 = src - i0, w0 = 1 - w1.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// ----------------------------------------------------------------------------- shared steps of the GN + ReLU + bilinear kernels
// (the four kernels that normalise and blend agree bit for bit because they run these, not copies of them)
// Per-channel affine of the normalisation, v * a + g, of a channel quad: s0, s1 = its four (mean, rstd) pairs as two 16-byte loads,
// gm / bt = gamma / beta of the same channels.  Loading is the caller's: gn_relu_upsample_sum_kernel loads first and computes later.
__device__ __forceinline__ void gn_affine4(f32x4 s0, f32x4 s1, f32x4 gm, f32x4 bt, f32x4& a, f32x4& g) {
    const float mean[4] = {s0[0], s0[2], s1[0], s1[2]}, rstd[4] = {s0[1], s0[3], s1[1], s1[3]};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float ae, ge;
        lm_gn_affine(mean[e], rstd[e], gm[e], bt[e], ae, ge);
        a[e] = ae;
        g[e] = ge;
    }
}
// the same from the statistics of (b, c): st = stats + (b * C + c) * 2
__device__ __forceinline__ void gn_affine4_at(const float* st, f32x4 gm, f32x4 bt, f32x4& a, f32x4& g) {
    gn_affine4(reinterpret_cast<const f32x4*>(st)[0], reinterpret_cast<const f32x4*>(st)[1], gm, bt, a, g);
}
__device__ __forceinline__ f32x4 gn_relu4(f32x4 v, f32x4 a, f32x4 g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = lm_gn_relu(v[e], a[e], g[e]);
    return v;
}
__device__ __forceinline__ f32x4 bilerp4(f32x4 v00, f32x4 v01, f32x4 v10, f32x4 v11, float wy0, float wy1, float wx0, float wx1) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = lm_bilerp(v00[e], v01[e], v10[e], v11[e], wy0, wy1, wx0, wx1);
    return o;
}
// flat index of an output channel quad of [B][Ho][Wo][C / 4] -> first channel, column, row, image
__device__ __forceinline__ void decode_quad(long i, int C, int Ho, int Wo, int& c, int& ox, int& oy, int& b) {
    const int c4n = C / 4;
    c = (int)(i % c4n) * 4;
    long t = i / c4n;
    ox = (int)(t % Wo);
    t /= Wo;
    oy = (int)(t % Ho);
    b = (int)(t / Ho);
}

// ----------------------------------------------------------------------------- GroupNorm stats
constexpr int GN_CHUNK = 512;   // pixels per partial block

__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ x, double* __restrict__ part,
                                                         int HW, int C, int nchunk) {
    __shared__ double red[2][256];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int lanes_p = 256 / C;                 // pixel lanes per block (C in {64,128,256})
    const int c = threadIdx.x % C, pl = threadIdx.x / C;
    const int p0 = chunk * GN_CHUNK;
    const int p1 = min(p0 + GN_CHUNK, HW);
    double s = 0.0, ss = 0.0;
    const float* xb = x + (long)b * HW * C;
    for (int p = p0 + pl; p < p1; p += lanes_p) {
        const double v = (double)xb[(long)p * C + c];
        s += v;
        ss += v * v;
    }
    red[0][threadIdx.x] = s;
    red[1][threadIdx.x] = ss;
    __syncthreads();
    if (pl == 0) {
        for (int q = 1; q < lanes_p; ++q) {       // fixed order
            s += red[0][q * C + c];
            ss += red[1][q * C + c];
        }
        double* o = part + (((long)b * nchunk + chunk) * C + c) * 2;
        o[0] = s;
        o[1] = ss;
    }
}

// grid (ceil(C/32), B), 256 threads = 8 chunk lanes x 32 channels; fixed summation order => deterministic
// `split` equal channel groups: stats come out as [split][B][C / split][2], so each group is a contiguous [B][C / split][2] block (the two
// semantic branches share one merged GEMM and take one half each)
__global__ __launch_bounds__(256) void gn_final_kernel(const double* __restrict__ part, float* __restrict__ stats, int HW, int C,
                                                       int nchunk, float eps, int split) {
    __shared__ double red[2][8][32];
    const int b = blockIdx.y;
    const int cl = threadIdx.x & 31, kl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    double s = 0.0, ss = 0.0;
    if (c < C)
        for (int k = kl; k < nchunk; k += 8) {
            const double* o = part + (((long)b * nchunk + k) * C + c) * 2;
            s += o[0];
            ss += o[1];
        }
    red[0][kl][cl] = s;
    red[1][kl][cl] = ss;
    __syncthreads();
    if (kl == 0 && c < C) {
        for (int q = 1; q < 8; ++q) {
            s += red[0][q][cl];
            ss += red[1][q][cl];
        }
        const double mean = s / HW;
        double var = ss / HW - mean * mean;
        if (var < 0.0) var = 0.0;
        const int cg = C / split, g = c / cg;
        float* o = stats + (((long)g * gridDim.y + b) * cg + (c - g * cg)) * 2;
        o[0] = (float)mean;
        o[1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// ----------------------------------------------------------------------------- GN + ReLU + bilinear (+=)
__global__ __launch_bounds__(256) void gn_relu_upsample_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ y, int Hi, int Wi, int Ho, int Wo, int C,
                                                               int accumulate, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    int c, ox, oy, b;
    decode_quad(i, C, Ho, Wo, c, ox, oy, b);
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    lm_bilin_axis(oy, Hi, Ho, y0, y1, wy0, wy1);
    lm_bilin_axis(ox, Wi, Wo, x0, x1, wx0, wx1);
    f32x4 a, g;
    gn_affine4_at(stats + ((long)b * C + c) * 2, *reinterpret_cast<const f32x4*>(gamma + c), *reinterpret_cast<const f32x4*>(beta + c), a, g);
    const float* xb = x + (long)b * Hi * Wi * C + c;
    auto tap = [&](int yy, int xx) { return gn_relu4(*reinterpret_cast<const f32x4*>(xb + ((long)yy * Wi + xx) * C), a, g); };
    f32x4 o = bilerp4(tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1), wy0, wy1, wx0, wx1);
    f32x4* yp = reinterpret_cast<f32x4*>(y + i * 4);
    if (accumulate) o = *yp + o;
    *yp = o;
}

// ----------------------------------------------------------------------------- sum of up to 3 GN + ReLU + bilinear terms
// y = ((t0 + t1) + t2), t_k = bilinear(relu(gn_k(x_k))): the reference's `s2 + s3 + s4` (postprojector.py:621,647) in one pass
// instead of one write and two read-modify-writes of y.  Same per-term arithmetic and summation order as three calls of the
// kernel above.  32-bit index math (the launch checks the sizes).
struct GnTerm {
    const float* x;
    const float* stats;
    int Hi, Wi, ld;      // ld: floats between pixels of x (>= C: a term may be a channel slice of a wider tensor)
    float sy, sx;        // lm_bilin_axis's source scales (Hi - 1) / (Ho - 1), (Wi - 1) / (Wo - 1): the same IEEE quotients, taken on the host
};
struct GnSum {
    GnTerm t[3];
    int n;
};

// Optional fused 1x1 projection (feature_layer 128 -> 8, output_layer_endp 128 -> 1; postprojector.py:628-651): the C/4 lanes of a
// pixel sit in one wave (C/4 a power of two <= 64), each multiplies its 4 channels into `cout` partial sums, a butterfly over those lanes
// adds them up and the first lane stores y1[pixel][0..cout) (+ bias).  With y == nullptr the summed tensor itself is never written.
struct Proj1x1 {
    const float* w;      // [C][16] (pack_small layout), nullptr = no projection
    const float* bias;   // [cout] or nullptr
    float* y1;           // [B*Ho*Wo][ldy1]
    int cout, ldy1;
};

// The projection of one pixel in gn_relu_upsample_sum_kernel and gn_sum3_lds_kernel.  Each kernel forms the partial sums itself -
// part[n] = fmaf(acc[e], w[e][n], part[n]) from 0 over its channels e = 0, 1, 2, 3 IN THIS ORDER, n = the 8 (padded) outputs - because
// the weights come from LDS in one and from registers in the other.  The rest is shared:
// transpose-reduce over the c4n = C/4 lanes of the pixel: each of the first three steps halves the outputs a lane keeps while doubling
// the lanes summed (4 + 2 + 1 shuffles), then plain butterflies: 9-10 shuffles instead of 8 x log2(C/4).  Leaves the sum of output
// proj_lane_output(li) in part[0]; `lane` = lane of the wave.  (It returns nothing: with a return value the callers' fmaf chains came
// out as 16 scalar FMAs instead of 8 packed ones.)
__device__ __forceinline__ void proj_reduce(float (&part)[8], int lane, unsigned c4n) {
#pragma unroll
    for (int half = 4, mask = 1; half >= 1; half >>= 1, mask <<= 1) {
        const bool upper = (lane & mask) != 0;
#pragma unroll
        for (int jj = 0; jj < half; ++jj) {
            // (two plain selects: left to itself the compiler turns them into `part[upper ? jj : jj + half]`, a run-time index it
            // resolves with a compare + select per array element - ~200 of the kernel's 500 VALU instructions, profiles/README.md)
            float lo = part[jj], hi = part[jj + half];
            asm volatile("" : "+v"(lo), "+v"(hi));
            const float send = upper ? lo : hi, keep = upper ? hi : lo;
            part[jj] = keep + __shfl_xor(send, mask);
        }
    }
    for (unsigned o = 8; o < c4n; o <<= 1) part[0] += __shfl_xor(part[0], (int)o);
}
// the output n that lane li = c / 4 of the pixel holds after proj_reduce, and whether the lane stores it (+ bias[n]) to y1[pixel][n]:
// lanes >= 8 hold copies
__device__ __forceinline__ int proj_lane_output(unsigned li) { return 4 * (int)(li & 1) + 2 * (int)((li >> 1) & 1) + (int)((li >> 2) & 1); }
__device__ __forceinline__ bool proj_lane_stores(const Proj1x1& Q, unsigned li, int n) { return li < 8 && n < Q.cout; }

// grid (ceil(Wo * C/4 / 256), Ho, B): the output row and the image come from the block index, the column with one division by C/4 (a
// shift for the power-of-two channel counts of the FPN).
// N terms, SAME = bit k set when term k has the output's size (one tap, returned as it is).  Both are TEMPLATE parameters: with run-time
// term counts / sizes every term sat behind a branch, its loads could not be hoisted above the previous term's arithmetic, and a thread
// paid up to three serial memory round trips - the counters showed 73 % of the wave cycles parked at s_waitcnt with 8 waves per SIMD
// (tools/prof_gn_pmc.sh).  Now the statistics and every tap of every term are loaded first (up to 6 + 6 16-byte loads in flight per
// lane), then the arithmetic runs term by term in the order of three gn_relu_upsample_kernel calls.
// 16 bytes at element `elem` of a wave-uniform base: byte offset kept in 32 bits so that the access becomes scalar base + vector offset
__device__ __forceinline__ f32x4 ld_quad(const float* base, unsigned elem) {
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + (elem << 2));
}

template <int N, int SAME>
__global__ __launch_bounds__(256) void gn_relu_upsample_sum_kernel(GnSum P, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float* __restrict__ y, int Ho, int Wo, int C, int c4shift, Proj1x1 Q) {
    __shared__ __attribute__((aligned(16))) float wl[256 * 8];   // projection weights [C][8] (cout padded with zeros)
    const unsigned c4n = (unsigned)C / 4;
    const unsigned j0 = blockIdx.x * 256u + threadIdx.x;      // (column, channel quad) inside the output row
    const bool live = j0 < (unsigned)Wo * c4n;                // (a multiple of C/4: the lanes of a pixel are live together)
    const unsigned j = live ? j0 : 0u;                        // (dead threads of the row's last workgroup load pixel 0 and store nothing)
    const int ox = c4shift >= 0 ? (int)(j >> c4shift) : (int)(j / c4n);
    const int c = (int)(j - (unsigned)ox * c4n) * 4;
    const int oy = (int)blockIdx.y, b = (int)blockIdx.z;
    const unsigned i = ((unsigned)(b * Ho + oy) * (unsigned)Wo) * c4n + j;      // flat output quad
    // ---- phase 1: every load of the thread
    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c), bt = *reinterpret_cast<const f32x4*>(beta + c);
    f32x4 st0[N], st1[N], tap[N][4];
    float wy0[N], wy1[N], wx0[N], wx1[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const GnTerm& T = P.t[k];
        // (wave-uniform 64-bit bases + 32-bit per-lane element offsets: scalar base / vector offset addressing instead of a 64-bit
        // multiply-add chain per tap; an image of a term stays below 2^31 elements - checked by the launcher)
        const float* stb = T.stats + (long)b * C * 2;                 // (mean, rstd) x 4 channels
        st0[k] = ld_quad(stb, (unsigned)(c * 2));
        st1[k] = ld_quad(stb, (unsigned)(c * 2 + 4));
        const float* xb = T.x + (long)b * T.Hi * T.Wi * T.ld;
        if ((SAME >> k) & 1) {
            tap[k][0] = ld_quad(xb, (unsigned)((oy * T.Wi + ox) * T.ld + c));
        } else {
            int y0, y1, x0, x1;
            lm_bilin_axis_scaled(oy, T.Hi, T.sy, y0, y1, wy0[k], wy1[k]);
            lm_bilin_axis_scaled(ox, T.Wi, T.sx, x0, x1, wx0[k], wx1[k]);
            tap[k][0] = ld_quad(xb, (unsigned)((y0 * T.Wi + x0) * T.ld + c));
            tap[k][1] = ld_quad(xb, (unsigned)((y0 * T.Wi + x1) * T.ld + c));
            tap[k][2] = ld_quad(xb, (unsigned)((y1 * T.Wi + x0) * T.ld + c));
            tap[k][3] = ld_quad(xb, (unsigned)((y1 * T.Wi + x1) * T.ld + c));
        }
    }
    // the projection weights are staged BEHIND the taps' loads: in front of them every workgroup paid two memory round trips in a
    // row - weights, barrier, taps
    if (Q.w) {
        for (int k = threadIdx.x; k < C * 8; k += 256) wl[k] = (k & 7) < Q.cout ? Q.w[(k >> 3) * 16 + (k & 7)] : 0.f;
        __syncthreads();
    }
    if (!live) return;
    // ---- phase 2: arithmetic, term by term
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < N; ++k) {
        f32x4 a, g;
        gn_affine4(st0[k], st1[k], gm, bt, a, g);
        f32x4 o;
        if ((SAME >> k) & 1)                // same size: the blend has weights (1, 0) and returns the tap itself, bit for bit
            o = gn_relu4(tap[k][0], a, g);
        else
            o = bilerp4(gn_relu4(tap[k][0], a, g), gn_relu4(tap[k][1], a, g), gn_relu4(tap[k][2], a, g), gn_relu4(tap[k][3], a, g),
                        wy0[k], wy1[k], wx0[k], wx1[k]);
        if (k == 0) {
            acc = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] + o[e];
        }
    }
    if (y) *reinterpret_cast<f32x4*>(y + (long)i * 4) = acc;
    if (Q.w) {
        // partial sums of this lane's 4 channels for the 8 (padded) outputs, weights from the LDS copy [C][8]
        float part[8];
#pragma unroll
        for (int n = 0; n < 8; ++n) part[n] = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(wl + (c + e) * 8), w1 = *reinterpret_cast<const f32x4*>(wl + (c + e) * 8 + 4);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                part[n] = fmaf(acc[e], w0[n], part[n]);
                part[4 + n] = fmaf(acc[e], w1[n], part[4 + n]);
            }
        }
        proj_reduce(part, threadIdx.x & 63, c4n);
        const unsigned li = (unsigned)c >> 2;
        const int n = proj_lane_output(li);
        if (proj_lane_stores(Q, li, n)) Q.y1[(long)((b * Ho + oy) * Wo + ox) * Q.ldy1 + n] = part[0] + (Q.bias ? Q.bias[n] : 0.f);
    }
}

// ----------------------------------------------------------------------------- one GN + ReLU + bilinear term, source staged in LDS
// The one-term up-sampling call (s4 of the semantic branches: 256 channels, 144^2 -> 288^2, 0.68 GB written per 8 tiles) ran at 2.7 TB/s
// in the kernel above against 5.8 TB/s for the same-size case: four 16-byte taps per output quad from the vector cache, each normalised
// again by every output that touches it.  Here a workgroup owns UT_R x UT_C output pixels x all channels: the source block it needs
// (<= UT_SR x UT_SC pixels for scales <= 1/2 + eps, checked by the launcher) is read ONCE, normalised + ReLU'd once per element and kept
// in LDS; the outputs then blend four ds_read_b128 taps.  Same per-element arithmetic (lm_gn_relu, then lm_bilerp with lm_bilin_axis
// weights, through the helpers at the top of this file) as gn_relu_upsample_kernel / gn_relu_upsample_sum_kernel<1, 0>.
constexpr int UT_R = 8, UT_C = 16;

// The LDS up-sampling tile of gn_relu_up_lds_kernel and gn_sum3_lds_kernel.  The kernels declare the LDS - the normalised + ReLU'd
// source block ups[SR * SC][C] (dynamic) and the eight tap tables - and the helpers get pointers to it.
// first tap of output row / column o0: the origin of the tile's source block
__device__ __forceinline__ int up_tile_origin(int o0, int in, float scale) {
    int i0, i1;
    float w0, w1;
    lm_bilin_axis_scaled(o0, in, scale, i0, i1, w0, w1);
    return i0;
}
// entry t of one axis' tap tables: the taps (relative to the origin) and weights of output row / column o0 + t, clamped to the image.
// Threads 0..UT_R-1 write the rows and 64..64+UT_C-1 the columns; the kernel's barrier comes before the tables are read.  (That
// two-armed `if` stays in the kernels: inside a helper the compiler merges the arms' stores behind selected addresses, +15 instructions.)
__device__ __forceinline__ void up_axis_taps(int t, int o0, int out, int in, float scale, int origin, int* t0, int* t1, float* w0, float* w1) {
    int a0, a1;
    lm_bilin_axis_scaled(min(o0 + t, out - 1), in, scale, a0, a1, w0[t], w1[t]);
    t0[t] = a0 - origin;
    t1[t] = a1 - origin;
}
// source block (SC columns from (sy0, sx0), nsrc pixels) of image b -> ups, normalised with (a, g).  256 % (C/4) == 0: a thread keeps
// one channel quad c and walks the pixels p0, p0 + pstep, ...
__device__ __forceinline__ void up_tile_stage(float* ups, const GnTerm& T, int b, int C, int c, int p0, int pstep, int sy0, int sx0, int SC,
                                              int nsrc, f32x4 a, f32x4 g) {
    const float* xb = T.x + (long)b * T.Hi * T.Wi * T.ld + c;
    constexpr int UNR = 4;                                             // loads in flight per thread and round
    for (int pb = p0; pb < nsrc; pb += pstep * UNR) {
        f32x4 v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int pp = pb + u * pstep;
            const int r = pp / SC, q = pp - r * SC;
            const int yy = min(sy0 + r, T.Hi - 1), xx = min(sx0 + q, T.Wi - 1);     // (clamped: rows / columns past the image are never blended)
            if (pp < nsrc) v[u] = *reinterpret_cast<const f32x4*>(xb + ((long)yy * T.Wi + xx) * T.ld);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int pp = pb + u * pstep;
            if (pp < nsrc) *reinterpret_cast<f32x4*>(ups + (long)pp * C + c) = gn_relu4(v[u], a, g);
        }
    }
}
// channel quad c of the tile's output (r, q): four ds_read_b128 taps, blended
struct UpTile {
    const float* ups;
    const int *ty0, *ty1, *tx0, *tx1;              // taps (relative to the block origin) of the tile's rows / columns
    const float *twy0, *twy1, *twx0, *twx1;        // and their weights
    int SC, C;
};
__device__ __forceinline__ f32x4 up_tile_blend(const UpTile& U, int r, int q, int c) {
    const float* s0 = U.ups + (long)(U.ty0[r] * U.SC) * U.C + c;
    const float* s1 = U.ups + (long)(U.ty1[r] * U.SC) * U.C + c;
    const f32x4 v00 = *reinterpret_cast<const f32x4*>(s0 + U.tx0[q] * U.C), v01 = *reinterpret_cast<const f32x4*>(s0 + U.tx1[q] * U.C);
    const f32x4 v10 = *reinterpret_cast<const f32x4*>(s1 + U.tx0[q] * U.C), v11 = *reinterpret_cast<const f32x4*>(s1 + U.tx1[q] * U.C);
    return bilerp4(v00, v01, v10, v11, U.twy0[r], U.twy1[r], U.twx0[q], U.twx1[q]);
}

__global__ __launch_bounds__(256) void gn_relu_up_lds_kernel(GnTerm T, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ y, int Ho, int Wo, int C, int SR, int SC) {
    extern __shared__ __attribute__((aligned(16))) float ups[];
    __shared__ int ty0[UT_R], ty1[UT_R], tx0[UT_C], tx1[UT_C];
    __shared__ float twy0[UT_R], twy1[UT_R], twx0[UT_C], twx1[UT_C];
    const UpTile U{ups, ty0, ty1, tx0, tx1, twy0, twy1, twx0, twx1, SC, C};
    const int tid = threadIdx.x, c4n = C / 4;
    const int oy0 = blockIdx.y * UT_R, ox0 = blockIdx.x * UT_C, b = blockIdx.z;
    const int ny = min(UT_R, Ho - oy0), nx = min(UT_C, Wo - ox0);
    const int sy0 = up_tile_origin(oy0, T.Hi, T.sy), sx0 = up_tile_origin(ox0, T.Wi, T.sx);
    if (tid < UT_R) up_axis_taps(tid, oy0, Ho, T.Hi, T.sy, sy0, ty0, ty1, twy0, twy1);
    else if (tid >= 64 && tid < 64 + UT_C) up_axis_taps(tid - 64, ox0, Wo, T.Wi, T.sx, sx0, tx0, tx1, twx0, twx1);
    // ---- phase 1: source block -> LDS
    const int cq = tid % c4n, pstep = 256 / c4n, p0 = tid / c4n;
    const int c = cq * 4;
    f32x4 a, g;
    gn_affine4_at(T.stats + ((long)b * C + c) * 2, *reinterpret_cast<const f32x4*>(gamma + c), *reinterpret_cast<const f32x4*>(beta + c), a, g);
    up_tile_stage(ups, T, b, C, c, p0, pstep, sy0, sx0, SC, SR * SC, a, g);
    __syncthreads();
    // ---- phase 2: outputs
    const long obase = ((long)b * Ho + oy0) * Wo + ox0;
    for (int pp = p0; pp < UT_R * UT_C; pp += pstep) {
        const int r = pp / UT_C, q = pp % UT_C;
        if (r >= ny || q >= nx) continue;
        __builtin_nontemporal_store(up_tile_blend(U, r, q, c), reinterpret_cast<f32x4*>(y + (obase + (long)r * Wo + q) * C + c));
    }
}

// ----------------------------------------------------------------------------- s2 + s3 + s4 with the up-sampled term staged in LDS
// The three-term call of the semantic branches - two same-size terms (s2, s4) and ONE up-sampled term (s3: 144^2 -> 288^2) followed by the
// branch's 1x1 output layer - ran at 2.9 TB/s in gn_relu_upsample_sum_kernel<3, 5>: per output quad six 16-byte loads, three
// (mean, rstd) pairs, three GroupNorm affines, the blend and the projection weights from LDS.  Here a workgroup owns UT_R x UT_C output
// pixels x all channels, a thread keeps ONE channel quad for all its pixels: the affines of the three terms and its 4 x 8 projection
// weights are made once per thread, the up-sampled term's source block is normalised once per element and staged in LDS (as in
// gn_relu_up_lds_kernel), and an output quad costs two 16-byte global loads + four ds_read_b128.  The arithmetic and its order are
// gn_relu_upsample_sum_kernel<3, 5>'s through the shared helpers (gn_affine4, gn_relu4, bilerp4, (t0 + t1) + t2, the fmaf chain,
// proj_reduce): the same bits (test_gn_sum_three_terms_lds_bit_identical).  C/4 lanes of a pixel sit in one wave (C/4 | 64).
__global__ __launch_bounds__(256) void gn_sum3_lds_kernel(GnSum P, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ y, int Ho, int Wo, int C, int SR, int SC, Proj1x1 Q) {
    extern __shared__ __attribute__((aligned(16))) float ups[];       // source block of term 1
    __shared__ int ty0[UT_R], ty1[UT_R], tx0[UT_C], tx1[UT_C];
    __shared__ float twy0[UT_R], twy1[UT_R], twx0[UT_C], twx1[UT_C];
    const UpTile U{ups, ty0, ty1, tx0, tx1, twy0, twy1, twx0, twx1, SC, C};
    const int tid = threadIdx.x, c4n = C / 4;
    const int oy0 = blockIdx.y * UT_R, ox0 = blockIdx.x * UT_C, b = blockIdx.z;
    const int ny = min(UT_R, Ho - oy0), nx = min(UT_C, Wo - ox0);
    const GnTerm& T0 = P.t[0];
    const GnTerm& T1 = P.t[1];
    const GnTerm& T2 = P.t[2];
    const int sy0 = up_tile_origin(oy0, T1.Hi, T1.sy), sx0 = up_tile_origin(ox0, T1.Wi, T1.sx);
    if (tid < UT_R) up_axis_taps(tid, oy0, Ho, T1.Hi, T1.sy, sy0, ty0, ty1, twy0, twy1);
    else if (tid >= 64 && tid < 64 + UT_C) up_axis_taps(tid - 64, ox0, Wo, T1.Wi, T1.sx, sx0, tx0, tx1, twx0, twx1);
    const int cq = tid % c4n, pstep = 256 / c4n, p0 = tid / c4n;
    const int c = cq * 4;
    // the three affines of this thread's channel quad
    f32x4 a[3], g[3];
    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c), bt = *reinterpret_cast<const f32x4*>(beta + c);
#pragma unroll
    for (int k = 0; k < 3; ++k) gn_affine4_at(P.t[k].stats + ((long)b * C + c) * 2, gm, bt, a[k], g[k]);
    // projection weights of this thread's four channels, [e][8] (cout padded with zeros, like the LDS copy of the per-output kernel)
    float pw[4][8];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int n = 0; n < 8; ++n) pw[e][n] = n < Q.cout ? Q.w[(c + e) * 16 + n] : 0.f;
    // ---- phase 1: source block of the up-sampled term -> LDS
    up_tile_stage(ups, T1, b, C, c, p0, pstep, sy0, sx0, SC, SR * SC, a[1], g[1]);
    __syncthreads();
    // ---- phase 2: outputs, UNR2 pixels of this thread in flight
    const float* x0b = T0.x + (long)b * T0.Hi * T0.Wi * T0.ld + c;
    const float* x2b = T2.x + (long)b * T2.Hi * T2.Wi * T2.ld + c;
    const unsigned li = (unsigned)cq;
    const int nsel = proj_lane_output(li);
    const float pbias = (proj_lane_stores(Q, li, nsel) && Q.bias) ? Q.bias[nsel] : 0.f;
    constexpr int UNR2 = 4;
    for (int pb = p0; pb < UT_R * UT_C; pb += pstep * UNR2) {
        f32x4 t0[UNR2], t2[UNR2];
        bool live[UNR2];
        int rr[UNR2], qq[UNR2];
#pragma unroll
        for (int u = 0; u < UNR2; ++u) {
            const int pp = pb + u * pstep;
            rr[u] = pp / UT_C; qq[u] = pp % UT_C;
            live[u] = rr[u] < ny && qq[u] < nx;
            const int oy = min(oy0 + rr[u], Ho - 1), ox = min(ox0 + qq[u], Wo - 1);       // (dead pixels load a valid one and store nothing)
            t0[u] = *reinterpret_cast<const f32x4*>(x0b + ((long)oy * T0.Wi + ox) * T0.ld);
            t2[u] = *reinterpret_cast<const f32x4*>(x2b + ((long)oy * T2.Wi + ox) * T2.ld);
        }
#pragma unroll
        for (int u = 0; u < UNR2; ++u) {
            const f32x4 o0 = gn_relu4(t0[u], a[0], g[0]), o1 = up_tile_blend(U, min(rr[u], UT_R - 1), qq[u], c), o2 = gn_relu4(t2[u], a[2], g[2]);
            f32x4 acc;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = (o0[e] + o1[e]) + o2[e];
            const long opix = ((long)b * Ho + oy0 + rr[u]) * Wo + ox0 + qq[u];
            if (y && live[u]) *reinterpret_cast<f32x4*>(y + opix * C + c) = acc;
            float part[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) part[n] = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int n = 0; n < 8; ++n) part[n] = fmaf(acc[e], pw[e][n], part[n]);
            proj_reduce(part, tid & 63, (unsigned)c4n);
            if (live[u] && proj_lane_stores(Q, li, nsel)) Q.y1[opix * Q.ldy1 + nsel] = part[0] + pbias;
        }
    }
}

// ----------------------------------------------------------------------------- plain bilinear, NHWC -> NHWC slice
__global__ __launch_bounds__(256) void upsample_nhwc_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ add, int lda,
                                                            float* __restrict__ y, int ldy, int Hi, int Wi, int Ho, int Wo,
                                                            int C, long total4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    int c, ox, oy, b;
    decode_quad(i, C, Ho, Wo, c, ox, oy, b);
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    lm_bilin_axis(oy, Hi, Ho, y0, y1, wy0, wy1);
    lm_bilin_axis(ox, Wi, Wo, x0, x1, wx0, wx1);
    const float* xb = x + (long)b * Hi * Wi * ldx + c;
    const f32x4 v00 = *reinterpret_cast<const f32x4*>(xb + ((long)y0 * Wi + x0) * ldx);
    const f32x4 v01 = *reinterpret_cast<const f32x4*>(xb + ((long)y0 * Wi + x1) * ldx);
    const f32x4 v10 = *reinterpret_cast<const f32x4*>(xb + ((long)y1 * Wi + x0) * ldx);
    const f32x4 v11 = *reinterpret_cast<const f32x4*>(xb + ((long)y1 * Wi + x1) * ldx);
    const long opix = ((long)b * Ho + oy) * Wo + ox;
    f32x4 o = bilerp4(v00, v01, v10, v11, wy0, wy1, wx0, wx1);
    if (add) o = o + *reinterpret_cast<const f32x4*>(add + opix * lda + c);
    *reinterpret_cast<f32x4*>(y + opix * ldy + c) = o;
}

// NHWC (few channels) -> planar [B,C,Ho,Wo]
__global__ __launch_bounds__(256) void upsample_to_chw_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y,
                                                              int Hi, int Wi, int Ho, int Wo, int C, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % Wo);
    long t = i / Wo;
    const int oy = (int)(t % Ho);
    t /= Ho;
    const int c = (int)(t % C);
    const int b = (int)(t / C);
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    lm_bilin_axis(oy, Hi, Ho, y0, y1, wy0, wy1);
    lm_bilin_axis(ox, Wi, Wo, x0, x1, wx0, wx1);
    const float* xb = x + (long)b * Hi * Wi * ldx + c;
    const float v00 = xb[((long)y0 * Wi + x0) * ldx], v01 = xb[((long)y0 * Wi + x1) * ldx];
    const float v10 = xb[((long)y1 * Wi + x0) * ldx], v11 = xb[((long)y1 * Wi + x1) * ldx];
    y[i] = lm_bilerp(v00, v01, v10, v11, wy0, wy1, wx0, wx1);
}

// four horizontally adjacent outputs per thread (Wo % 4 == 0): one row decode and one y-axis interpolation per 16-byte store, 32-bit
// index math.  Same blend as the scalar kernel: lm_bilerp's fixed order (common.h), so the two agree bit for bit.
__global__ __launch_bounds__(256) void upsample_to_chw4_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y,
                                                               int Hi, int Wi, int Ho, int Wo, int C, unsigned total4) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total4) return;
    const unsigned wq = (unsigned)Wo / 4;
    const int ox0 = (int)(i % wq) * 4;
    unsigned t = i / wq;
    const int oy = (int)(t % (unsigned)Ho);
    t /= (unsigned)Ho;
    const int c = (int)(t % (unsigned)C);
    const int b = (int)(t / (unsigned)C);
    int y0, y1;
    float wy0, wy1;
    lm_bilin_axis(oy, Hi, Ho, y0, y1, wy0, wy1);
    const float* xb = x + (long)b * Hi * Wi * ldx + c;
    const float* r0 = xb + (long)y0 * Wi * ldx;
    const float* r1 = xb + (long)y1 * Wi * ldx;
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int x0, x1;
        float wx0, wx1;
        lm_bilin_axis(ox0 + k, Wi, Wo, x0, x1, wx0, wx1);
        const float v00 = r0[(long)x0 * ldx], v01 = r0[(long)x1 * ldx], v10 = r1[(long)x0 * ldx], v11 = r1[(long)x1 * ldx];
        o[k] = lm_bilerp(v00, v01, v10, v11, wy0, wy1, wx0, wx1);
    }
    *reinterpret_cast<f32x4*>(y + (long)i * 4) = o;
}

// ----------------------------------------------------------------------------- LayerNorm: one wave per row
// Two-pass arithmetic, PER * 64 >= D columns per lane slot.  MASKED: the columns >= D are masked out - a masked column holds 0 and adds
// 0 to the lane's sum, so each lane's sums and the butterfly run in the same order as without the mask.
template <int PER, bool MASKED>
__device__ __forceinline__ void layernorm_row(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                              float* __restrict__ y, long rows, int D, float eps) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + row * D;
    float v[PER];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = k * 64 + lane;
        v[k] = (!MASKED || c < D) ? xr[c] : 0.f;
        s += v[k];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const float d = (!MASKED || k * 64 + lane < D) ? v[k] - mean : 0.f;
        q += d * d;
    }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q / (float)D + eps);
    float* yr = y + row * D;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = k * 64 + lane;
        if (!MASKED || c < D) yr[c] = (v[k] - mean) * rstd * gamma[c] + beta[c];
    }
}

// D = PER * 64 (512 and 1024)
template <int PER>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y, long rows,
                                                        float eps) {
    layernorm_row<PER, false>(x, gamma, beta, y, rows, PER * 64, eps);
}

// The other widths (D % 32 == 0, 32 <= D <= 4096, not 768; the ViT at patch sizes 4 / 6 / 12 / 16 has D = 128 / 288 / 1152 / 2048)
template <int PER>
__global__ __launch_bounds__(256) void layernorm_masked_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ y, long rows, int D,
                                                               float eps) {
    layernorm_row<PER, true>(x, gamma, beta, y, rows, D, eps);
}

__global__ __launch_bounds__(256) void unpatchify_kernel(const float* __restrict__ t, float* __restrict__ y, int G, int P,
                                                         int C, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;   // index into NHWC output [B, G*P, G*P, C]
    if (i >= total) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int xx = (int)(r % (G * P));
    r /= (G * P);
    const int yy = (int)(r % (G * P));
    const int b = (int)(r / (G * P));
    const int gh = yy / P, p1 = yy % P, gw = xx / P, p2 = xx % P;
    y[i] = t[((long)b * G * G + gh * G + gw) * (P * P * C) + (p1 * P + p2) * C + c];
}

int launch_gn_final(void* stream, const double* part, float* stats, int B, int HW, int C, int nchunk, float eps, int split) {
    hipLaunchKernelGGL(gn_final_kernel, dim3(lm_cdiv(C, 32), B), dim3(256), 0, (hipStream_t)stream, part, stats, HW, C, nchunk, eps, split);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

}  // namespace

LM_API int lm_gn_stats(void* stream, const float* x, double* workspace, float* stats, int B, int HW, int C, float eps) {
    LM_REQUIRE(x && workspace && stats, "gn_stats: null pointer");
    LM_REQUIRE(C <= 256 && 256 % C == 0, "gn_stats: C=%d must divide 256", C);
    const int nchunk = lm_cdiv(HW, GN_CHUNK);
    hipLaunchKernelGGL(gn_partial_kernel, dim3(nchunk, B), dim3(256), 0, (hipStream_t)stream, x, workspace, HW, C, nchunk);
    LM_LAUNCH_CHECK();
    return launch_gn_final(stream, workspace, stats, B, HW, C, nchunk, eps, 1);
}

// second pass for partials produced by lm_conv2d_nhwc_mfma_f32_gnstats ([B][nchunk][C][2] doubles)
LM_API int lm_gn_finalize(void* stream, const double* partial, float* stats, int B, int HW, int C, int nchunk, float eps) {
    LM_REQUIRE(partial && stats && nchunk >= 1, "gn_finalize: bad args");
    return launch_gn_final(stream, partial, stats, B, HW, C, nchunk, eps, 1);
}

// the same with the statistics laid out per channel group: stats [split][B][C / split][2] (C % split == 0) - same values
LM_API int lm_gn_finalize_split(void* stream, const double* partial, float* stats, int B, int HW, int C, int nchunk, float eps, int split) {
    LM_REQUIRE(partial && stats && nchunk >= 1 && split >= 1 && C % split == 0, "gn_finalize_split: bad args (C=%d split=%d)", C, split);
    return launch_gn_final(stream, partial, stats, B, HW, C, nchunk, eps, split);
}

LM_API long lm_gn_stats_workspace_bytes(int B, int HW, int C) {
    return (long)B * lm_cdiv(HW, GN_CHUNK) * C * 2 * (long)sizeof(double);
}

LM_API int lm_gn_relu_upsample(void* stream, const float* x, const float* stats, const float* gamma, const float* beta,
                               float* y, int B, int Hi, int Wi, int Ho, int Wo, int C, int accumulate) {
    LM_REQUIRE(x && stats && gamma && beta && y && C % 4 == 0, "gn_relu_upsample: bad args");
    const long total4 = (long)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(gn_relu_upsample_kernel, dim3(lm_cdiv(total4, 256)), dim3(256), 0, (hipStream_t)stream,
                       x, stats, gamma, beta, y, Hi, Wi, Ho, Wo, C, accumulate, total4);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

namespace {
// Source rows (columns) the tiles of `tile` output rows need at most: last second tap - first first tap + 1, from the SAME float
// arithmetic as lm_bilin_axis (IEEE single precision on both sides, no contraction), so the kernel's LDS block is exactly large enough.
int up_block_extent(int in, int out, int tile) {
#pragma clang fp contract(off)
    const float scale = (out > 1) ? (float)(in - 1) / (float)(out - 1) : 0.f;
    auto tap0 = [&](int o) {
        int i0 = (int)(scale * (float)o);
        return i0 > in - 1 ? in - 1 : i0;
    };
    int ext = 1;
    for (int o0 = 0; o0 < out; o0 += tile) {
        const int ol = (o0 + tile - 1 < out ? o0 + tile - 1 : out - 1);
        const int last0 = tap0(ol), last1 = last0 + (last0 < in - 1 ? 1 : 0);
        const int e = last1 - tap0(o0) + 1;
        if (e > ext) ext = e;
    }
    return ext;
}

// Whether the up-sampled term T takes an LDS kernel: its test-only switch is on, the scale is <= 1/2 on both axes, and the source block
// of a UT_R x UT_C output tile (SR x SC pixels x C floats) fits `cap` bytes.
struct UpLdsRoute {
    int SR, SC;
    size_t bytes;
};
bool up_lds_route(const GnTerm& T, int Ho, int Wo, int C, size_t cap, bool on, UpLdsRoute& R) {
    if (!on || T.Hi <= 1 || T.Wi <= 1 || Ho < 2 * T.Hi - 1 || Wo < 2 * T.Wi - 1) return false;
    R.SR = up_block_extent(T.Hi, Ho, UT_R);
    R.SC = up_block_extent(T.Wi, Wo, UT_C);
    R.bytes = (size_t)R.SR * R.SC * C * sizeof(float);
    return R.bytes <= cap;
}
// grid (ceil(Wo / UT_C), ceil(Ho / UT_R), B), `lds` bytes of dynamic LDS
template <class Kernel, class... Args>
int launch_up_tile(Kernel kernel, size_t lds, void* stream, int B, int Ho, int Wo, Args... args) {
    if (int e = lm_ensure_dynamic_lds((const void*)kernel, lds)) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)lm_cdiv(Wo, UT_C), (unsigned)lm_cdiv(Ho, UT_R), (unsigned)B), dim3(256), lds, (hipStream_t)stream, args...);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

int launch_gn_sum(void* stream, int n, const float* const* x, const float* const* stats, const int* Hi, const int* Wi, const int* ldx,
                  const float* gamma, const float* beta, float* y, int B, int Ho, int Wo, int C, Proj1x1 Q) {
    LM_REQUIRE(n >= 1 && n <= 3 && x && stats && Hi && Wi && gamma && beta && C > 0 && C % 4 == 0, "gn_relu_upsample_sum: bad args");
    const long total4 = (long)B * Ho * Wo * (C / 4);
    LM_REQUIRE(total4 > 0 && total4 < (1L << 31), "gn_relu_upsample_sum: %ld output quads do not fit 32-bit indices", total4);
    GnSum P;
    P.n = n;
    for (int k = 0; k < 3; ++k) {
        const int q = k < n ? k : 0;
        LM_REQUIRE(x[q] && stats[q] && Hi[q] > 0 && Wi[q] > 0, "gn_relu_upsample_sum: bad term %d", q);
        const int ld = ldx ? ldx[q] : C;
        LM_REQUIRE(ld >= C && ld % 4 == 0, "gn_relu_upsample_sum: bad leading dimension %d of term %d", ld, q);
        LM_REQUIRE((long)Hi[q] * Wi[q] * ld < (1L << 30), "gn_relu_upsample_sum: term %d: an image of %ld elements does not fit 32-bit byte offsets", q,
                   (long)Hi[q] * Wi[q] * ld);
        P.t[k] = GnTerm{x[q], stats[q], Hi[q], Wi[q], ld, Ho > 1 ? (float)(Hi[q] - 1) / (float)(Ho - 1) : 0.f,
                        Wo > 1 ? (float)(Wi[q] - 1) / (float)(Wo - 1) : 0.f};
    }
    const int c4n = C / 4;
    LM_REQUIRE(256 % c4n == 0 || !Q.w, "gn_relu_upsample_sum: the fused 1x1 projection needs C/4 = %d to divide 256", c4n);
    LM_REQUIRE(Ho <= 65535 && B <= 65535, "gn_relu_upsample_sum: grid too large");
    int c4shift = -1;
    for (int sft = 0; sft < 16; ++sft)
        if ((1 << sft) == c4n) c4shift = sft;
    int same = 0;
    for (int k = 0; k < n; ++k)
        if (Hi[k] == Ho && Wi[k] == Wo) same |= 1 << k;
    UpLdsRoute R;
    if (n == 1 && same == 0 && !Q.w && y && 256 % c4n == 0) {
        // one up-sampling term: source block staged in LDS
        static const bool lds_up = [] { const char* e = getenv("LM_GN_UP_LDS"); return !e || atoi(e) != 0; }();
        if (up_lds_route(P.t[0], Ho, Wo, C, 72 * 1024, lds_up, R))
            return launch_up_tile(gn_relu_up_lds_kernel, R.bytes, stream, B, Ho, Wo, P.t[0], gamma, beta, y, Ho, Wo, C, R.SR, R.SC);
    }
    if (n == 3 && same == 5 && Q.w && c4n >= 8 && c4n <= 64 && (c4n & (c4n - 1)) == 0) {
        // s2 + s3 + s4 (+ the branch's 1x1 output layer): the up-sampled middle term through LDS, affines and weights once per thread
        static const bool lds_sum = [] { const char* e = getenv("LM_GN_SUM_LDS"); return !e || atoi(e) != 0; }();
        if (up_lds_route(P.t[1], Ho, Wo, C, 64 * 1024, lds_sum, R))
            return launch_up_tile(gn_sum3_lds_kernel, R.bytes, stream, B, Ho, Wo, P, gamma, beta, y, Ho, Wo, C, R.SR, R.SC, Q);
    }
    const dim3 grid((unsigned)lm_cdiv((long)Wo * c4n, 256), (unsigned)Ho, (unsigned)B);
#define LM_GNS(NN, SS)                                                                                                           \
    case (NN) * 8 + (SS):                                                                                                        \
        hipLaunchKernelGGL((gn_relu_upsample_sum_kernel<NN, SS>), grid, dim3(256), 0, (hipStream_t)stream, P, gamma, beta, y, Ho, Wo, C, \
                           c4shift, Q);                                                                                         \
        break;
    switch (n * 8 + same) {
        LM_GNS(1, 0) LM_GNS(1, 1)
        LM_GNS(2, 0) LM_GNS(2, 1) LM_GNS(2, 2) LM_GNS(2, 3)
        LM_GNS(3, 0) LM_GNS(3, 1) LM_GNS(3, 2) LM_GNS(3, 3) LM_GNS(3, 4) LM_GNS(3, 5) LM_GNS(3, 6) LM_GNS(3, 7)
    }
#undef LM_GNS
    LM_LAUNCH_CHECK();
    return LM_OK;
}
}  // namespace

LM_API int lm_gn_relu_upsample_sum(void* stream, int n, const float* const* x, const float* const* stats, const int* Hi, const int* Wi,
                                   const int* ldx, const float* gamma, const float* beta, float* y, int B, int Ho, int Wo, int C) {
    LM_REQUIRE(y, "gn_relu_upsample_sum: null output");
    return launch_gn_sum(stream, n, x, stats, Hi, Wi, ldx, gamma, beta, y, B, Ho, Wo, C, Proj1x1{nullptr, nullptr, nullptr, 0, 0});
}

// Same sum followed by a 1x1 convolution y1 = sum @ w + bias (cout <= 8, w in the [C][16] layout of lm_conv2d_nhwc_small) computed from
// registers; y may be NULL, in which case the C-channel sum is never written (feature_layer / output_layer_endp read nothing else).
LM_API int lm_gn_relu_upsample_sum_conv1x1(void* stream, int n, const float* const* x, const float* const* stats, const int* Hi,
                                           const int* Wi, const int* ldx, const float* gamma, const float* beta, float* y, int B, int Ho,
                                           int Wo, int C, const float* w_c16, const float* bias, int cout, float* y1, int ldy1) {
    LM_REQUIRE(w_c16 && y1 && cout >= 1 && cout <= 8 && ldy1 >= cout, "gn_relu_upsample_sum_conv1x1: bad projection (cout=%d)", cout);
    const int c4n = C / 4;
    LM_REQUIRE(C % 4 == 0 && c4n >= 8 && c4n <= 64 && (c4n & (c4n - 1)) == 0,
               "gn_relu_upsample_sum_conv1x1: C=%d: C/4 must be a power of two in [8, 64] (one pixel per wave segment)", C);
    return launch_gn_sum(stream, n, x, stats, Hi, Wi, ldx, gamma, beta, y, B, Ho, Wo, C, Proj1x1{w_c16, bias, y1, cout, ldy1});
}

LM_API int lm_upsample_bilinear_nhwc(void* stream, const float* x, int ldx, const float* add, int lda, float* y, int ldy,
                                     int B, int Hi, int Wi, int Ho, int Wo, int C) {
    LM_REQUIRE(x && y && C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && (!add || lda % 4 == 0), "upsample_nhwc: bad args");
    const long total4 = (long)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(upsample_nhwc_kernel, dim3(lm_cdiv(total4, 256)), dim3(256), 0, (hipStream_t)stream,
                       x, ldx, add, lda, y, ldy, Hi, Wi, Ho, Wo, C, total4);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

LM_API int lm_upsample_bilinear_to_chw(void* stream, const float* x, int ldx, float* y, int B, int Hi, int Wi,
                                       int Ho, int Wo, int C) {
    LM_REQUIRE(x && y && C >= 1, "upsample_to_chw: bad args");
    const long total = (long)B * C * Ho * Wo;
    if (Wo % 4 == 0 && total / 4 < (1L << 31) && ((uintptr_t)y & 15) == 0) {
        hipLaunchKernelGGL(upsample_to_chw4_kernel, dim3(lm_cdiv(total / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                           x, ldx, y, Hi, Wi, Ho, Wo, C, (unsigned)(total / 4));
        LM_LAUNCH_CHECK();
        return LM_OK;
    }
    hipLaunchKernelGGL(upsample_to_chw_kernel, dim3(lm_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       x, ldx, y, Hi, Wi, Ho, Wo, C, total);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

LM_API int lm_layernorm_rows(void* stream, const float* x, const float* gamma, const float* beta, float* y,
                             long rows, int D, float eps) {
    // D = 768 stays refused as it always was: the entry-point tests pin that refusal, and no reference config uses it
    LM_REQUIRE(x && gamma && beta && y && D >= 32 && D <= 4096 && D % 32 == 0 && D != 768,
               "layernorm: D=%d must be 512 or 1024, or another multiple of 32 in [32, 4096] except 768", D);
    const dim3 grid(lm_cdiv(rows, 4));
    hipStream_t s = (hipStream_t)stream;
    if (D == 512)
        hipLaunchKernelGGL(layernorm_kernel<8>, grid, dim3(256), 0, s, x, gamma, beta, y, rows, eps);
    else if (D == 1024)
        hipLaunchKernelGGL(layernorm_kernel<16>, grid, dim3(256), 0, s, x, gamma, beta, y, rows, eps);
#define LM_LN_MASKED(PER) else if (D <= PER * 64) hipLaunchKernelGGL(layernorm_masked_kernel<PER>, grid, dim3(256), 0, s, x, gamma, beta, y, rows, D, eps);
    LM_LN_MASKED(1) LM_LN_MASKED(2) LM_LN_MASKED(4) LM_LN_MASKED(8) LM_LN_MASKED(16) LM_LN_MASKED(32) LM_LN_MASKED(64)
#undef LM_LN_MASKED
    LM_LAUNCH_CHECK();
    return LM_OK;
}

LM_API int lm_unpatchify(void* stream, const float* tokens, float* y_nhwc, int B, int G, int P, int C) {
    LM_REQUIRE(tokens && y_nhwc, "unpatchify: null pointer");
    const long total = (long)B * G * P * G * P * C;
    hipLaunchKernelGGL(unpatchify_kernel, dim3(lm_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, tokens, y_nhwc, G, P, C, total);
    LM_LAUNCH_CHECK();
    return LM_OK;
}
