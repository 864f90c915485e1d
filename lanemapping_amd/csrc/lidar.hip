// Sparse-voxel LiDAR encoder front end: hard voxelisation, sparse-convolution
// rulebooks, densify + H flip, bicubic up-sampling.
//
// PARITY UNPINNED for the voxeliser and the sparse convolutions: the reference only CALLS them
// (baseline/models/pcencoder/lidarencoder.py:29-35 builds mmdet3d's VoxelizationByGridShape and SparseEncoder,
// :93,:102 call them); the arithmetic lives in mmdet3d dev-1.x / mmcv.ops (unpinned commit, absent here).  What is
// restated is their published behaviour:
//   * hard voxelisation, deterministic flavour: c = floor((p - range_min) / voxel_size) per axis, points outside the grid
//     are dropped, non-finite coordinates are dropped (a point with a NaN or +-Inf x, y or z is outside every grid; a
//     non-finite intensity is an ordinary value), voxels are numbered by the index of their first point, a voxel keeps
//     its first `max_points` points (index order), voxels beyond `max_voxels` are dropped; coords are (z, y, x);
//   * LidarEncoder.voxelize (:104-129): batch index prepended, feature = sum of kept points / count;
//   * spconv: SubMConv3d keeps the active set, SparseConv3d activates every output site whose window holds an active
//     input; out[o] = sum_k W[k] in[o*stride - pad + k] (cross-correlation, taps ordered (kz, ky, kx));
//   * SparseConvTensor.dense() + view(N, C*D, H, W), then torch.flip(dims=[2]) (:70) and bicubic align_corners=False (:72).
// The in-repo tail (bicubic .. 1x1 heads) IS pinned against the imported reference (tests/golden G11).
// The index kernels (voxelize, grid build, output sites, rulebook) are held to exact equality with brute-force references at cell
// edges, caps, key widths and volume seams by tests/test_gpu_sparse_index.py.
//
// Design: the grids are small enough (21 x 600 x 600 int32 = 30 MB per sample) to keep a DENSE row-index volume in HBM, so
// "hashing" is a plain load and output-site compaction is one exclusive scan in raster order (deterministic row order).
// The convolutions themselves run on the MFMA gather kernel (conv_mfma.hip, lm_conv_gather_mfma_f32).
#include "common.h"
#include "las_record.h"
#include "prim.h"

namespace {

constexpr unsigned INVALID_KEY = 0xFFFFFFFFu;

struct VoxGeom {
    float lo[3], vs[3];   // x, y, z
    int g[3];             // grid size x, y, z
};

// floor((p - lo) / vs) as an int, -1 where it is no cell index of any grid.  The range is decided on the FLOAT: a NaN fails every
// comparison, +-Inf and anything from 2^31 up fail one, so none of them reaches the conversion ((int)NaN is 0 on this hardware and
// would pass for cell 0).  Every value that does convert is an integer below 2^31 and converts exactly.
__device__ __forceinline__ int cell_index(float p, float lo, float vs) {
    const float f = floorf((p - lo) / vs);
    return (f >= 0.f && f < 2147483648.f) ? (int)f : -1;
}

__global__ __launch_bounds__(256) void vox_keys_kernel(const float4* __restrict__ pts, long n, VoxGeom G, unsigned* __restrict__ keys,
                                                       unsigned* __restrict__ vals, unsigned* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const int cx = cell_index(p.x, G.lo[0], G.vs[0]), cy = cell_index(p.y, G.lo[1], G.vs[1]), cz = cell_index(p.z, G.lo[2], G.vs[2]);
    const bool ok = cx >= 0 && cx < G.g[0] && cy >= 0 && cy < G.g[1] && cz >= 0 && cz < G.g[2];
    keys[i] = ok ? ((unsigned)cz * (unsigned)G.g[1] + (unsigned)cy) * (unsigned)G.g[0] + (unsigned)cx : INVALID_KEY;
    vals[i] = (unsigned)i;
    flags[i] = 0u;
}

__device__ __forceinline__ bool is_head(const unsigned* keys, long i) {
    const unsigned k = keys[i];
    return k != INVALID_KEY && (i == 0 || keys[i - 1] != k);
}

// sorted (stable) by cell: the first entry of a run is the voxel's first point -> flag it in point order
__global__ __launch_bounds__(256) void vox_heads_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, long n,
                                                        unsigned* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && is_head(keys, i)) flags[vals[i]] = 1u;
}

// rank[] = exclusive scan of flags in point order = voxel number in first-appearance order
__global__ __launch_bounds__(256) void vox_emit_kernel(const float4* __restrict__ pts, const unsigned* __restrict__ keys,
                                                       const unsigned* __restrict__ vals, const unsigned* __restrict__ rank,
                                                       const unsigned* __restrict__ flags, const unsigned* __restrict__ rrank,
                                                       long n, VoxGeom G, int max_points,
                                                       int max_voxels, int batch_idx, const int* __restrict__ row_base, int cap_rows,
                                                       float* __restrict__ feats, int ldf, int* __restrict__ coords,
                                                       int* __restrict__ row_end) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int base = row_base ? *row_base : 0;
    if (i == n - 1) {
        const unsigned total = rank[n - 1] + flags[n - 1];
        int nv = (int)(total < (unsigned)max_voxels ? total : (unsigned)max_voxels);
        if (base + nv > cap_rows) nv = cap_rows - base;   // host checks and reports the overflow
        *row_end = base + nv;
    }
    if (!is_head(keys, i)) return;
    unsigned v = rank[vals[i]];
    if (v >= (unsigned)max_voxels) return;                // the cap is defined on the first-appearance numbering
    if (rrank) v = rrank[i];                              // raster-order numbering of the kept voxels
    if (base + (long)v >= cap_rows) return;
    const unsigned k = keys[i];
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
    int cnt = 0;
    for (long j = i; j < n && cnt < max_points && keys[j] == k; ++j, ++cnt) {
        const float4 p = pts[vals[j]];
        sx += p.x;
        sy += p.y;
        sz += p.z;
        sw += p.w;
    }
    const float c = (float)cnt;
    float* f = feats + (long)(base + v) * ldf;
    f[0] = sx / c;
    f[1] = sy / c;
    f[2] = sz / c;
    f[3] = sw / c;
    for (int e = 4; e < ldf; ++e) f[e] = 0.f;
    int* o = coords + (long)(base + v) * 4;
    const int cx = (int)(k % (unsigned)G.g[0]);
    const unsigned t = k / (unsigned)G.g[0];
    o[0] = batch_idx;
    o[1] = (int)(t / (unsigned)G.g[1]);
    o[2] = (int)(t % (unsigned)G.g[1]);
    o[3] = cx;
}

// kept[i] (sorted position) = head of a voxel that survives the max_voxels cap; its exclusive scan numbers the kept
// voxels in (z, y, x) raster order, which is the order the radix sort left them in
__global__ __launch_bounds__(256) void vox_kept_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                       const unsigned* __restrict__ rank, long n, int max_voxels,
                                                       unsigned* __restrict__ kept) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) kept[i] = (is_head(keys, i) && rank[vals[i]] < (unsigned)max_voxels) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void fill_i32_kernel(int* __restrict__ p, long n, int v) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

struct Grid3 {
    int B, D, H, W;
};
struct Conv3 {
    int k[3], s[3], p[3];   // z, y, x
};

__device__ __forceinline__ long cell_of(const Grid3& g, int b, int z, int y, int x) { return (((long)b * g.D + z) * g.H + y) * g.W + x; }

__global__ __launch_bounds__(256) void grid_scatter_kernel(const int* __restrict__ coords, long n, Grid3 g, int* __restrict__ grid) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int* c = coords + i * 4;
    grid[cell_of(g, c[0], c[1], c[2], c[3])] = (int)i;
}

// every active input marks the output sites whose window contains it
__global__ __launch_bounds__(256) void conv_mark_kernel(const int* __restrict__ coords, long n, Conv3 cv, Grid3 go, int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int* c = coords + i * 4;
    for (int kz = 0; kz < cv.k[0]; ++kz) {
        const int tz = c[1] + cv.p[0] - kz;
        if (tz < 0 || tz % cv.s[0]) continue;
        const int oz = tz / cv.s[0];
        if (oz >= go.D) continue;
        for (int ky = 0; ky < cv.k[1]; ++ky) {
            const int ty = c[2] + cv.p[1] - ky;
            if (ty < 0 || ty % cv.s[1]) continue;
            const int oy = ty / cv.s[1];
            if (oy >= go.H) continue;
            for (int kx = 0; kx < cv.k[2]; ++kx) {
                const int tx = c[3] + cv.p[2] - kx;
                if (tx < 0 || tx % cv.s[2]) continue;
                const int ox = tx / cv.s[2];
                if (ox >= go.W) continue;
                flags[cell_of(go, c[0], oz, oy, ox)] = 1;
            }
        }
    }
}

// flags + exclusive scan -> row-index grid (-1 = inactive) and the output coordinate list in raster order
__global__ __launch_bounds__(256) void conv_compact_kernel(const int* __restrict__ flags, const int* __restrict__ ids, long cells, Grid3 go,
                                                           int cap_rows, int* __restrict__ grid, int* __restrict__ coords,
                                                           int* __restrict__ count) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    if (i == cells - 1) *count = ids[i] + flags[i];
    const int id = ids[i];
    if (!flags[i] || id >= cap_rows) {
        grid[i] = -1;
        return;
    }
    grid[i] = id;
    long t = i;
    const int x = (int)(t % go.W);
    t /= go.W;
    const int y = (int)(t % go.H);
    t /= go.H;
    const int z = (int)(t % go.D);
    int* o = coords + (long)id * 4;
    o[0] = (int)(t / go.D);
    o[1] = z;
    o[2] = y;
    o[3] = x;
}

// nbr[row][tap] = input row feeding output `row` through kernel tap (kz, ky, kx), -1 if that site is inactive / outside
__global__ __launch_bounds__(256) void rulebook_kernel(const int* __restrict__ out_coords, long n, Conv3 cv, Grid3 gi,
                                                       const int* __restrict__ in_grid, int* __restrict__ nbr) {
    const int taps = cv.k[0] * cv.k[1] * cv.k[2];
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * taps) return;
    const long row = e / taps;
    int t = (int)(e - row * taps);
    const int kx = t % cv.k[2];
    t /= cv.k[2];
    const int ky = t % cv.k[1];
    const int kz = t / cv.k[1];
    const int* c = out_coords + row * 4;
    const int z = c[1] * cv.s[0] - cv.p[0] + kz, y = c[2] * cv.s[1] - cv.p[1] + ky, x = c[3] * cv.s[2] - cv.p[2] + kx;
    int r = -1;
    if ((unsigned)z < (unsigned)gi.D && (unsigned)y < (unsigned)gi.H && (unsigned)x < (unsigned)gi.W)
        r = in_grid[cell_of(gi, c[0], z, y, x)];
    nbr[e] = r;
}

// dense()[b, c, z, y, x] -> NHWC image [b][H-1-y or y][x][c*D + z]; one 64-lane wave per active row
__global__ __launch_bounds__(256) void densify_kernel(const float* __restrict__ feats, int ldf, const int* __restrict__ coords, long n,
                                                      Grid3 g, int C, int flip_h, float* __restrict__ out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int* c = coords + row * 4;
    const int y = flip_h ? g.H - 1 - c[2] : c[2];
    float* o = out + (((long)c[0] * g.H + y) * g.W + c[3]) * ((long)C * g.D);
    for (int ch = threadIdx.x & 63; ch < C; ch += 64) o[(long)ch * g.D + c[1]] = feats[row * ldf + ch];
}

__device__ __forceinline__ float cubic1(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.f; }                 // |x| <= 1, A = -0.75
__device__ __forceinline__ float cubic2(float x) { return ((-0.75f * x + 3.75f) * x - 6.f) * x + 3.f; }          // 1 < |x| < 2

// torch upsample_bicubic2d, align_corners=False: src = (dst + 0.5) * in/out - 0.5, taps clamped to the border
__global__ __launch_bounds__(256) void bicubic_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C,
                                                      int Ho, int Wo, float sh, float sw) {
    const int c4n = C / 4;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * Ho * Wo * c4n) return;
    const int c4 = (int)(e % c4n);
    long t = e / c4n;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    const float ry = sh * ((float)oy + 0.5f) - 0.5f, rx = sw * ((float)ox + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    const float ty = ry - fy, tx = rx - fx;
    const int iy = (int)fy, ix = (int)fx;
    const float wy[4] = {cubic2(ty + 1.f), cubic1(ty), cubic1(1.f - ty), cubic2(2.f - ty)};
    const float wx[4] = {cubic2(tx + 1.f), cubic1(tx), cubic1(1.f - tx), cubic2(2.f - tx)};
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int yy = min(max(iy - 1 + a, 0), H - 1);
        float4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int xx = min(max(ix - 1 + q, 0), W - 1);
            const float4 v = *reinterpret_cast<const float4*>(x + (((long)b * H + yy) * W + xx) * C + c4 * 4);
            r.x += v.x * wx[q];
            r.y += v.y * wx[q];
            r.z += v.z * wx[q];
            r.w += v.w * wx[q];
        }
        acc.x += r.x * wy[a];
        acc.y += r.y * wy[a];
        acc.z += r.z * wy[a];
        acc.w += r.w * wy[a];
    }
    *reinterpret_cast<float4*>(y + (((long)b * Ho + oy) * Wo + ox) * C + c4 * 4) = acc;
}

size_t sort_temp_bytes(long n) { return lm_prim_sort_temp_bytes(n); }       // (prim.hip: the library's own radix sort and scan)
size_t scan_temp_bytes(long n) { return lm_prim_scan_temp_bytes(n); }

}  // namespace

LM_API long lm_voxelize_workspace_bytes(long n_points) {
    const long n = n_points > 0 ? n_points : 1;
    const size_t t1 = sort_temp_bytes(n), t2 = scan_temp_bytes(n);
    return (long)(8 * lm_align256((size_t)n * 4) + lm_align256(t1 > t2 ? t1 : t2));
}

// points [n,4] f32 (x, y, z, intensity) of ONE sample -> rows [*row_base, *row_end) of feats [cap_rows, ldf] (mean of the
// kept points, channels 4.. zero) and coords [cap_rows, 4] int32 (batch_idx, z, y, x).  row_base / row_end are DEVICE ints
// so that the samples of a batch chain without a host round trip (row_base == NULL means 0).  Row order inside the sample:
// raster_order == 0: the reference's (voxels numbered by their first point); 1: (z, y, x) raster order of the same voxel set
// (what the sparse convolutions want: spatial neighbours are row neighbours, so rulebook gathers hit in L2).
LM_API int lm_voxelize_hard(void* stream, const float* points, long n, const float* range_lo_xyz, const float* voxel_size_xyz,
                            const int* grid_xyz, int max_points, int max_voxels, int batch_idx, const int* row_base, int cap_rows,
                            float* feats, int ldf, int* coords, int* row_end, int raster_order, void* workspace,
                            long workspace_bytes) {
    LM_REQUIRE(range_lo_xyz && voxel_size_xyz && grid_xyz && feats && coords && row_end && workspace, "voxelize: null pointer");
    LM_REQUIRE(points || n == 0, "voxelize: null points");
    LM_REQUIRE(n >= 0 && n < (1L << 31) && ldf >= 4 && max_points >= 1 && max_voxels >= 1 && cap_rows >= 1, "voxelize: bad sizes");
    LM_REQUIRE((long)grid_xyz[0] * grid_xyz[1] * grid_xyz[2] < (long)INVALID_KEY && grid_xyz[0] > 0 && grid_xyz[1] > 0 && grid_xyz[2] > 0,
               "voxelize: grid too large");
    LM_REQUIRE(lm_voxelize_workspace_bytes(n) <= workspace_bytes, "voxelize: workspace too small (%ld B needed)",
               lm_voxelize_workspace_bytes(n));
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {   // no points: the sample contributes no rows
        if (row_base) LM_HIP(hipMemcpyAsync(row_end, row_base, sizeof(int), hipMemcpyDeviceToDevice, s));
        else LM_HIP(lm_zero_async(row_end, sizeof(int), s));
        return LM_OK;
    }
    VoxGeom G;
    for (int a = 0; a < 3; ++a) {
        G.lo[a] = range_lo_xyz[a];
        G.vs[a] = voxel_size_xyz[a];
        G.g[a] = grid_xyz[a];
        LM_REQUIRE(G.vs[a] > 0.f, "voxelize: voxel size must be positive");
    }
    const size_t seg = lm_align256((size_t)n * 4);
    char* w = (char*)workspace;
    unsigned *keys_in = (unsigned*)w, *keys_out = (unsigned*)(w + seg), *vals_in = (unsigned*)(w + 2 * seg),
             *vals_out = (unsigned*)(w + 3 * seg), *flags = (unsigned*)(w + 4 * seg), *rank = (unsigned*)(w + 5 * seg);
    unsigned *kept = (unsigned*)(w + 6 * seg), *rrank = (unsigned*)(w + 7 * seg);
    void* temp = w + 8 * seg;
    size_t t1 = sort_temp_bytes(n), t2 = scan_temp_bytes(n);
    const int blocks = lm_cdiv(n, 256);
    const float4* p4 = reinterpret_cast<const float4*>(points);
    hipLaunchKernelGGL(vox_keys_kernel, dim3(blocks), dim3(256), 0, s, p4, n, G, keys_in, vals_in, flags);
    LM_LAUNCH_CHECK();
    // stable sort by cell: only the bits a cell index can have take part, chosen so that the all-ones INVALID_KEY still sorts last
    const long cells = (long)grid_xyz[0] * grid_xyz[1] * grid_xyz[2];
    int end_bit = 8;
    while (end_bit < 32 && cells > (1L << end_bit) - 1) end_bit += 8;
    {
        unsigned *kr = nullptr, *vr = nullptr;
        const int rc = lm_prim_sort_pairs_u32(s, keys_in, keys_out, vals_in, vals_out, n, end_bit, temp, t1, &kr, &vr);
        if (rc != LM_OK) return rc;
        keys_out = kr;
        vals_out = vr;
    }
    hipLaunchKernelGGL(vox_heads_kernel, dim3(blocks), dim3(256), 0, s, keys_out, vals_out, n, flags);
    LM_LAUNCH_CHECK();
    {
        const int rc = lm_prim_exclusive_scan_u32(s, flags, rank, n, temp, t2);
        if (rc != LM_OK) return rc;
    }
    if (raster_order) {
        hipLaunchKernelGGL(vox_kept_kernel, dim3(blocks), dim3(256), 0, s, keys_out, vals_out, rank, n, max_voxels, kept);
        LM_LAUNCH_CHECK();
        const int rc = lm_prim_exclusive_scan_u32(s, kept, rrank, n, temp, t2);
        if (rc != LM_OK) return rc;
    }
    hipLaunchKernelGGL(vox_emit_kernel, dim3(blocks), dim3(256), 0, s, p4, keys_out, vals_out, rank, flags,
                       raster_order ? rrank : (const unsigned*)nullptr, n, G, max_points, max_voxels,
                       batch_idx, row_base, cap_rows, feats, ldf, coords, row_end);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// grid [B, D, H, W] int32 := -1, then grid[coords[i]] = i
LM_API int lm_sparse_grid_build(void* stream, const int* coords, long n, int* grid, int B, int D, int H, int W) {
    LM_REQUIRE(grid && (coords || n == 0) && B > 0 && D > 0 && H > 0 && W > 0, "sparse_grid_build: bad args");
    const long cells = (long)B * D * H * W;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fill_i32_kernel, dim3(lm_cdiv(cells, 256)), dim3(256), 0, s, grid, cells, -1);
    LM_LAUNCH_CHECK();
    if (n > 0) {
        hipLaunchKernelGGL(grid_scatter_kernel, dim3(lm_cdiv(n, 256)), dim3(256), 0, s, coords, n, Grid3{B, D, H, W}, grid);
        LM_LAUNCH_CHECK();
    }
    return LM_OK;
}

LM_API long lm_sparse_conv_outputs_workspace_bytes(long out_cells) {
    const long n = out_cells > 0 ? out_cells : 1;
    return (long)(2 * lm_align256((size_t)n * 4) + lm_align256(scan_temp_bytes(n)));
}

// Active output sites of a SparseConv3d (kernel / stride / padding in z, y, x order) over the input rows `in_coords`:
// out_grid [B, Do, Ho, Wo] receives the output row index of every site (-1 inactive), out_coords the sites in raster
// order, *out_count (device int) their number (may exceed cap_rows: rows beyond it are dropped, the host must check).
LM_API int lm_sparse_conv_outputs(void* stream, const int* in_coords, long n_in, int B, const int* ksp_zyx9, int Do, int Ho, int Wo,
                                  int* out_grid, int* out_coords, int cap_rows, int* out_count, void* workspace, long workspace_bytes) {
    LM_REQUIRE(in_coords && ksp_zyx9 && out_grid && out_coords && out_count && workspace && n_in > 0, "sparse_conv_outputs: bad args");
    const long cells = (long)B * Do * Ho * Wo;
    LM_REQUIRE(cells > 0 && cells < (1L << 31), "sparse_conv_outputs: bad output grid");
    LM_REQUIRE(lm_sparse_conv_outputs_workspace_bytes(cells) <= workspace_bytes, "sparse_conv_outputs: workspace too small");
    Conv3 cv;
    for (int a = 0; a < 3; ++a) {
        cv.k[a] = ksp_zyx9[a];
        cv.s[a] = ksp_zyx9[3 + a];
        cv.p[a] = ksp_zyx9[6 + a];
        LM_REQUIRE(cv.k[a] >= 1 && cv.s[a] >= 1 && cv.p[a] >= 0, "sparse_conv_outputs: bad kernel geometry");
    }
    const size_t seg = lm_align256((size_t)cells * 4);
    char* w = (char*)workspace;
    int *flags = (int*)w, *ids = (int*)(w + seg);
    void* temp = w + 2 * seg;
    size_t tb = scan_temp_bytes(cells);
    hipStream_t s = (hipStream_t)stream;
    const Grid3 go{B, Do, Ho, Wo};
    LM_HIP(lm_zero_async(flags, (size_t)cells * 4, s));
    hipLaunchKernelGGL(conv_mark_kernel, dim3(lm_cdiv(n_in, 256)), dim3(256), 0, s, in_coords, n_in, cv, go, flags);
    LM_LAUNCH_CHECK();
    {
        const int rc = lm_prim_exclusive_scan_u32(s, (const unsigned*)flags, (unsigned*)ids, cells, temp, tb);
        if (rc != LM_OK) return rc;
    }
    hipLaunchKernelGGL(conv_compact_kernel, dim3(lm_cdiv(cells, 256)), dim3(256), 0, s, flags, ids, cells, go, cap_rows, out_grid,
                       out_coords, out_count);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// nbr [n_out, kz*ky*kx] int32: input row under every kernel tap of every output row (SubMConv3d: out == in, stride 1,
// pad = k/2; SparseConv3d: the layer's own geometry).  in_grid is the [B, D, H, W] row-index volume of the INPUT.
LM_API int lm_sparse_rulebook(void* stream, const int* out_coords, long n_out, const int* in_grid, int B, int D, int H, int W,
                              const int* ksp_zyx9, int* nbr) {
    LM_REQUIRE(out_coords && in_grid && ksp_zyx9 && nbr && n_out > 0, "sparse_rulebook: bad args");
    Conv3 cv;
    for (int a = 0; a < 3; ++a) {
        cv.k[a] = ksp_zyx9[a];
        cv.s[a] = ksp_zyx9[3 + a];
        cv.p[a] = ksp_zyx9[6 + a];
    }
    const long total = n_out * cv.k[0] * cv.k[1] * cv.k[2];
    hipLaunchKernelGGL(rulebook_kernel, dim3(lm_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, out_coords, n_out, cv,
                       Grid3{B, D, H, W}, in_grid, nbr);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// SparseConvTensor.dense() -> view(N, C*D, H, W) -> optional flip of H, written channels-last: out [B, H, W, C*D]
LM_API int lm_sparse_to_dense_nhwc(void* stream, const float* feats, int ldf, const int* coords, long n, float* out, int B, int D,
                                   int H, int W, int C, int flip_h) {
    LM_REQUIRE(out && (n == 0 || (feats && coords)) && ldf >= C && C > 0, "sparse_to_dense: bad args");
    hipStream_t s = (hipStream_t)stream;
    LM_HIP(lm_zero_async(out, (size_t)B * D * H * W * C * sizeof(float), s));
    if (n > 0) {
        hipLaunchKernelGGL(densify_kernel, dim3(lm_cdiv(n, 4)), dim3(256), 0, s, feats, ldf, coords, n, Grid3{B, D, H, W}, C, flip_h, out);
        LM_LAUNCH_CHECK();
    }
    return LM_OK;
}

// F.interpolate(mode='bicubic', align_corners=False) on an NHWC tensor (lidarencoder.py:72)
LM_API int lm_upsample_bicubic_nhwc(void* stream, const float* x, float* y, int B, int H, int W, int C, int Ho, int Wo) {
    LM_REQUIRE(x && y && B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0 && C % 4 == 0, "upsample_bicubic: bad args (C=%d)", C);
    const long total = (long)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(bicubic_kernel, dim3(lm_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, B, H, W, C, Ho, Wo,
                       (float)H / (float)Ho, (float)W / (float)Wo);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// LAS point records -> [N,4] f32 in HBM (the reference reads LAS through laspy on the host,
// baseline/datasets/laserlane_proposals.py:618-636 `read_las`: positions = X * scale + offset, intensity clipped to
// [800, 33000] then (i - 800) / 33000).  ASPRS LAS 1.0-1.4, point data record formats 0-10: every format starts with
// X, Y, Z (int32 LE) and intensity (uint16 LE); the rest of the record is skipped.  HBM-bound byte work: a workgroup stages
// 256 records with coalesced dword loads into LDS and each lane decodes one record from there.
namespace {

__global__ __launch_bounds__(256) void las_decode_kernel(const unsigned* __restrict__ rec, int record_len, long n, double sx, double sy,
                                                         double sz, double ox, double oy, double oz, float lo, float hi, int normalise,
                                                         float4* __restrict__ out) {
    extern __shared__ unsigned stage[];
    const long first = (long)blockIdx.x * 256;
    const long cnt = n - first < 256 ? n - first : 256;
    const long byte0 = first * record_len;                       // multiple of 256 * record_len => 4-byte aligned
    const long words = (cnt * record_len + 3) / 4;
    const unsigned* src = rec + byte0 / 4;
    for (long w = threadIdx.x; w < words; w += 256) stage[w] = src[w];
    __syncthreads();
    if (threadIdx.x >= cnt) return;
    const unsigned char* r = reinterpret_cast<const unsigned char*>(stage) + (long)threadIdx.x * record_len;
    auto i32 = [&](int o) { return (int)((unsigned)r[o] | ((unsigned)r[o + 1] << 8) | ((unsigned)r[o + 2] << 16) | ((unsigned)r[o + 3] << 24)); };
    const double x = (double)i32(0) * sx + ox, y = (double)i32(4) * sy + oy, z = (double)i32(8) * sz + oz;
    const double raw = (double)((unsigned)r[12] | ((unsigned)r[13] << 8));
    const double it = normalise ? (fmin(fmax(raw, (double)lo), (double)hi) - (double)lo) / (double)hi : raw;   // f64 like read_las
    out[first + threadIdx.x] = float4{(float)x, (float)y, (float)z, (float)it};
}

unsigned short rd16(const unsigned char* p) { return (unsigned short)(p[0] | (p[1] << 8)); }
unsigned rd32(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24); }
unsigned long rd64(const unsigned char* p) { return (unsigned long)rd32(p) | ((unsigned long)rd32(p + 4) << 32); }
double rdf64(const unsigned char* p) {
    unsigned long v = rd64(p);
    double d;
    __builtin_memcpy(&d, &v, 8);
    return d;
}

}  // namespace

// Parse the LAS public header block (HOST bytes).  Errors: not a LAS file, truncated, compressed (LAZ) or unknown format.
LM_API int lm_las_parse_header(const unsigned char* bytes, long len, LmLasHeader* h) {
    LM_REQUIRE(bytes && h, "las_parse_header: null pointer");
    LM_REQUIRE(len >= 227 && bytes[0] == 'L' && bytes[1] == 'A' && bytes[2] == 'S' && bytes[3] == 'F', "las_parse_header: not a LAS file");
    h->version_major = bytes[24];
    h->version_minor = bytes[25];
    const int header_size = rd16(bytes + 94);
    h->offset_to_points = rd32(bytes + 96);
    const int fmt = bytes[104];
    LM_REQUIRE((fmt & 0x80) == 0 && (fmt & 0x40) == 0, "las_parse_header: compressed (LAZ) point data is not supported");
    h->point_format = fmt & 0x3F;
    LM_REQUIRE(h->point_format <= 10, "las_parse_header: unknown point data record format %d", h->point_format);
    h->record_len = rd16(bytes + 105);
    h->n_points = rd32(bytes + 107);                              // legacy count
    for (int a = 0; a < 3; ++a) {
        h->scale[a] = rdf64(bytes + 131 + 8 * a);
        h->offset[a] = rdf64(bytes + 155 + 8 * a);
        h->max_xyz[a] = rdf64(bytes + 179 + 16 * a);
        h->min_xyz[a] = rdf64(bytes + 187 + 16 * a);
    }
    if (h->version_major == 1 && h->version_minor >= 4) {
        LM_REQUIRE(len >= 375 && header_size >= 375, "las_parse_header: truncated LAS 1.4 header");
        const long n64 = (long)rd64(bytes + 247);
        if (n64 > 0) h->n_points = n64;
    }
    LM_REQUIRE(h->record_len >= las_min_len[h->point_format], "las_parse_header: record length %d too short for format %d", h->record_len,
               h->point_format);
    LM_REQUIRE(h->offset_to_points >= header_size && h->offset_to_points + h->n_points * h->record_len <= len,
               "las_parse_header: point data (%ld records of %d B at %ld) exceeds the file (%ld B)", h->n_points, h->record_len,
               h->offset_to_points, len);
    return LM_OK;
}

// records: DEVICE copy of the point data (4-byte aligned, n * record_len bytes rounded up to a multiple of 4).
// out [n,4] f32 = X*scale + (offset - shift) evaluated in f64 (shift = the tile's las_read_offset keeps f32 exact to the mm), intensity raw (normalise == 0, what lm_bev_raster_batch takes) or read_las's (clip - lo) / hi.
LM_API int lm_las_decode_points(void* stream, const unsigned char* records, int record_len, long n, const double* scale,
                                const double* offset, const double* shift, float inten_lo, float inten_hi, int normalise,
                                float* out_xyzi) {
    LM_REQUIRE(scale && offset && out_xyzi && (records || n == 0), "las_decode_points: null pointer");
    // (not las_check_records: no format is given, any record_len in 20 .. 160 is taken, and the refusal has its own words)
    LM_REQUIRE(record_len >= 20 && record_len <= 160 && n >= 0, "las_decode_points: bad record length %d", record_len);
    LM_REQUIRE(((uintptr_t)records & 3) == 0 && ((uintptr_t)out_xyzi & 15) == 0, "las_decode_points: buffers must be 4 / 16-byte aligned");
    if (n == 0) return LM_OK;
    const LasXf X = las_xf(scale, offset, shift, inten_lo, inten_hi, normalise);
    hipLaunchKernelGGL(las_decode_kernel, dim3(lm_cdiv(n, 256)), dim3(256), las_stage_bytes(record_len), (hipStream_t)stream,
                       reinterpret_cast<const unsigned*>(records), record_len, n, X.sx, X.sy, X.sz, X.ox, X.oy, X.oz, X.lo, X.hi, X.normalise,
                       reinterpret_cast<float4*>(out_xyzi));
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// Decode + select + stable compaction: the records that pass a predicate on classification, flag bits, return numbers and
// decoded height, written densely in file order.  Formats 0-5 and 6-10 keep these fields in different bits of bytes 14-16:
//                      return number   number of returns   classification   synthetic / key-point / withheld / overlap
//   formats 0-5        byte 14 [0:2]   byte 14 [3:5]       byte 15 [0:4]    byte 15 bits 5 / 6 / 7 / (does not exist)
//   formats 6-10       byte 14 [0:3]   byte 14 [4:7]       byte 16          byte 15 bits 0 / 1 / 2 / 3
// Three launches, nothing read back: a count pass (kept records of every 256-record block, and LDS class counters of all records),
// prim.hip's exclusive scan over the block counts, and an emit pass that re-evaluates the predicate and stores to block offset + rank,
// the rank from a ballot (lanes are in file order) plus the counts of the waves before.  Every slot is reserved by a prefix: no
// atomics on HBM, the same bits each run.  HBM traffic = 2 n record_len read + 16 kept written + 4 bytes per block.
namespace {

constexpr int SEL_HIST_GROUPS = 2048;   // most workgroups of the count pass (8 resident per CU) = columns of the partial class histogram

// (LasXf, LasSel, las_record_xyzi, las_record_keep and las_stage_block: las_record.h, shared with label.hip and profile.hip)
// counts[b] = kept records of block b, counts[nblk] = 0 (the scan turns it into the total); hist_part (may be NULL) [256][gridDim.x]:
// the classes of ALL records this workgroup walked, counted in LDS and written once
__global__ __launch_bounds__(256) void las_select_count_kernel(const unsigned* __restrict__ rec, int record_len, long n, long nblk, LasXf X,
                                                               LasSel S, unsigned* __restrict__ counts, unsigned* __restrict__ hist_part) {
    extern __shared__ unsigned sel_stage[];
    __shared__ unsigned hist[256];
    __shared__ unsigned wcnt[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (hist_part) hist[threadIdx.x] = 0u;                         // (the barrier of the first staging orders this before the adds)
    for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int cnt = las_stage_block(rec, record_len, n, b, sel_stage);
        bool keep = false;
        if ((int)threadIdx.x < cnt) {
            unsigned cls;
            float4 p;
            keep = las_record_keep(reinterpret_cast<const unsigned char*>(sel_stage) + (int)threadIdx.x * record_len, X, S, cls, p);
            if (hist_part) atomicAdd(&hist[cls], 1u);
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wcnt[wv] = (unsigned)__popcll(bal);
        __syncthreads();                                           // also: the stage is free for the next block
        if (threadIdx.x == 0) counts[b] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[nblk] = 0u;
    if (hist_part) {
        __syncthreads();
        hist_part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
    }
}

// one wave per class: the sum of its row of partial counts (integers: exact whatever the order), 64 workgroups
__global__ __launch_bounds__(256) void las_select_hist_kernel(const unsigned* __restrict__ hist_part, int groups, unsigned long* __restrict__ hist) {
    const int bin = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    unsigned long long s = 0;
    for (int g = lane; g < groups; g += 64) s += hist_part[(size_t)bin * groups + g];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (lane == 0) hist[bin] = (unsigned long)s;
}

// offs = the scanned counts; one workgroup per block of 256 records
__global__ __launch_bounds__(256) void las_select_emit_kernel(const unsigned* __restrict__ rec, int record_len, long n, long nblk, LasXf X,
                                                              LasSel S, const unsigned* __restrict__ offs, float4* __restrict__ out,
                                                              long* __restrict__ kept) {
    extern __shared__ unsigned sel_stage[];
    __shared__ unsigned wcnt[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long b = blockIdx.x;
    const int cnt = las_stage_block(rec, record_len, n, b, sel_stage);
    bool keep = false;
    float4 p = {0.f, 0.f, 0.f, 0.f};
    if ((int)threadIdx.x < cnt) {
        unsigned cls;
        keep = las_record_keep(reinterpret_cast<const unsigned char*>(sel_stage) + (int)threadIdx.x * record_len, X, S, cls, p);
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wcnt[wv] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < wv) before += wcnt[k];
    // offs[b] + rank < offs[nblk] <= n: the count pass evaluated the same predicate on the same bytes
    if (keep) out[(long)offs[b] + before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = p;
    if (b == 0 && threadIdx.x == 0) *kept = (long)offs[nblk];
}

long sel_blocks(long n) { return (n + 255) / 256; }
long sel_groups(long n) { return sel_blocks(n) < SEL_HIST_GROUPS ? sel_blocks(n) : SEL_HIST_GROUPS; }

}  // namespace

LM_API long lm_las_select_workspace_bytes(long n) {
    if (n < 0 || n > 2147483647L) return 0;
    const long L = sel_blocks(n) + 1;
    return (long)(lm_align256((size_t)L * 4) + lm_align256(scan_temp_bytes(L)) + lm_align256((size_t)256 * (n ? sel_groups(n) : 1) * 4));
}

// lm_las_decode_points restricted to the records that pass `select`: out_xyzi[0 .. *kept) = the rows the plain decode writes for them,
// in file order; rows from *kept on are not written.  kept: DEVICE long.  class_hist: DEVICE [256] u64 or NULL, the classification of
// all n records.  Asynchronous like the plain decode: the caller reads *kept back when it needs the number.
LM_API int lm_las_decode_select(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                                const double* scale, const double* offset, const double* shift, float inten_lo, float inten_hi,
                                int normalise, const LmLasSelect* select, void* workspace, long workspace_bytes, float* out_xyzi,
                                long* kept, unsigned long* class_hist) {
    // (not las_check_records: any record_len in 20 .. 160 is taken whatever the format, and the refusals have their own words)
    LM_REQUIRE(record_len >= 20 && record_len <= 160, "las_decode_select: bad record length %d", record_len);
    LM_REQUIRE(n >= 0 && n <= 2147483647L, "las_decode_select: n=%ld records, at most 2^31 - 1 are supported", n);
    LM_REQUIRE(point_format >= 0 && point_format <= 10, "las_decode_select: unknown point data record format %d", point_format);
    LM_REQUIRE(scale && offset && select && kept && (n == 0 || (records && out_xyzi && workspace)), "las_decode_select: null pointer");
    LasSel S;
    if (int e = las_check_select("las_decode_select", "", select, point_format, S)) return e;
    LM_REQUIRE(((uintptr_t)records & 3) == 0 && ((uintptr_t)out_xyzi & 15) == 0 && ((uintptr_t)workspace & 3) == 0 &&
                   ((uintptr_t)kept & 7) == 0 && ((uintptr_t)class_hist & 7) == 0,
               "las_decode_select: buffers must be 4 / 16 / 4 / 8 / 8-byte aligned");
    LM_REQUIRE(lm_las_select_workspace_bytes(n) <= workspace_bytes, "las_decode_select: workspace too small (%ld B needed)",
               lm_las_select_workspace_bytes(n));
    hipStream_t s = (hipStream_t)hip_stream;
    if (n == 0) {
        LM_HIP(lm_zero_async(kept, sizeof(long), s));
        if (class_hist) LM_HIP(lm_zero_async(class_hist, 256 * sizeof(unsigned long), s));
        return LM_OK;
    }
    const LasXf X = las_xf(scale, offset, shift, inten_lo, inten_hi, normalise);
    const long nblk = sel_blocks(n), L = nblk + 1;
    const int groups = (int)sel_groups(n);
    char* w = (char*)workspace;
    unsigned* counts = (unsigned*)w;
    w += lm_align256((size_t)L * 4);
    void* scan_tmp = w;
    const size_t scan_bytes = lm_align256(scan_temp_bytes(L));
    w += scan_bytes;
    unsigned* hist_part = class_hist ? (unsigned*)w : nullptr;
    const size_t lds = las_stage_bytes(record_len);
    const unsigned* rec = reinterpret_cast<const unsigned*>(records);
    hipLaunchKernelGGL(las_select_count_kernel, dim3((unsigned)groups), dim3(256), lds, s, rec, record_len, n, nblk, X, S, counts, hist_part);
    LM_LAUNCH_CHECK();
    if (class_hist) {
        hipLaunchKernelGGL(las_select_hist_kernel, dim3(64), dim3(256), 0, s, hist_part, groups, class_hist);
        LM_LAUNCH_CHECK();
    }
    if (int e = lm_prim_exclusive_scan_u32(s, counts, counts, L, scan_tmp, scan_bytes)) return e;
    hipLaunchKernelGGL(las_select_emit_kernel, dim3((unsigned)nblk), dim3(256), lds, s, rec, record_len, n, nblk, X, S, counts,
                       reinterpret_cast<float4*>(out_xyzi), kept);
    LM_LAUNCH_CHECK();
    return LM_OK;
}
