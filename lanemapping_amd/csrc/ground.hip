// Per-tile ground model of the strip route: a coarse grid of ground heights under every tile, out of the points already binned for the
// rasteriser, and the selection of points by their height above it.  Input of both entries is the (points, tile_offsets, params) triple
// lm_bev_raster_batch takes, walked with the scaffold of tile_points.h (tile constants, workgroup -> tile, streaming loop, key of a
// height, host prologue): a point counts for tile b exactly when raster.hip would keep it for b.  A point whose vz (the tile-frame
// height the rasteriser turns into G) is not finite counts nowhere and is never selected.
//
// The cell grid is Gy = ceil(H / cell_px) by Gx = ceil(W / cell_px); the cell of a point is (row / cell_px, col / cell_px).
//   (a) cell minima   a workgroup streams one chunk of GCHUNK = 16,384 points of one tile (lm_stream_points: 256 lanes x 64 loads, 8 in
//                     flight per lane), keeps the tile's Gy Gx minima in LDS as keys of vz (lm_key_of; 0xFFFFFFFF = empty) under LDS
//                     atomic min, and flushes its non-empty cells to keys [B][Gy][Gx] (memset to 0xFF) with integer atomic min: order
//                     independent, the same bits every run.  The minimum is taken on the key: -0.0 < +0.0.
//   (b) smoothing     one workgroup per tile: ground = lower median (element (k - 1) / 2 of the k keys in ascending order) of the
//                     non-empty cells of the 3 x 3 neighbourhood clipped at the grid edge, NaN for k = 0; ground_min = the minimum of the
//                     tile's finite ground cells, +inf when it has none.
//   (c) selection     kept <=> window test && vz finite && h_lo <= vz - ground[b][cell] <= h_hi (one f32 subtraction; a NaN ground keeps
//                     nothing).  Stable compaction per tile, the scheme of lm_las_decode_select: count per block of SEL_BLOCK = 256 points
//                     (blocks never straddle two tiles), exclusive scan (prim.hip), emit to block offset + ballot rank.  A workgroup
//                     takes SEL_GROUP = 8 consecutive blocks of one tile so that 8 loads per lane are in flight.  No atomics.
// HBM traffic: (a) 16 N read, (c) 32 N read + 16 kept written.
#include "common.h"
#include "prim.h"
#include "tile_points.h"

#include <cmath>
#include <vector>

namespace {

constexpr int GT = 256;                      // threads per workgroup, every kernel of this file
constexpr int G_PER_THREAD = 64;
constexpr int GCHUNK = GT * G_PER_THREAD;    // points per workgroup of (a)
constexpr int LB = 8;                        // loads in flight per lane
constexpr int SEL_BLOCK = 256;               // points per counted block of (c)
constexpr int SEL_GROUP = 8;                 // blocks per workgroup of (c)
constexpr int SEL_CHUNK = SEL_BLOCK * SEL_GROUP;
constexpr int MAX_CELLS = 32768;             // 128 KB of LDS keys

struct GroundTile : LmTileRange {            // cbase: chunks of (a), block groups of (c)
    long bbase;                              // 256-point blocks of the tiles before this one (c)
};
static_assert(sizeof(GroundTile) == 96 && alignof(GroundTile) == 16, "96 bytes per tile: lm_*_workspace_bytes");

// window test + finite height -> the point's cell; cdiv divides by cell_px
__device__ __forceinline__ bool point_cell(const f32x4 p, const GroundTile& X, int H, int W, const LmFastDiv& cdiv, int Gx, int& cell,
                                           float& vz) {
    int row, col;
    if (!lm_point_window(p, X, H, W, row, col, vz)) return false;
    if (!(fabsf(vz) < INFINITY)) return false;
    cell = (int)lm_fastdiv((unsigned)row, cdiv) * Gx + (int)lm_fastdiv((unsigned)col, cdiv);
    return true;
}

// (a) grid: sum over tiles of ceil(count / GCHUNK); dynamic LDS = ncell words
__global__ __launch_bounds__(GT) void ground_min_kernel(const f32x4* __restrict__ pts, const GroundTile* __restrict__ tiles, int B,
                                                        unsigned* __restrict__ keys, int H, int W, LmFastDiv cdiv, int Gx, int ncell) {
    extern __shared__ unsigned cmin[];
    const int tid = threadIdx.x;
    const int t = lm_tile_of(tiles, B, (long)blockIdx.x);
    const GroundTile X = tiles[t];
    const long first = ((long)blockIdx.x - X.cbase) * GCHUNK;
    const long left = X.count - first;                          // >= 1
    for (int i = tid; i < ncell; i += GT) cmin[i] = LM_KEY_EMPTY;
    __syncthreads();
    lm_stream_points<GT, G_PER_THREAD, LB>(pts + X.start + first, left, tid, [&](const f32x4 p, bool valid) {
        int cell;
        float vz;
        if (valid && point_cell(p, X, H, W, cdiv, Gx, cell, vz)) atomicMin(&cmin[cell], lm_key_of(vz));
    });
    __syncthreads();
    unsigned* dst = keys + (long)t * ncell;
    for (int i = tid; i < ncell; i += GT) {
        const unsigned k = cmin[i];
        if (k != LM_KEY_EMPTY) atomicMin(dst + i, k);
    }
}

// (b) grid: B workgroups
__global__ __launch_bounds__(GT) void ground_smooth_kernel(const unsigned* __restrict__ keys, float* __restrict__ ground,
                                                           float* __restrict__ ground_min, float* __restrict__ cell_min, int Gy, int Gx) {
    __shared__ unsigned tmin;
    const int tid = threadIdx.x, ncell = Gy * Gx;
    const long tile0 = (long)blockIdx.x * ncell;
    const unsigned* k = keys + tile0;
    if (tid == 0) tmin = LM_KEY_EMPTY;
    __syncthreads();
    unsigned mine = LM_KEY_EMPTY;
    for (int c = tid; c < ncell; c += GT) {
        const int cy = c / Gx, cx = c - cy * Gx;
        unsigned v[9];
        int n = 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const int y = cy + e / 3 - 1, x = cx + e % 3 - 1;
            v[e] = (y >= 0 && y < Gy && x >= 0 && x < Gx) ? k[y * Gx + x] : LM_KEY_EMPTY;
            n += v[e] != LM_KEY_EMPTY;
        }
        // the element of rank (n - 1) / 2; equal keys are ranked by their position, so exactly one element has each rank
        const int want = (n - 1) / 2;
        unsigned res = LM_KEY_EMPTY;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            int rank = 0;
#pragma unroll
            for (int f = 0; f < 9; ++f) rank += (v[f] < v[e]) || (f < e && v[f] == v[e]);
            if (v[e] != LM_KEY_EMPTY && rank == want) res = v[e];
        }
        ground[tile0 + c] = __uint_as_float(res == LM_KEY_EMPTY ? LM_QNAN_BITS : __float_as_uint(lm_value_of(res)));
        if (cell_min) cell_min[tile0 + c] = __uint_as_float(k[c] == LM_KEY_EMPTY ? LM_QNAN_BITS : __float_as_uint(lm_value_of(k[c])));
        mine = res < mine ? res : mine;
    }
    if (mine != LM_KEY_EMPTY) atomicMin(&tmin, mine);
    __syncthreads();
    if (tid == 0) ground_min[blockIdx.x] = tmin == LM_KEY_EMPTY ? INFINITY : lm_value_of(tmin);
}

// (c) grid: sum over tiles of ceil(count / SEL_CHUNK).  EMIT = false: counts[bbase + block] = kept points of the block;
// EMIT = true: counts holds the scanned counts, the kept points go to out[counts[block] + rank in the block]
template <bool EMIT>
__global__ __launch_bounds__(GT) void ground_select_kernel(const f32x4* __restrict__ pts, const GroundTile* __restrict__ tiles, int B,
                                                           const float* __restrict__ ground, int H, int W, LmFastDiv cdiv, int Gx, int ncell,
                                                           float h_lo, float h_hi, unsigned* __restrict__ counts, f32x4* __restrict__ out) {
    __shared__ unsigned wcnt[SEL_GROUP][GT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int t = lm_tile_of(tiles, B, (long)blockIdx.x);
    const GroundTile X = tiles[t];
    const long grp = (long)blockIdx.x - X.cbase;
    const long left = X.count - grp * SEL_CHUNK;                // >= 1
    const f32x4* base = pts + X.start + grp * SEL_CHUNK;
    const float* g = ground + (long)t * ncell;
    f32x4 p[SEL_GROUP];
#pragma unroll
    for (int j = 0; j < SEL_GROUP; ++j) {
        const long i = (long)j * SEL_BLOCK + tid;
        p[j] = __builtin_nontemporal_load(base + (i < left ? i : left - 1));
    }
    unsigned keep = 0;                                          // bit j: this lane's point of block j is kept
    unsigned long long bal[SEL_GROUP];
#pragma unroll
    for (int j = 0; j < SEL_GROUP; ++j) {
        const long i = (long)j * SEL_BLOCK + tid;
        int cell;
        float vz;
        bool k = i < left && point_cell(p[j], X, H, W, cdiv, Gx, cell, vz);
        if (k) {
            const float h = vz - g[cell];
            k = h >= h_lo && h <= h_hi;
        }
        bal[j] = __ballot(k);
        keep |= (unsigned)k << j;
        if (lane == 0) wcnt[j][wv] = (unsigned)__popcll(bal[j]);
    }
    __syncthreads();
    const int nblk = (int)((left < SEL_CHUNK ? left : SEL_CHUNK) + SEL_BLOCK - 1) / SEL_BLOCK;   // blocks of this group: 1 .. SEL_GROUP
    unsigned* cnt = counts + X.bbase + grp * SEL_GROUP;
    if (!EMIT) {
        if (tid < nblk) cnt[tid] = wcnt[tid][0] + wcnt[tid][1] + wcnt[tid][2] + wcnt[tid][3];
    } else {
#pragma unroll
        for (int j = 0; j < SEL_GROUP; ++j) {
            if (j >= nblk) break;
            unsigned before = 0;
#pragma unroll
            for (int w = 0; w < GT / 64 - 1; ++w)
                if (w < wv) before += wcnt[j][w];
            // cnt[j] + rank < total kept <= N: the count pass evaluated the same predicate on the same bytes
            if (keep >> j & 1u) out[(long)cnt[j] + before + (unsigned)__popcll(bal[j] & ((1ull << lane) - 1ull))] = p[j];
        }
    }
}

// scanned block counts -> out_offsets [B + 1] in 64 bits; nblocks = index of the terminating entry (the total)
__global__ __launch_bounds__(GT) void ground_offsets_kernel(const unsigned* __restrict__ scanned, const GroundTile* __restrict__ tiles, int B,
                                                            long nblocks, long* __restrict__ out_offsets) {
    const int t = blockIdx.x * GT + threadIdx.x;
    if (t < B) out_offsets[t] = (long)scanned[tiles[t].bbase];
    if (t == B) out_offsets[B] = (long)scanned[nblocks];
}

}  // namespace

// cell_px (named before the offsets are read), then the shared prologue; per = points per workgroup (cbase), bbase in blocks of SEL_BLOCK
static int derive_tiles(const char* who, const long* tile_offsets, const LmRasterParams* params, int B, int H, int W, int cell_px, long per,
                        std::vector<GroundTile>& out, long* n_wg, long* n_blocks, long* n_points) {
    LM_REQUIRE(cell_px >= 8 && cell_px <= 128, "%s: cell_px=%d, 8 to 128 are supported", who, cell_px);
    LM_REQUIRE(lm_cdivl(H, cell_px) * lm_cdivl(W, cell_px) <= MAX_CELLS, "%s: cell_px=%d gives %ld cells per tile, at most %d are supported",
               who, cell_px, lm_cdivl(H, cell_px) * lm_cdivl(W, cell_px), MAX_CELLS);
    long blocks = 0;
    const auto tile_blocks = [&](int, GroundTile& T, long&) -> int {
        T.bbase = blocks;
        blocks += lm_cdivl(T.count, SEL_BLOCK);
        return LM_OK;
    };
    if (int e = lm_tile_ranges(who, tile_offsets, params, B, 1, H, W, per, out, n_wg, n_points, tile_blocks)) return e;
    LM_REQUIRE(*n_points <= 2147483647L, "%s: %ld points, at most 2^31 - 1 are supported", who, *n_points);
    *n_blocks = blocks;
    return LM_OK;
}

LM_API long lm_tile_ground_workspace_bytes(int B, int H, int W, int cell_px) {
    if (B < 1 || B > LM_MAX_TILES || H <= 0 || W <= 0 || cell_px < 8 || cell_px > 128) return 0;
    const long ncell = lm_cdivl(H, cell_px) * lm_cdivl(W, cell_px);
    if (ncell > MAX_CELLS) return 0;
    return (long)(lm_align256((size_t)B * sizeof(GroundTile)) + lm_align256((size_t)B * ncell * 4));
}

// points: device [sum N][4]; tile_offsets: HOST [B+1]; params: HOST [B]; ground [B][Gy][Gx], ground_min [B], cell_min [B][Gy][Gx] or NULL:
// device f32.  Asynchronous, but copies host memory of this call to the device: refuses a capturing stream (common.h).
LM_API int lm_tile_ground(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H,
                          int W, int cell_px, void* workspace, long workspace_bytes, float* ground, float* ground_min, float* cell_min) {
    LM_NO_CAPTURE(hip_stream, "tile_ground", LM_WHY_HOST_COPY);
    static thread_local std::vector<GroundTile> h_tiles;
    long n_wg, n_blocks, N;
    if (int e = derive_tiles("tile_ground", tile_offsets, params, B, H, W, cell_px, GCHUNK, h_tiles, &n_wg, &n_blocks, &N)) return e;
    LM_REQUIRE(workspace && ground && ground_min, "tile_ground: null pointer (workspace / ground / ground_min)");
    if (int e = lm_tile_points_check("tile_ground", points_xyzi, N, workspace)) return e;
    LM_REQUIRE(lm_tile_ground_workspace_bytes(B, H, W, cell_px) <= workspace_bytes, "tile_ground: workspace too small (%ld B needed)",
               lm_tile_ground_workspace_bytes(B, H, W, cell_px));
    const int Gy = (int)lm_cdivl(H, cell_px), Gx = (int)lm_cdivl(W, cell_px), ncell = Gy * Gx;
    hipStream_t s = (hipStream_t)hip_stream;
    char* w = (char*)workspace;
    GroundTile* d_tiles = (GroundTile*)w;
    w += lm_align256((size_t)B * sizeof(GroundTile));
    unsigned* keys = (unsigned*)w;
    LM_HIP(hipMemsetAsync(keys, 0xFF, (size_t)B * ncell * 4, s));
    if (n_wg > 0) {
        LM_HIP(hipMemcpyAsync(d_tiles, h_tiles.data(), (size_t)B * sizeof(GroundTile), hipMemcpyHostToDevice, s));
        const size_t lds = (size_t)ncell * sizeof(unsigned);
        if (int e = lm_ensure_dynamic_lds((const void*)ground_min_kernel, lds)) return e;
        hipLaunchKernelGGL(ground_min_kernel, dim3((unsigned)n_wg), dim3(GT), lds, s, reinterpret_cast<const f32x4*>(points_xyzi), d_tiles, B,
                           keys, H, W, lm_fastdiv_make((unsigned)cell_px), Gx, ncell);
        LM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ground_smooth_kernel, dim3((unsigned)B), dim3(GT), 0, s, keys, ground, ground_min, cell_min, Gy, Gx);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

LM_API long lm_ground_select_workspace_bytes(long N, int B) {
    if (N < 0 || N > 2147483647L || B < 1 || B > LM_MAX_TILES) return 0;
    const long L = N / SEL_BLOCK + B + 1;                       // at most this many blocks + the terminating entry
    return (long)(lm_align256((size_t)B * sizeof(GroundTile)) + lm_align256((size_t)L * 4) + lm_align256(lm_prim_scan_temp_bytes(L)));
}

// ground: device [B][Gy][Gx] (lm_tile_ground's, same H, W, cell_px); points_out: device [tile_offsets[B] - tile_offsets[0]][4];
// out_offsets: device [B+1] int64; out_offsets_host: HOST [B+1] or NULL (not NULL: one synchronisation of the stream).
LM_API int lm_ground_select(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H,
                            int W, int cell_px, const float* ground, float h_lo, float h_hi, void* workspace, long workspace_bytes,
                            float* points_out, long* out_offsets, long* out_offsets_host) {
    LM_NO_CAPTURE(hip_stream, "ground_select", LM_WHY_HOST_COPY_SYNC);
    static thread_local std::vector<GroundTile> h_tiles;
    long n_wg, n_blocks, N;
    if (int e = derive_tiles("ground_select", tile_offsets, params, B, H, W, cell_px, SEL_CHUNK, h_tiles, &n_wg, &n_blocks, &N)) return e;
    LM_REQUIRE(h_lo == h_lo, "ground_select: h_lo must not be NaN");
    LM_REQUIRE(h_hi == h_hi, "ground_select: h_hi must not be NaN");
    LM_REQUIRE(h_lo <= h_hi, "ground_select: h_lo=%g > h_hi=%g: the range is empty", (double)h_lo, (double)h_hi);
    LM_REQUIRE(workspace && ground && out_offsets, "ground_select: null pointer (workspace / ground / out_offsets)");
    LM_REQUIRE((points_xyzi && points_out) || N == 0, "ground_select: null points / points_out");
    LM_REQUIRE(((uintptr_t)points_xyzi & 15) == 0 && ((uintptr_t)points_out & 15) == 0 && ((uintptr_t)workspace & 15) == 0 &&
                   ((uintptr_t)out_offsets & 7) == 0,
               "ground_select: points, points_out and workspace must be 16-byte aligned, out_offsets 8-byte");
    LM_REQUIRE(lm_ground_select_workspace_bytes(N, B) <= workspace_bytes, "ground_select: workspace too small (%ld B needed)",
               lm_ground_select_workspace_bytes(N, B));
    const int Gx = (int)lm_cdivl(W, cell_px), ncell = (int)lm_cdivl(H, cell_px) * Gx;
    const long L = n_blocks + 1;                                // <= N / 256 + B + 1
    hipStream_t s = (hipStream_t)hip_stream;
    char* w = (char*)workspace;
    GroundTile* d_tiles = (GroundTile*)w;
    w += lm_align256((size_t)B * sizeof(GroundTile));
    unsigned* counts = (unsigned*)w;
    w += lm_align256((size_t)(N / SEL_BLOCK + B + 1) * 4);
    void* scan_tmp = w;
    const size_t scan_bytes = lm_align256(lm_prim_scan_temp_bytes(N / SEL_BLOCK + B + 1));
    const LmFastDiv cdiv = lm_fastdiv_make((unsigned)cell_px);
    const f32x4* pts = reinterpret_cast<const f32x4*>(points_xyzi);
    LM_HIP(hipMemcpyAsync(d_tiles, h_tiles.data(), (size_t)B * sizeof(GroundTile), hipMemcpyHostToDevice, s));
    LM_HIP(hipMemsetAsync(counts + n_blocks, 0, sizeof(unsigned), s));           // the scan turns it into the total
    if (n_wg > 0) {
        hipLaunchKernelGGL(ground_select_kernel<false>, dim3((unsigned)n_wg), dim3(GT), 0, s, pts, d_tiles, B, ground, H, W, cdiv, Gx, ncell,
                           h_lo, h_hi, counts, (f32x4*)nullptr);
        LM_LAUNCH_CHECK();
    }
    if (int e = lm_prim_exclusive_scan_u32(s, counts, counts, L, scan_tmp, scan_bytes)) return e;
    if (n_wg > 0) {
        hipLaunchKernelGGL(ground_select_kernel<true>, dim3((unsigned)n_wg), dim3(GT), 0, s, pts, d_tiles, B, ground, H, W, cdiv, Gx, ncell,
                           h_lo, h_hi, counts, reinterpret_cast<f32x4*>(points_out));
        LM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ground_offsets_kernel, dim3((unsigned)(B / GT + 1)), dim3(GT), 0, s, counts, d_tiles, B, n_blocks, out_offsets);
    LM_LAUNCH_CHECK();
    if (out_offsets_host) {
        LM_HIP(hipMemcpyAsync(out_offsets_host, out_offsets, (size_t)(B + 1) * sizeof(long), hipMemcpyDeviceToHost, s));
        LM_HIP(hipStreamSynchronize(s));
    }
    return LM_OK;
}
