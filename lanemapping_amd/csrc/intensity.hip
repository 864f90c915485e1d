// Intensity window of the LAS routes: two order statistics (percentiles) of the intensities of the points a tile, or a group of tiles,
// keeps, out of the points already binned for the rasteriser.  Input is the (points, tile_offsets, params) triple lm_bev_raster_batch
// takes, walked with the scaffold of tile_points.h (tile constants, workgroup -> tile, streaming loop, host prologue).  A point counts
// for tile b exactly when raster.hip would keep it for b and its intensity is not NaN.
//
// Key of a point: k = (int)floorf(fminf(fmaxf(i, 0), 65535)), 0 .. 65535 (LAS intensities are u16: the key is the intensity).  With n
// counted points in group g, window[g][0] is the key of 0-based rank (n - 1) q_lo_ppm / 1,000,000 (64-bit floor division) in ascending
// order, window[g][1] the same with q_hi_ppm: lower order statistics, values that occur in the data.  n = 0: (-1, -1).
//
// Exact in two levels of 4096 x 16 keys, all counters integers added with integer atomics (order independent: the same bits on every run):
//   (a) coarse   a workgroup streams a span of ICPW chunks of ICHUNK = 16,384 points of one tile (lm_stream_points: 256 lanes x 64 loads
//                per chunk, 8 in flight per lane), counts k >> 4 in 4096 LDS counters and flushes its non-zero counters to
//                hist[group][4096].
//   (b) locate   one workgroup per group: n, the two ranks, the coarse bin each rank falls into and the rank left inside that bin.
//   (c) fine     the same stream again; a point whose k >> 4 is one of its group's two located bins counts k & 15 in 2 x 16 LDS
//                counters, flushed to fine[group][2][16].  The predicate and the bytes are those of (a), so the 16 counters of a located
//                bin sum to its coarse count and the rank left inside the bin always falls on one of them.
//   (d) resolve  one thread per group walks the 16 counters: window, count.
// Same-address LDS atomics: a saturated scanner puts a large share of a wave's 64 points on one key.  wave_count() first lets the
// lowest active lane add the number of lanes that share its counter (two such rounds), only the rest add one each.
// HBM traffic: 16 N read in (a) and in (c).  No host synchronisation, no scratch.
#include "common.h"
#include "tile_points.h"

#include <cmath>
#include <vector>

namespace {

constexpr int IT = 256;                      // threads per workgroup, every kernel of this file
constexpr int I_PER_THREAD = 64;
constexpr int ICHUNK = IT * I_PER_THREAD;    // points per chunk
constexpr int ICPW = 4;                      // chunks per workgroup: one flush of up to 4096 counters per 65,536 points
constexpr long ISPAN = (long)ICHUNK * ICPW;
constexpr int LB = 8;                        // loads in flight per lane
constexpr int NBIN = 4096;                   // coarse bins of 16 keys
constexpr unsigned NO_BIN = 0xFFFFFFFFu;     // no key has this coarse bin

struct IntenTile : LmTileRange {
    int group, pad;
};
static_assert(sizeof(IntenTile) == 96 && alignof(IntenTile) == 16, "96 bytes per tile: lm_tile_intensity_workspace_bytes");

struct Located {                             // per group, written by (b)
    unsigned bin[2];                         // coarse bin of the lower / upper rank, NO_BIN for an empty group
    unsigned rem[2];                         // rank inside that bin
};

// window test + intensity not NaN -> the key
__device__ __forceinline__ bool point_key(const f32x4 p, const IntenTile& X, int H, int W, int& key) {
    int row, col;
    float vz;
    if (!lm_point_window(p, X, H, W, row, col, vz)) return false;
    if (!(p[3] == p[3])) return false;
    key = (int)floorf(fminf(fmaxf(p[3], 0.0f), 65535.0f));
    return true;
}

// counter[idx] += 1 for every lane with `on`; called by all 64 lanes of a wave together (wave-uniform control flow)
__device__ __forceinline__ void wave_count(unsigned* counter, int idx, bool on) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long m = __ballot(on);
        if (m == 0) return;                                     // wave-uniform
        const int leader = __ffsll((long long)m) - 1;
        const int lidx = __builtin_amdgcn_readlane(idx, leader);
        const unsigned long long same = __ballot(on && idx == lidx);
        if (lane == leader) atomicAdd(&counter[lidx], (unsigned)__popcll(same));
        on = on && idx != lidx;
    }
    if (on) atomicAdd(&counter[idx], 1u);
}

// (a) and (c), grid: sum over tiles of ceil(count / ISPAN).  FINE = false: hist[group][NBIN]; FINE = true: fine[group][2][16]
template <bool FINE>
__global__ __launch_bounds__(IT) void inten_count_kernel(const f32x4* __restrict__ pts, const IntenTile* __restrict__ tiles, int B,
                                                         const Located* __restrict__ loc, unsigned* __restrict__ out, int H, int W) {
    __shared__ unsigned cnt[FINE ? 32 : NBIN];
    constexpr int NC = FINE ? 32 : NBIN;
    const int tid = threadIdx.x;
    const int t = lm_tile_of(tiles, B, (long)blockIdx.x);
    const IntenTile X = tiles[t];
    const long first = ((long)blockIdx.x - X.cbase) * ISPAN;
    const long rest = X.count - first;                          // >= 1
    const long left = rest < ISPAN ? rest : ISPAN;
    unsigned bin_lo = NO_BIN, bin_hi = NO_BIN;
    if (FINE) {
        bin_lo = loc[X.group].bin[0];
        bin_hi = loc[X.group].bin[1];
    }
    for (int i = tid; i < NC; i += IT) cnt[i] = 0;
    __syncthreads();
    lm_stream_points<IT, I_PER_THREAD * ICPW, LB>(pts + X.start + first, left, tid, [&](const f32x4 p, bool valid) {
        int key = 0;
        const bool on = valid && point_key(p, X, H, W, key);   // (no early return: wave_count is wave-collective)
        const unsigned bin = (unsigned)key >> 4;
        if (!FINE) {
            wave_count(cnt, (int)bin, on);
        } else {
            wave_count(cnt, key & 15, on && bin == bin_lo);
            wave_count(cnt + 16, key & 15, on && bin == bin_hi);
        }
    });
    __syncthreads();
    unsigned* dst = out + (long)X.group * NC;
    for (int i = tid; i < NC; i += IT) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(dst + i, c);
    }
}

// (b) grid: G workgroups.  A thread owns 16 consecutive coarse bins.
__global__ __launch_bounds__(IT) void inten_locate_kernel(const unsigned* __restrict__ hist, Located* __restrict__ loc, long* __restrict__ count,
                                                          int q_lo_ppm, int q_hi_ppm) {
    __shared__ unsigned long long part[IT];
    const int tid = threadIdx.x, g = blockIdx.x;
    const unsigned* h = hist + (long)g * NBIN + tid * (NBIN / IT);
    unsigned c[NBIN / IT];
    unsigned long long mine = 0;
#pragma unroll
    for (int e = 0; e < NBIN / IT; ++e) {
        c[e] = h[e];
        mine += c[e];
    }
    part[tid] = mine;
    __syncthreads();
    unsigned long long before = 0, n = 0;
    for (int i = 0; i < IT; ++i) {
        const unsigned long long v = part[i];
        before += i < tid ? v : 0;
        n += v;
    }
    if (tid == 0) {
        count[g] = (long)n;
        if (n == 0) loc[g].bin[0] = loc[g].bin[1] = NO_BIN, loc[g].rem[0] = loc[g].rem[1] = 0;
    }
    if (n == 0) return;
    const unsigned long long rank[2] = {(n - 1) * (unsigned long long)q_lo_ppm / 1000000ull, (n - 1) * (unsigned long long)q_hi_ppm / 1000000ull};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (rank[s] < before || rank[s] >= before + mine) continue;      // exactly one thread holds each rank
        unsigned long long r = rank[s] - before;
#pragma unroll
        for (int e = 0; e < NBIN / IT; ++e) {
            if (r < c[e]) {
                loc[g].bin[s] = (unsigned)(tid * (NBIN / IT) + e);
                loc[g].rem[s] = (unsigned)r;
                break;
            }
            r -= c[e];
        }
    }
}

// (d) grid: ceil(G / IT) workgroups, one thread per group
__global__ __launch_bounds__(IT) void inten_resolve_kernel(const unsigned* __restrict__ fine, const Located* __restrict__ loc, int G,
                                                           int* __restrict__ window) {
    const int g = blockIdx.x * IT + threadIdx.x;
    if (g >= G) return;
    const Located L = loc[g];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        int key = -1;
        if (L.bin[s] != NO_BIN) {
            const unsigned* f = fine + ((long)g * 2 + s) * 16;
            unsigned r = L.rem[s];
            key = (int)(L.bin[s] * 16 + 15);                    // (the 16 counters sum to the bin's coarse count > rem)
            for (int e = 0; e < 16; ++e) {
                const unsigned c = f[e];
                if (r < c) {
                    key = (int)(L.bin[s] * 16 + e);
                    break;
                }
                r -= c;
            }
        }
        window[g * 2 + s] = key;
    }
}

}  // namespace

LM_API long lm_tile_intensity_workspace_bytes(int B, int G) {
    if (B < 1 || B > LM_MAX_TILES || G < 1 || G > B) return 0;
    return (long)(lm_align256((size_t)B * sizeof(IntenTile)) + lm_align256((size_t)G * NBIN * 4) + lm_align256((size_t)G * sizeof(Located)) +
                  lm_align256((size_t)G * 32 * 4));
}

// points: device [sum N][4]; tile_offsets: HOST [B+1]; params: HOST [B]; group: HOST [B] or NULL; window [G][2] int32, count [G] int64,
// coarse_hist [G][4096] u32 or NULL: device.  Asynchronous, but copies host memory of this call to the device: refuses a capturing
// stream (common.h).
LM_API int lm_tile_intensity_window(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B,
                                    int H, int W, const int* group, int G, int q_lo_ppm, int q_hi_ppm, void* workspace,
                                    long workspace_bytes, int* window, long* count, unsigned* coarse_hist) {
    LM_NO_CAPTURE(hip_stream, "tile_intensity_window", LM_WHY_HOST_COPY);
    static thread_local std::vector<IntenTile> h_tiles;
    LM_REQUIRE(B >= 1 && B <= LM_MAX_TILES, "tile_intensity_window: B=%d tiles, 1 to %d are supported", B, LM_MAX_TILES);   // G is judged against it
    LM_REQUIRE(G >= 1 && G <= B, "tile_intensity_window: G=%d groups, 1 to B=%d are supported", G, B);
    LM_REQUIRE(group || G == B, "tile_intensity_window: group is null (tile b is group b), so G=%d must equal B=%d", G, B);
    LM_REQUIRE(workspace && window && count, "tile_intensity_window: null pointer (workspace / window / count)");
    LM_REQUIRE(q_lo_ppm >= 0 && q_lo_ppm <= 1000000, "tile_intensity_window: q_lo_ppm=%d is outside 0..1000000", q_lo_ppm);
    LM_REQUIRE(q_hi_ppm >= 0 && q_hi_ppm <= 1000000, "tile_intensity_window: q_hi_ppm=%d is outside 0..1000000", q_hi_ppm);
    LM_REQUIRE(q_lo_ppm <= q_hi_ppm, "tile_intensity_window: q_lo_ppm=%d > q_hi_ppm=%d", q_lo_ppm, q_hi_ppm);
    long n_wg, N;
    const auto tile_group = [&](int b, IntenTile& T, long&) -> int {
        const int g = group ? group[b] : b;
        LM_REQUIRE(g >= 0 && g < G, "tile_intensity_window: group[%d]=%d is outside 0..G-1=%d", b, g, G - 1);
        T.group = g, T.pad = 0;
        return LM_OK;
    };
    if (int e = lm_tile_ranges("tile_intensity_window", tile_offsets, params, B, 1, H, W, ISPAN, h_tiles, &n_wg, &N, tile_group)) return e;
    LM_REQUIRE(N < 4294967296L, "tile_intensity_window: tile_offsets span %ld points, fewer than 2^32 are supported (32-bit counters)", N);
    if (int e = lm_tile_points_check("tile_intensity_window", points_xyzi, N, workspace)) return e;
    LM_REQUIRE(((uintptr_t)window & 3) == 0 && ((uintptr_t)count & 7) == 0 && ((uintptr_t)coarse_hist & 3) == 0,
               "tile_intensity_window: window and coarse_hist must be 4-byte aligned, count 8-byte");
    LM_REQUIRE(lm_tile_intensity_workspace_bytes(B, G) <= workspace_bytes, "tile_intensity_window: workspace too small (%ld B needed)",
               lm_tile_intensity_workspace_bytes(B, G));
    hipStream_t s = (hipStream_t)hip_stream;
    char* w = (char*)workspace;
    IntenTile* d_tiles = (IntenTile*)w;
    w += lm_align256((size_t)B * sizeof(IntenTile));
    unsigned* hist = coarse_hist ? coarse_hist : (unsigned*)w;  // the caller's histogram is the one the passes count into
    w += lm_align256((size_t)G * NBIN * 4);
    Located* loc = (Located*)w;
    w += lm_align256((size_t)G * sizeof(Located));
    unsigned* fine = (unsigned*)w;
    const f32x4* pts = reinterpret_cast<const f32x4*>(points_xyzi);
    LM_HIP(hipMemsetAsync(hist, 0, (size_t)G * NBIN * 4, s));
    LM_HIP(hipMemsetAsync(fine, 0, (size_t)G * 32 * 4, s));
    if (n_wg > 0) {
        LM_HIP(hipMemcpyAsync(d_tiles, h_tiles.data(), (size_t)B * sizeof(IntenTile), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(inten_count_kernel<false>, dim3((unsigned)n_wg), dim3(IT), 0, s, pts, d_tiles, B, (const Located*)nullptr, hist, H, W);
        LM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(inten_locate_kernel, dim3((unsigned)G), dim3(IT), 0, s, hist, loc, count, q_lo_ppm, q_hi_ppm);
    LM_LAUNCH_CHECK();
    if (n_wg > 0) {
        hipLaunchKernelGGL(inten_count_kernel<true>, dim3((unsigned)n_wg), dim3(IT), 0, s, pts, d_tiles, B, loc, fine, H, W);
        LM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(inten_resolve_kernel, dim3((unsigned)((G + IT - 1) / IT)), dim3(IT), 0, s, fine, loc, G, window);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// ---- Intensity balance: a local asphalt level per ground cell, and a gain field applied to the binned points (the rule: include/lanemap_hip.h).
// The cell grid is ground.hip's: Gy = ceil(H / cell_px) by Gx = ceil(W / cell_px), the cell of a point is (row / cell_px, col / cell_px).
// lm_tile_intensity_cells: the order statistic of rank (n - 1) q_ppm / 1,000,000 of every cell's keys, exact in two levels of 256 x 256
// keys.  There are B Gy Gx rows of 256 counters - far more than LDS holds - so the counters live in the workspace and are added to with
// integer global atomics (order independent: the same bits on every run), the lanes of a wave that hit one counter merged first
// (wave_count above: consecutive returns of a scan line fall into one cell at one brightness).
//   (a) coarse   the stream of inten_count_kernel; counts k >> 8 in hist[tile][cell][256]
//   (b) locate   one wave per cell, 4 counters per lane, the prefix sum over the lanes: n, the coarse bin that holds the rank and the rank
//                left inside it; zeroes the cell's 256 counters for (c)
//   (c) fine     the same stream; a point whose k >> 8 is its cell's located bin counts k & 255 in the same row
//   (d) resolve  one wave per cell: level.  Then one thread per cell: model, the lower median of the known levels of the 3 x 3 cells
// lm_tile_intensity_apply: one streaming pass, 16 bytes in and 16 bytes out per point; the four gains of a point come from L2.
// HBM traffic: 16 N read in (a) and in (c), 32 N in the apply.  None of these kernels uses LDS.
namespace {

constexpr int CB = 256;                      // keys per coarse bin = fine counters per bin
constexpr int BAL_MIN_CELL_PX = 16, BAL_MAX_CELL_PX = 128;
constexpr int BAL_MAX_CELLS = 32768;         // cells per tile: 32 MiB of counters
constexpr int CELLS_PER_WG = IT / 64;        // (b), (d): one wave per cell

struct CellLoc {                             // per cell, written by (b)
    unsigned bin, rem;                       // NO_BIN for an empty cell
};

// window test + intensity not NaN -> the point's pixel and key
__device__ __forceinline__ bool point_pixel_key(const f32x4 p, const IntenTile& X, int H, int W, int& row, int& col, int& key) {
    float vz;
    if (!lm_point_window(p, X, H, W, row, col, vz)) return false;
    if (!(p[3] == p[3])) return false;
    key = (int)floorf(fminf(fmaxf(p[3], 0.0f), 65535.0f));
    return true;
}

// (a) and (c), grid: sum over tiles of ceil(count / ISPAN).  hist [B][ncell][256]; FINE: loc [B][ncell]
template <bool FINE>
__global__ __launch_bounds__(IT) void cells_count_kernel(const f32x4* __restrict__ pts, const IntenTile* __restrict__ tiles, int B,
                                                         const CellLoc* __restrict__ loc, unsigned* __restrict__ hist, int H, int W,
                                                         LmFastDiv cdiv, int Gx, int ncell) {
    const int tid = threadIdx.x;
    const int t = lm_tile_of(tiles, B, (long)blockIdx.x);
    const IntenTile X = tiles[t];
    const long first = ((long)blockIdx.x - X.cbase) * ISPAN;
    const long rest = X.count - first;                          // >= 1
    const long left = rest < ISPAN ? rest : ISPAN;
    unsigned* dst = hist + (long)t * ncell * CB;
    const CellLoc* L = loc + (long)t * ncell;
    lm_stream_points<IT, I_PER_THREAD * ICPW, LB>(pts + X.start + first, left, tid, [&](const f32x4 p, bool valid) {
        int row = 0, col = 0, key = 0;
        bool on = valid && point_pixel_key(p, X, H, W, row, col, key);   // (no early return: wave_count is wave-collective)
        const int cell = on ? (int)lm_fastdiv((unsigned)row, cdiv) * Gx + (int)lm_fastdiv((unsigned)col, cdiv) : 0;   // < ncell
        if (FINE) on = on && L[cell].bin == (unsigned)key >> 8;
        wave_count(dst, cell * CB + (FINE ? key & (CB - 1) : key >> 8), on);
    });
}

// inclusive prefix sum of v over the 64 lanes of a wave
__device__ __forceinline__ unsigned wave_inclusive(unsigned v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// The 256 counters of a row lie over the lanes of a wave, 4 consecutive ones per lane.  n = their sum; for rank < n exactly one lane
// returns true, with the counter that holds the rank and the rank left inside it.
__device__ __forceinline__ bool wave_find(const uint4 v, int lane, unsigned inc, unsigned rank, unsigned& idx, unsigned& rem) {
    const unsigned c[4] = {v.x, v.y, v.z, v.w};
    const unsigned mine = v.x + v.y + v.z + v.w, before = inc - mine;
    if (rank < before || rank >= inc) return false;
    unsigned r = rank - before;
    idx = (unsigned)lane * 4 + 3, rem = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (r < c[e]) {
            idx = (unsigned)lane * 4 + e, rem = r;
            break;
        }
        r -= c[e];
    }
    return true;
}

// (b) grid: ceil(cells / 4) workgroups, cells = B ncell
__global__ __launch_bounds__(IT) void cells_locate_kernel(unsigned* __restrict__ hist, CellLoc* __restrict__ loc, int* __restrict__ count,
                                                          long cells, int q_ppm) {
    const int lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * CELLS_PER_WG + (threadIdx.x >> 6);
    if (c >= cells) return;                                     // wave-uniform
    uint4* row = reinterpret_cast<uint4*>(hist + c * CB) + lane;
    const uint4 v = *row;
    const unsigned inc = wave_inclusive(v.x + v.y + v.z + v.w, lane);
    const unsigned n = __shfl(inc, 63);                         // < 2^31: the entry bounds the points
    *row = make_uint4(0u, 0u, 0u, 0u);
    if (lane == 0) {
        count[c] = (int)n;
        if (n == 0) loc[c].bin = NO_BIN, loc[c].rem = 0;
    }
    if (n == 0) return;
    const unsigned rank = (unsigned)((unsigned long long)(n - 1) * (unsigned long long)q_ppm / 1000000ull);
    unsigned idx, rem;
    if (wave_find(v, lane, inc, rank, idx, rem)) loc[c].bin = idx, loc[c].rem = rem;
}

// (d) grid: as (b).  The 256 fine counters of a cell sum to the count of its located bin > rem.
__global__ __launch_bounds__(IT) void cells_level_kernel(const unsigned* __restrict__ fine, const CellLoc* __restrict__ loc,
                                                         int* __restrict__ level, long cells) {
    const int lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * CELLS_PER_WG + (threadIdx.x >> 6);
    if (c >= cells) return;                                     // wave-uniform
    const CellLoc L = loc[c];
    if (L.bin == NO_BIN) {
        if (lane == 0) level[c] = -1;
        return;
    }
    const uint4 v = *(reinterpret_cast<const uint4*>(fine + c * CB) + lane);
    const unsigned inc = wave_inclusive(v.x + v.y + v.z + v.w, lane);
    unsigned idx, rem;
    if (wave_find(v, lane, inc, L.rem, idx, rem)) level[c] = (int)(L.bin * CB + idx);
}

// model: grid ceil(cells / IT), one thread per cell: ground_smooth_kernel's rule on the levels of the known cells
__global__ __launch_bounds__(IT) void cells_model_kernel(const int* __restrict__ level, const int* __restrict__ count, int* __restrict__ model,
                                                         long cells, int Gy, int Gx, int min_points) {
    const long c = (long)blockIdx.x * IT + threadIdx.x;
    if (c >= cells) return;
    const int ncell = Gy * Gx;
    const long tile0 = c / ncell * ncell;
    const int in = (int)(c - tile0), cy = in / Gx, cx = in - cy * Gx;
    int v[9];
    bool known[9];
    int n = 0;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        const int y = cy + e / 3 - 1, x = cx + e % 3 - 1;
        const bool inside = y >= 0 && y < Gy && x >= 0 && x < Gx;
        known[e] = inside && count[tile0 + y * Gx + x] >= min_points;
        v[e] = known[e] ? level[tile0 + y * Gx + x] : 0;
        n += known[e];
    }
    // the element of rank (n - 1) / 2 among the known; equal levels are ranked by their position, so exactly one element has each rank
    const int want = (n - 1) / 2;
    int res = -1;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        int rank = 0;
#pragma unroll
        for (int f = 0; f < 9; ++f) rank += known[f] && (v[f] < v[e] || (f < e && v[f] == v[e]));
        if (known[e] && rank == want) res = v[e];
    }
    model[c] = res;
}

// position of a pixel between the cell centres of one axis: the two cells and the weight of the second
__device__ __forceinline__ float cell_axis(int px, int cell_px, int G, int& i0, int& i1) {
    float u = __fdiv_rn((float)(2 * px + 1 - cell_px), (float)(2 * cell_px));
    u = fminf(fmaxf(u, 0.0f), (float)(G - 1));
    const float fl = floorf(u);
    i0 = (int)fl;
    i1 = i0 + 1 < G ? i0 + 1 : G - 1;
    return __fsub_rn(u, fl);
}

// grid: sum over tiles of ceil(count / ISPAN).  out may be pts: a lane stores the point it loaded, and a lane past the end, which
// loaded the span's last point a second time, stores nothing.
__global__ __launch_bounds__(IT) void balance_apply_kernel(const f32x4* pts, const IntenTile* __restrict__ tiles, int B,
                                                           const float* __restrict__ gains, f32x4* out, int H, int W, int cell_px, int Gy,
                                                           int Gx) {
    const int tid = threadIdx.x;
    const int t = lm_tile_of(tiles, B, (long)blockIdx.x);
    const IntenTile X = tiles[t];
    const long first = ((long)blockIdx.x - X.cbase) * ISPAN;
    const long rest = X.count - first;                          // >= 1
    const long left = rest < ISPAN ? rest : ISPAN;
    const float* g = gains + (long)t * Gy * Gx;
    f32x4* dst = out + X.start + first;
    long at = tid;                                              // lm_stream_points hands lane tid the points tid, tid + IT, ... in order
    lm_stream_points<IT, I_PER_THREAD * ICPW, LB>(pts + X.start + first, left, tid, [&](f32x4 p, bool valid) {
        const long i = at;
        at += IT;
        if (!valid) return;
        int row, col, key;
        if (point_pixel_key(p, X, H, W, row, col, key)) {
            int x0, x1, y0, y1;
            const float fx = cell_axis(col, cell_px, Gx, x0, x1), fy = cell_axis(row, cell_px, Gy, y0, y1);
            const float ux = __fsub_rn(1.0f, fx), uy = __fsub_rn(1.0f, fy);
            const float top = __fadd_rn(__fmul_rn(g[y0 * Gx + x0], ux), __fmul_rn(g[y0 * Gx + x1], fx));
            const float bot = __fadd_rn(__fmul_rn(g[y1 * Gx + x0], ux), __fmul_rn(g[y1 * Gx + x1], fx));
            const float gain = __fadd_rn(__fmul_rn(top, uy), __fmul_rn(bot, fy));
            p[3] = fminf(__fmul_rn(p[3], gain), 65535.0f);
        }
        __builtin_nontemporal_store(p, dst + i);
    });
}

// the checks both entries share, and the tile table
static int balance_tiles(const char* who, const long* tile_offsets, const LmRasterParams* params, int B, int H, int W, int cell_px,
                         std::vector<IntenTile>& out, long* n_wg, long* N) {
    LM_REQUIRE(B >= 1 && B <= LM_MAX_TILES, "%s: B=%d tiles, 1 to %d are supported", who, B, LM_MAX_TILES);
    LM_REQUIRE(cell_px >= BAL_MIN_CELL_PX && cell_px <= BAL_MAX_CELL_PX, "%s: cell_px=%d, %d to %d are supported", who, cell_px,
               BAL_MIN_CELL_PX, BAL_MAX_CELL_PX);
    LM_REQUIRE(H > 0 && W > 0, "%s: bad tile size H=%d W=%d", who, H, W);
    LM_REQUIRE(lm_cdivl(H, cell_px) * lm_cdivl(W, cell_px) <= BAL_MAX_CELLS, "%s: cell_px=%d gives %ld cells per tile, at most %d are supported",
               who, cell_px, lm_cdivl(H, cell_px) * lm_cdivl(W, cell_px), BAL_MAX_CELLS);
    const auto no_group = [](int, IntenTile& T, long&) -> int {
        T.group = 0, T.pad = 0;
        return LM_OK;
    };
    if (int e = lm_tile_ranges(who, tile_offsets, params, B, 1, H, W, ISPAN, out, n_wg, N, no_group)) return e;
    LM_REQUIRE(*N <= 2147483647L, "%s: tile_offsets span %ld points, at most 2^31 - 1 are supported (32-bit counts)", who, *N);
    return LM_OK;
}

}  // namespace

LM_API long lm_tile_intensity_cells_workspace_bytes(int B, int H, int W, int cell_px) {
    if (B < 1 || B > LM_MAX_TILES || H <= 0 || W <= 0 || cell_px < BAL_MIN_CELL_PX || cell_px > BAL_MAX_CELL_PX) return 0;
    const long ncell = lm_cdivl(H, cell_px) * lm_cdivl(W, cell_px);
    if (ncell > BAL_MAX_CELLS) return 0;
    return (long)(lm_align256((size_t)B * sizeof(IntenTile)) + lm_align256((size_t)B * ncell * CB * 4) +
                  lm_align256((size_t)B * ncell * sizeof(CellLoc)));
}

// points: device [sum N][4]; tile_offsets: HOST [B+1]; params: HOST [B]; level, count, model: device [B][Gy][Gx] int32.  Asynchronous, but
// copies host memory of this call to the device: refuses a capturing stream (common.h).
LM_API int lm_tile_intensity_cells(const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H, int W,
                                   int cell_px, int q_ppm, int min_points, void* workspace, long workspace_bytes, int* level, int* count,
                                   int* model, void* hip_stream) {
    LM_NO_CAPTURE(hip_stream, "tile_intensity_cells", LM_WHY_HOST_COPY);
    static thread_local std::vector<IntenTile> h_tiles;
    if (B == 0) return LM_OK;
    long n_wg, N;
    if (int e = balance_tiles("tile_intensity_cells", tile_offsets, params, B, H, W, cell_px, h_tiles, &n_wg, &N)) return e;
    LM_REQUIRE(q_ppm >= 0 && q_ppm <= 1000000, "tile_intensity_cells: q_ppm=%d is outside 0..1000000", q_ppm);
    LM_REQUIRE(min_points >= 0, "tile_intensity_cells: min_points=%d is negative", min_points);
    LM_REQUIRE(workspace && level && count && model, "tile_intensity_cells: null pointer (workspace / level / count / model)");
    if (int e = lm_tile_points_check("tile_intensity_cells", points_xyzi, N, workspace)) return e;
    LM_REQUIRE(((uintptr_t)level & 3) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)model & 3) == 0,
               "tile_intensity_cells: level, count and model must be 4-byte aligned");
    LM_REQUIRE(lm_tile_intensity_cells_workspace_bytes(B, H, W, cell_px) <= workspace_bytes,
               "tile_intensity_cells: workspace too small (%ld B needed)", lm_tile_intensity_cells_workspace_bytes(B, H, W, cell_px));
    const int Gy = (int)lm_cdivl(H, cell_px), Gx = (int)lm_cdivl(W, cell_px), ncell = Gy * Gx;
    const long cells = (long)B * ncell;
    hipStream_t s = (hipStream_t)hip_stream;
    char* w = (char*)workspace;
    IntenTile* d_tiles = (IntenTile*)w;
    w += lm_align256((size_t)B * sizeof(IntenTile));
    unsigned* hist = (unsigned*)w;
    w += lm_align256((size_t)cells * CB * 4);
    CellLoc* loc = (CellLoc*)w;
    const f32x4* pts = reinterpret_cast<const f32x4*>(points_xyzi);
    const LmFastDiv cdiv = lm_fastdiv_make((unsigned)cell_px);
    const dim3 per_wave((unsigned)lm_cdivl(cells, CELLS_PER_WG));
    LM_HIP(hipMemsetAsync(hist, 0, (size_t)cells * CB * 4, s));
    if (n_wg > 0) {
        LM_HIP(hipMemcpyAsync(d_tiles, h_tiles.data(), (size_t)B * sizeof(IntenTile), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(cells_count_kernel<false>, dim3((unsigned)n_wg), dim3(IT), 0, s, pts, d_tiles, B, (const CellLoc*)nullptr, hist, H, W,
                           cdiv, Gx, ncell);
        LM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cells_locate_kernel, per_wave, dim3(IT), 0, s, hist, loc, count, cells, q_ppm);
    LM_LAUNCH_CHECK();
    if (n_wg > 0) {
        hipLaunchKernelGGL(cells_count_kernel<true>, dim3((unsigned)n_wg), dim3(IT), 0, s, pts, d_tiles, B, loc, hist, H, W, cdiv, Gx, ncell);
        LM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cells_level_kernel, per_wave, dim3(IT), 0, s, hist, loc, level, cells);
    LM_LAUNCH_CHECK();
    hipLaunchKernelGGL(cells_model_kernel, dim3((unsigned)lm_cdivl(cells, IT)), dim3(IT), 0, s, level, count, model, cells, Gy, Gx, min_points);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

LM_API long lm_tile_intensity_apply_workspace_bytes(int B) {
    if (B < 1 || B > LM_MAX_TILES) return 0;
    return (long)lm_align256((size_t)B * sizeof(IntenTile));
}

// gains: device [B][Gy][Gx] f32; out: device [sum N][4], may be points_xyzi itself (any other overlap is the caller's error).
// Asynchronous, but copies host memory of this call to the device: refuses a capturing stream (common.h).
LM_API int lm_tile_intensity_apply(const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H, int W,
                                   int cell_px, const float* gains, void* workspace, long workspace_bytes, float* out, void* hip_stream) {
    LM_NO_CAPTURE(hip_stream, "tile_intensity_apply", LM_WHY_HOST_COPY);
    static thread_local std::vector<IntenTile> h_tiles;
    if (B == 0) return LM_OK;
    long n_wg, N;
    if (int e = balance_tiles("tile_intensity_apply", tile_offsets, params, B, H, W, cell_px, h_tiles, &n_wg, &N)) return e;
    LM_REQUIRE(workspace && gains, "tile_intensity_apply: null pointer (workspace / gains)");
    LM_REQUIRE(out || N == 0, "tile_intensity_apply: null out");
    if (int e = lm_tile_points_check("tile_intensity_apply", points_xyzi, N, workspace)) return e;
    LM_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)gains & 3) == 0, "tile_intensity_apply: out must be 16-byte aligned, gains 4-byte");
    LM_REQUIRE(lm_tile_intensity_apply_workspace_bytes(B) <= workspace_bytes, "tile_intensity_apply: workspace too small (%ld B needed)",
               lm_tile_intensity_apply_workspace_bytes(B));
    if (n_wg == 0) return LM_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    IntenTile* d_tiles = (IntenTile*)workspace;
    LM_HIP(hipMemcpyAsync(d_tiles, h_tiles.data(), (size_t)B * sizeof(IntenTile), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(balance_apply_kernel, dim3((unsigned)n_wg), dim3(IT), 0, s, reinterpret_cast<const f32x4*>(points_xyzi), d_tiles, B, gains,
                       reinterpret_cast<f32x4*>(out), H, W, cell_px, (int)lm_cdivl(H, cell_px), (int)lm_cdivl(W, cell_px));
    LM_LAUNCH_CHECK();
    return LM_OK;
}
