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
