// The scaffold of the kernels that walk the point ranges of tiles: everything that consumes the (points, tile_offsets, params) triple of
// lm_bev_raster_batch next to the rasteriser itself (ground.hip, intensity.hip, drape.hip; strip.hip takes the window constants).
// Membership is the rasteriser's window test, lm_point_window (raster_xf.h), on constants from the rasteriser's host routine
// (lm_raster_derive), and that is arranged here, once:
//   LmWindowXf        the 64 bytes of per-tile constants the window test reads, and lm_window_xf() that fills them
//   LmTileRange       + the tile's point range and its first workgroup: the 88-byte prefix of a file's 96-byte per-tile struct
//   lm_tile_of        workgroup -> tile, a binary search over the per-tile prefix of workgroup counts (B up to 4096, any mix of tile
//                     sizes, one launch)
//   lm_key_of         the order-preserving u32 key of a float, for minima under integer atomic min
//   lm_stream_points  the streaming loop of a workgroup over its chunk of one tile
//   lm_tile_ranges    the host prologue: the shared argument checks, the constants and the ranges of every tile
#pragma once
#include "raster_xf.h"

#include <vector>

constexpr int LM_MAX_TILES = 4096;

struct alignas(16) LmWindowXf {              // the members of TileXf that lm_point_window reads
    float m[9], t[3], off[2], irow, icol;
};
static_assert(sizeof(LmWindowXf) == 64, "one tile's window constants are 64 bytes");

// 88 bytes of data, sizeof 96 (the alignment is inherited).  A file's tile struct derives from it and its own 8 bytes land behind
// cbase, in the tail padding a base with a base of its own leaves free: 96 bytes again, which each file asserts.  So never copy or
// assign a tile through an LmTileRange& - it would take those 8 bytes along; members are set one by one.
struct LmTileRange : LmWindowXf {
    long start, count;                       // point range in the concatenated buffer
    long cbase;                              // workgroups of the tiles before this one
};

// the rasteriser's own routine: the same float constants
static inline void lm_window_xf(const LmRasterParams& P, LmWindowXf& X) {
    TileXf T;
    lm_raster_derive(P, 0, 0, T);
    for (int i = 0; i < 9; ++i) X.m[i] = T.m[i];
    for (int i = 0; i < 3; ++i) X.t[i] = T.t[i];
    X.off[0] = T.off[0], X.off[1] = T.off[1], X.irow = T.irow, X.icol = T.icol;
}

// the tile of workgroup `wg`: the last t with cbase[t] <= wg (a tile without workgroups shares its base with its successor and is never
// chosen)
template <class T>
__device__ __forceinline__ int lm_tile_of(const T* __restrict__ tiles, int B, long wg) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tiles[mid].cbase <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Float bits with the sign bit flipped for v >= +0 and all bits flipped below: u32 order = float order, -0.0 < +0.0.  LM_KEY_EMPTY is the
// key of a NaN and above every other key; callers key finite values only.
constexpr unsigned LM_KEY_EMPTY = 0xFFFFFFFFu;
constexpr unsigned LM_QNAN_BITS = 0x7FC00000u;   // what an empty key reads as
__device__ __forceinline__ unsigned lm_key_of(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ float lm_value_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// A workgroup of THREADS lanes streams the `left` >= 1 points at `base`, at most THREADS * PER_THREAD of them: lane `tid` takes points
// tid, tid + THREADS, ... in batches of IN_FLIGHT coalesced 16-byte non-temporal loads.  The loads are unconditional (the index is
// clamped to the last point) and f(point, valid) is called for every lane of every issued batch, valid == false on the lanes past the
// end: f may be wave-collective.  Batches that lie wholly past the end are not issued (a workgroup-uniform break).
template <int THREADS, int PER_THREAD, int IN_FLIGHT, class F>
__device__ __forceinline__ void lm_stream_points(const f32x4* __restrict__ base, long left, int tid, F&& f) {
#pragma unroll 1
    for (int j0 = 0; j0 < PER_THREAD; j0 += IN_FLIGHT) {
        if ((long)j0 * THREADS >= left) break;
        f32x4 p[IN_FLIGHT];
#pragma unroll
        for (int j = 0; j < IN_FLIGHT; ++j) {
            const long i = (long)(j0 + j) * THREADS + tid;
            p[j] = __builtin_nontemporal_load(base + (i < left ? i : left - 1));
        }
#pragma unroll
        for (int j = 0; j < IN_FLIGHT; ++j) f(p[j], (long)(j0 + j) * THREADS + tid < left);
    }
}

// Host prologue of an entry that takes the triple: the shared argument checks, then out[b] = window constants, point range and cbase
// of tile b with `per` points per workgroup.  each(b, out[b], wgs) fills the file's own members and runs its per-tile checks; wgs is the
// number of workgroups tile b gets, ceil(count / per), which it may lower to 0; a non-zero return ends the call with that code.
// B = 0 (where min_B allows it) touches no pointer.  -> workgroups and points of all tiles.
template <class T, class Each>
static int lm_tile_ranges(const char* who, const long* tile_offsets, const LmRasterParams* params, int B, int min_B, int H, int W, long per,
                          std::vector<T>& out, long* n_wg, long* n_points, Each each) {
    static_assert(sizeof(T) == 96 && alignof(T) == 16, "a tile struct is LmTileRange + 8 bytes: the workspace queries count on 96");
    LM_REQUIRE(B >= min_B && B <= LM_MAX_TILES, "%s: B=%d tiles, %d to %d are supported", who, B, min_B, LM_MAX_TILES);
    LM_REQUIRE(B == 0 || (tile_offsets && params), "%s: null pointer (tile_offsets / params)", who);
    LM_REQUIRE(H > 0 && W > 0, "%s: bad tile size H=%d W=%d", who, H, W);
    *n_wg = *n_points = 0;
    out.resize((size_t)B);
    if (B == 0) return LM_OK;
    LM_REQUIRE(tile_offsets[0] >= 0, "%s: tile_offsets[0] is negative", who);
    long wg = 0;
    for (int b = 0; b < B; ++b) {
        const long n = tile_offsets[b + 1] - tile_offsets[b];
        LM_REQUIRE(n >= 0, "%s: tile_offsets must be non-decreasing (tile %d)", who, b);
        LM_REQUIRE(params[b].img_reso[0] > 0 && params[b].img_reso[1] > 0, "%s: bad resolution (tile %d)", who, b);
        T& X = out[(size_t)b];
        lm_window_xf(params[b], X);
        X.start = tile_offsets[b], X.count = n, X.cbase = wg;
        long wgs = lm_cdivl(n, per);
        if (int e = each(b, X, wgs)) return e;
        wg += wgs;
    }
    *n_wg = wg, *n_points = tile_offsets[B] - tile_offsets[0];
    return LM_OK;
}

// the checks on the device pointers that follow it
static inline int lm_tile_points_check(const char* who, const void* points, long n_points, const void* workspace) {
    LM_REQUIRE(points || n_points == 0, "%s: null points", who);
    LM_REQUIRE(((uintptr_t)points & 15) == 0 && ((uintptr_t)workspace & 15) == 0, "%s: points and workspace must be 16-byte aligned", who);
    return LM_OK;
}
