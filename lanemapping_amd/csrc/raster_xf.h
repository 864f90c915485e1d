// Per-tile constants of the LAS -> BEV rule and its window test, shared by the rasteriser (raster.hip), the strip binning (strip.hip) and
// the point-range kernels (tile_points.h): a point belongs to a tile exactly when lm_point_window() says so, in all of them, bit for bit.  All are compiled with
// -ffp-contract=off (build.py EXACT_FP): the expressions below are evaluated as written.
#pragma once
#include "common.h"

#include <cmath>

typedef float f32x4 __attribute__((ext_vector_type(4)));

// (LmRasterParams, the reference's per-tile parameter file, utils/io_utils.py:125-150: include/lanemap_hip.h)
struct TileXf {                        // derived per-tile constants (host, double -> float)
    float m[9], t[3], off[2], irow, icol, min_ele, iele, lo, hi, iscale;
    long start, count;                 // point range of the tile in the concatenated buffer
};

// The window test: v = M (p - t), row / col by floor(x + .5), unsigned compare against H and W.  XF = TileXf or any struct with its
// m, t, off, irow, icol members (LmWindowXf of tile_points.h keeps only those, 64 bytes per tile, in a device buffer).
template <class XF>
__device__ __forceinline__ bool lm_point_window(const f32x4 p, const XF& X, int H, int W, int& row, int& col, float& vz) {
    const float dx = p[0] - X.t[0], dy = p[1] - X.t[1], dz = p[2] - X.t[2];
    const float vx = (X.m[0] * dx + X.m[1] * dy) + X.m[2] * dz;
    const float vy = (X.m[3] * dx + X.m[4] * dy) + X.m[5] * dz;
    vz = (X.m[6] * dx + X.m[7] * dy) + X.m[8] * dz;
    row = (int)floorf((vx - X.off[0]) * X.irow + 0.5f);
    col = (int)floorf((vy - X.off[1]) * X.icol + 0.5f);
    return !((unsigned)row >= (unsigned)H || (unsigned)col >= (unsigned)W);
}

static inline void lm_raster_derive(const LmRasterParams& P, long start, long count, TileXf& X) {
    // inverse of the reference's rotation r(v) = q v q* / |q| = |q| R(q^) v   =>   M = R(q^)^T / |q|
    const double n = std::sqrt((double)P.quat[0] * P.quat[0] + (double)P.quat[1] * P.quat[1] + (double)P.quat[2] * P.quat[2] +
                               (double)P.quat[3] * P.quat[3]);
    const double w = P.quat[0] / n, x = P.quat[1] / n, y = P.quat[2] / n, z = P.quat[3] / n;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                         2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) X.m[i * 3 + j] = (float)(R[j * 3 + i] / n);
    for (int i = 0; i < 3; ++i) X.t[i] = P.trans[i];
    X.off[0] = P.bev_img_offset[0];
    X.off[1] = P.bev_img_offset[1];
    X.irow = 1.0f / P.img_reso[0];
    X.icol = 1.0f / P.img_reso[1];
    X.min_ele = P.local_min_ele;
    X.iele = 1.0f / P.ele_reso;
    X.lo = P.inten_lo;
    X.hi = P.inten_hi;
    X.iscale = 255.0f / P.inten_hi;
    X.start = start;
    X.count = count;
}
