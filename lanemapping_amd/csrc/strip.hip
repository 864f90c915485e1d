// Strip binning: one cloud [N,4] + T tile windows -> the points of tile 0, then tile 1, ... (the layout lm_bev_raster_batch takes),
// so that a whole LAS strip is cut into its (overlapping, possibly rotated) tiles on the GPU instead of on the host.
//
// Membership is the rasteriser's own window test, lm_point_window (raster_xf.h), on constants from the rasteriser's own host routine
// (lm_raster_derive): a point is in tile t exactly when raster.hip would not drop it for t.  Inside a tile the points keep their order
// in the cloud (stable), every output slot is reserved by a prefix and written with a vector store: no atomics, the same bits each run.
//
// Three passes over wave chunks (one wave = 2048 consecutive points, 32 coalesced 1 KB loads, 8 in flight per lane):
//   count    per wave a private LDS histogram over the T tiles -> table[t][chunk] (u32, tile-major), all T entries written (no memset)
//   scan     exclusive scan of the table in place (prim.hip).  The scan wraps at 2^32, the differences taken from it do not: the rank
//            of a chunk inside its tile, table[t][c] - table[t][0], is below N < 2^31; a one-workgroup kernel turns the per-tile totals
//            into the 64-bit counts[T] / offsets[T+1]
//   scatter  the same walk; the slot of a point = offsets[t] + rank of its chunk + points of t earlier in the chunk, the last term from
//            a ballot over the wave (lanes are in cloud order) added to a per-wave LDS cursor
// Which tiles a point is tested against comes from a coarse uniform grid over the union of the tile footprints, built on the host
// (lm_strip_build_grid): each cell lists the at most 8 tiles that touch it (a limit per cell, not per point), one 16-byte load per point.  A wave then takes the distinct
// tiles of its 64 points one after the other (a strip in acquisition order has one to three).  The lists are conservative for
// z in [z_lo, z_hi] (tilted tiles: the footprint moves with z); a wave holding a point outside that range, or a non-finite one, tests
// its 64 points against all T tiles instead, so the result never depends on the grid.
// HBM traffic = 16 N (count) + 16 N (scatter) + 16 sum(counts) + table; the per-wave table rows cost 4 T bytes per 32 KB of points.
//
// The chunked form (lm_strip_plan_create, lm_strip_bin_count, lm_strip_bin_scatter) bins a strip that is never held as one cloud: the
// same passes per chunk, the per-tile totals of every chunk added to a running int64 row by strip_advance_kernel - the counts in pass
// A, the cursors in pass B, which the scatter reads where it reads offsets above (and checks against the capacity: they are the
// caller's).  Chunks in cloud order give the bits of the whole-cloud call.  The grid and the tile constants go to the device once per
// layout, in a plan, instead of once per call; the whole-cloud call fills a plan of its own, and both forms run on one host path.
#include "common.h"
#include "prim.h"
#include "tile_points.h"

#include <cfloat>
#include <cmath>
#include <vector>

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int SW = 256;                  // threads per workgroup = 4 independent waves (no workgroup barrier anywhere)
constexpr int WAVES = SW / 64;
constexpr int PER_LANE = 32;
constexpr int WCHUNK = 64 * PER_LANE;    // points per wave = one column of the table
constexpr int LB = 8;                    // loads in flight per lane
constexpr int CELL_CAP = 8;              // tiles per grid cell (8 u16 = one 16-byte load)
constexpr unsigned NO_TILE = 0xFFFFu;
constexpr int MAX_T = 4096;
constexpr long MAX_CELLS = 1L << 18;
constexpr unsigned UNSET = 0xFFFFFFFFu;  // scatter cursor not yet read from the table (a real rank is < 2^31)

struct GridDev {
    float x0, y0, inv, zlo, zhi;
    int nx, ny;
};

// BOUNDED (the chunked scatter, lm_strip_bin_scatter): `offsets` are the caller's running cursors, so a slot is checked against
// `capacity` before it is written and an overrun is flagged in *err instead
template <bool SCATTER, bool BOUNDED>
struct WaveCtx {
    unsigned* cur;                       // this wave's LDS row: count of / cursor into every tile
    const unsigned* table;
    const long* offsets;
    f32x4* binned;
    long nwc, wc;
    long capacity;
    unsigned* err;
    int lane;

    // the lanes flagged in `b` (= ballot(in)) hold points of tile tt, in cloud order
    __device__ __forceinline__ void step(int tt, unsigned long long b, bool in, const f32x4 p) const {
        __builtin_amdgcn_wave_barrier();         // the lanes of the wave talk through this LDS row: keep the accesses in program order
        unsigned c = cur[tt];
        if (SCATTER) {
            if (c == UNSET) c = table[(long)tt * nwc + wc] - table[(long)tt * nwc];
            if (BOUNDED) {
                const long slot = offsets[tt] + (long)c + __popcll(b & ((1ull << lane) - 1ull));
                if (in) {
                    if ((unsigned long)slot < (unsigned long)capacity) binned[slot] = p;
                    else *err = 1u;              // (a vector store from the lane that holds the point)
                }
            } else if (in) binned[offsets[tt] + (long)c + __popcll(b & ((1ull << lane) - 1ull))] = p;
        }
        cur[tt] = c + (unsigned)__popcll(b);     // every lane stores the same value: LDS operations of one wave complete in order
        __builtin_amdgcn_wave_barrier();
    }
};

// grid: ceil(nwc / 4) workgroups; dynamic LDS = 4 * T words
template <bool SCATTER, bool BOUNDED = false>
__global__ __launch_bounds__(SW) void strip_pass_kernel(const f32x4* __restrict__ pts, long N, const LmWindowXf* __restrict__ xf, int T,
                                                        const u32x4* __restrict__ cells, GridDev G, int H, int W, unsigned* table, long nwc,
                                                        const long* __restrict__ offsets, f32x4* __restrict__ binned, long capacity,
                                                        unsigned* __restrict__ err) {
    extern __shared__ unsigned strip_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    WaveCtx<SCATTER, BOUNDED> C;
    C.cur = strip_lds + wv * T;
    C.table = table;
    C.offsets = offsets;
    C.binned = binned;
    C.nwc = nwc;
    C.capacity = capacity;
    C.err = err;
    C.wc = (long)blockIdx.x * WAVES + wv;
    C.lane = lane;
    if (C.wc >= nwc) return;
    for (int t = lane; t < T; t += 64) C.cur[t] = SCATTER ? UNSET : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const long first = C.wc * WCHUNK;
    const long left = N - first;                               // >= 1
    const f32x4* base = pts + first;
#pragma unroll 1
    for (int j0 = 0; j0 < PER_LANE; j0 += LB) {
        f32x4 pl[LB];
#pragma unroll
        for (int j = 0; j < LB; ++j) {
            const long i = (long)(j0 + j) * 64 + lane;
            pl[j] = __builtin_nontemporal_load(base + (i < left ? i : left - 1));   // unconditional, tail lanes masked below
        }
#pragma unroll
        for (int j = 0; j < LB; ++j) {
            const f32x4 p = pl[j];
            const bool valid = (long)(j0 + j) * 64 + lane < left;
            // (non-finite or absurd coordinates go the long way too: the window test of such a point is not a matter of geometry)
            const bool fast = fabsf(p[0]) <= 1e18f && fabsf(p[1]) <= 1e18f && fabsf(p[2]) <= 1e18f && p[2] >= G.zlo && p[2] <= G.zhi;
            int row, col;
            float vz;
            if (__ballot(valid && !fast)) {                    // wave-uniform: all T tiles, constants through scalar loads
                for (int t = 0; t < T; ++t) {
                    const bool in = valid && lm_point_window(p, xf[t], H, W, row, col, vz);
                    const unsigned long long b = __ballot(in);
                    if (b) C.step(t, b, in, p);
                }
                continue;
            }
            const float fx = (p[0] - G.x0) * G.inv, fy = (p[1] - G.y0) * G.inv;
            const bool on_grid = valid && fx >= 0.f && fx < (float)G.nx && fy >= 0.f && fy < (float)G.ny;
            u32x4 cl = {~0u, ~0u, ~0u, ~0u};
            if (on_grid) cl = cells[(int)fy * G.nx + (int)fx];
            unsigned id[CELL_CAP];
            unsigned pend = 0;                                 // bit k: this point is inside tile id[k] and not yet placed
#pragma unroll
            for (int k = 0; k < CELL_CAP; ++k) {
                id[k] = (cl[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                if (id[k] != NO_TILE && lm_point_window(p, xf[id[k]], H, W, row, col, vz)) pend |= 1u << k;
            }
            while (const unsigned long long any = __ballot(pend != 0)) {
                unsigned mine = NO_TILE;                       // the first lane's lowest pending tile is served next
#pragma unroll
                for (int k = CELL_CAP - 1; k >= 0; --k)
                    if (pend >> k & 1u) mine = id[k];
                const int tt = __builtin_amdgcn_readfirstlane(__shfl((int)mine, __ffsll((long long)any) - 1));
                unsigned mk = 0;
#pragma unroll
                for (int k = 0; k < CELL_CAP; ++k)
                    if ((pend >> k & 1u) && id[k] == (unsigned)tt) mk |= 1u << k;
                const bool in = mk != 0;
                C.step(tt, __ballot(in), in, p);
                pend &= ~mk;
            }
        }
    }
    if (!SCATTER) {
        for (int t = lane; t < T; t += 64) table[(long)t * nwc + C.wc] = C.cur[t];
        if (C.wc == 0 && lane == 0) table[(long)T * nwc] = 0u;   // the scan turns this last entry into the grand total (mod 2^32)
    }
}

// one workgroup: per-tile totals out of the scanned table -> counts[T], offsets[T+1] in 64 bits
__global__ __launch_bounds__(256) void strip_offsets_kernel(const unsigned* __restrict__ table, long nwc, int T, long* __restrict__ counts,
                                                            long* __restrict__ offsets) {
    __shared__ long part[256];
    const int tid = threadIdx.x, per = (T + 255) / 256;
    const int t0 = tid * per, t1 = (t0 + per < T) ? t0 + per : T;
    long s = 0;
    for (int t = t0; t < t1; ++t) s += nwc ? (long)(table[(long)(t + 1) * nwc] - table[(long)t * nwc]) : 0L;
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long run = 0;
        for (int i = 0; i < 256; ++i) {
            const long v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    long run = part[tid];
    for (int t = t0; t < t1; ++t) {
        const long c = nwc ? (long)(table[(long)(t + 1) * nwc] - table[(long)t * nwc]) : 0L;
        counts[t] = c;
        offsets[t] = run;
        run += c;
        if (t == T - 1) offsets[T] = run;
    }
}

// one workgroup, in stream order: the per-tile totals of one chunk, out of its scanned table, added to the caller's running int64 row
// (the counts of pass A, the cursors of pass B).  A tile per thread and step, nothing shared: no atomics, no LDS
__global__ __launch_bounds__(256) void strip_advance_kernel(const unsigned* __restrict__ table, long nwc, int T, long* __restrict__ running) {
    for (int t = threadIdx.x; t < T; t += 256) running[t] += (long)(table[(long)(t + 1) * nwc] - table[(long)t * nwc]);
}

long nwc_of(long N) { return (N + WCHUNK - 1) / WCHUNK; }

GridDev grid_dev(const LmStripGrid& grid, double z_lo, double z_hi) {
    GridDev G;
    G.x0 = (float)grid.x0, G.y0 = (float)grid.y0, G.inv = (float)(1.0 / grid.cell);
    G.zlo = (float)z_lo, G.zhi = (float)z_hi;
    // the lists hold for z in [z_lo, z_hi]: a float bound must not reach outside it
    if ((double)G.zlo < z_lo) G.zlo = std::nextafterf(G.zlo, INFINITY);
    if ((double)G.zhi > z_hi) G.zhi = std::nextafterf(G.zhi, -INFINITY);
    G.nx = grid.nx, G.ny = grid.ny;
    return G;
}

constexpr unsigned PLAN_MAGIC = 0x4C4D5350u;   // 'LMSP'

// The layout's constants on the device: what lm_strip_plan_create leaves behind for the chunked entries, once per layout, and what
// lm_strip_bin_points fills on its stack, once per call
struct StripPlan {
    unsigned magic;
    int T, H, W;
    GridDev G;
    const LmWindowXf* d_xf;              // both inside the caller's buffer (`consts`, or the head of the whole-cloud workspace)
    const u32x4* d_cells;
};

// ... and on the host, where plan_build leaves them and the uploads of plan_consts read them.  thread_local, no locals of an entry: an
// early error return must not end vectors while a copy may still be in flight; they hold until the thread's next call
thread_local std::vector<unsigned short> t_cells;              // [ny][nx][CELL_CAP]
thread_local std::vector<LmWindowXf> t_xf;

long consts_size(int T, long n_cells) {  // LmWindowXf[T] | cells
    return (long)(lm_align256((size_t)T * sizeof(LmWindowXf)) + lm_align256((size_t)n_cells * CELL_CAP * 2));
}

struct ChunkWork {                       // the workspace of one chunk: its table and the scan's scratch
    unsigned* table;
    void* scan_tmp;
    size_t scan_bytes;
    long nwc, L;
};

long chunk_workspace_bytes(long N, int T) {
    const long L = (long)T * nwc_of(N) + 1;
    return (long)(lm_align256((size_t)L * 4) + lm_align256(lm_prim_scan_temp_bytes(L)));
}

ChunkWork chunk_work(void* workspace, long N, int T) {         // chunk_workspace_bytes(N, T) bytes cut up
    const long nwc = nwc_of(N), L = (long)T * nwc + 1;
    return {(unsigned*)workspace, (char*)workspace + lm_align256((size_t)L * 4), lm_align256(lm_prim_scan_temp_bytes(L)), nwc, L};
}

struct Footprint {                       // one tile on the host, in double, from the float constants the device uses
    double m[6], t[3], inv[9], lo[2], hi[2];   // window in v-space: lo <= (vx, vy) <= hi
    double bb[4];                        // xmin, xmax, ymin, ymax of its footprint over z in [z_lo, z_hi]
    bool z_matters;

    void bound(double z_lo, double z_hi) {                     // footprint corners at both ends of the z range
        const double* A = inv;
        bb[0] = bb[2] = HUGE_VAL;
        bb[1] = bb[3] = -HUGE_VAL;
        for (int c = 0; c < 8; ++c) {
            const double vx = (c & 1) ? hi[0] : lo[0], vy = (c & 2) ? hi[1] : lo[1];
            double vz = 0;
            if (z_matters) vz = ((((c & 4) ? z_hi : z_lo) - t[2]) - A[6] * vx - A[7] * vy) / A[8];
            const double px = t[0] + A[0] * vx + A[1] * vy + (z_matters ? A[2] * vz : 0.0);
            const double py = t[1] + A[3] * vx + A[4] * vy + (z_matters ? A[5] * vz : 0.0);
            bb[0] = std::fmin(bb[0], px), bb[1] = std::fmax(bb[1], px);
            bb[2] = std::fmin(bb[2], py), bb[3] = std::fmax(bb[3], py);
        }
    }
};

}  // namespace

static int build_grid(const LmRasterParams* params, int T, int H, int W, double z_lo, double z_hi, LmStripGrid* grid,
                      std::vector<unsigned short>& cells) {
    LM_REQUIRE(params && grid && T >= 1 && T <= MAX_T && H > 0 && W > 0, "strip_bin: bad arguments (T=%d, at most %d tiles)", T, MAX_T);
    LM_REQUIRE(z_lo <= z_hi, "strip_bin: empty z range");
    const bool z_inf = std::isinf(z_lo) || std::isinf(z_hi);
    std::vector<Footprint> F((size_t)T);
    double bx0 = HUGE_VAL, bx1 = -HUGE_VAL, by0 = HUGE_VAL, by1 = -HUGE_VAL, min_ext = HUGE_VAL;
    for (int t = 0; t < T; ++t) {
        LM_REQUIRE(params[t].img_reso[0] > 0 && params[t].img_reso[1] > 0, "strip_bin: bad resolution (tile %d)", t);
        TileXf X;
        lm_raster_derive(params[t], 0, 0, X);
        Footprint& f = F[(size_t)t];
        for (int i = 0; i < 6; ++i) f.m[i] = X.m[i];
        for (int i = 0; i < 3; ++i) f.t[i] = X.t[i];
        const double M[9] = {X.m[0], X.m[1], X.m[2], X.m[3], X.m[4], X.m[5], X.m[6], X.m[7], X.m[8]};
        const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
        LM_REQUIRE(std::isfinite(det) && std::fabs(det) > 0, "strip_bin: degenerate quaternion (tile %d)", t);
        const double A[9] = {(M[4] * M[8] - M[5] * M[7]) / det, (M[2] * M[7] - M[1] * M[8]) / det, (M[1] * M[5] - M[2] * M[4]) / det,
                             (M[5] * M[6] - M[3] * M[8]) / det, (M[0] * M[8] - M[2] * M[6]) / det, (M[2] * M[3] - M[0] * M[5]) / det,
                             (M[3] * M[7] - M[4] * M[6]) / det, (M[1] * M[6] - M[0] * M[7]) / det, (M[0] * M[4] - M[1] * M[3]) / det};
        f.z_matters = X.m[2] != 0.f || X.m[5] != 0.f;
        LM_REQUIRE(!(f.z_matters && z_inf), "strip_bin: tile %d is tilted, a finite z range is needed", t);
        LM_REQUIRE(std::fabs(A[8]) > 1e-6 * (std::fabs(A[6]) + std::fabs(A[7]) + std::fabs(A[8])), "strip_bin: tile %d is edge-on", t);
        const double r0 = 1.0 / (double)X.irow, r1 = 1.0 / (double)X.icol;
        const double vlo[2] = {X.off[0] - 0.5 * r0, X.off[1] - 0.5 * r1}, vhi[2] = {X.off[0] + (H - 0.5) * r0, X.off[1] + (W - 0.5) * r1};
        for (int i = 0; i < 9; ++i) f.inv[i] = A[i];
        f.lo[0] = vlo[0], f.lo[1] = vlo[1], f.hi[0] = vhi[0], f.hi[1] = vhi[1];
        f.bound(z_lo, z_hi);
        LM_REQUIRE(std::isfinite(f.bb[0]) && std::isfinite(f.bb[1]) && std::isfinite(f.bb[2]) && std::isfinite(f.bb[3]),
                   "strip_bin: tile %d has no finite footprint", t);
        bx0 = std::fmin(bx0, f.bb[0]), bx1 = std::fmax(bx1, f.bb[1]), by0 = std::fmin(by0, f.bb[2]), by1 = std::fmax(by1, f.bb[3]);
        min_ext = std::fmin(min_ext, std::fmin(f.bb[1] - f.bb[0], f.bb[3] - f.bb[2]));
    }
    const double pad = 1e-3 * std::fmax(bx1 - bx0, by1 - by0) + 1e-6 * std::fmax(std::fmax(std::fabs(bx0), std::fabs(bx1)), std::fmax(std::fabs(by0), std::fabs(by1)));
    bx0 -= pad, bx1 += pad, by0 -= pad, by1 += pad;
    for (int t = 0; t < T; ++t) {
        Footprint& f = F[(size_t)t];
        // fp32 evaluation of v and of row / col: a few ulp of the largest term; 1e-5 relative is two orders above that
        const double Dx = std::fmax(std::fabs(bx0 - f.t[0]), std::fabs(bx1 - f.t[0])), Dy = std::fmax(std::fabs(by0 - f.t[1]), std::fabs(by1 - f.t[1]));
        const double Dz = f.z_matters ? std::fmax(std::fabs(z_lo - f.t[2]), std::fabs(z_hi - f.t[2])) : 0.0;
        double mar[2];
        for (int a = 0; a < 2; ++a)
            mar[a] = 1e-5 * (std::fabs(f.m[3 * a]) * Dx + std::fabs(f.m[3 * a + 1]) * Dy + std::fabs(f.m[3 * a + 2]) * Dz + std::fabs(f.lo[a]) + std::fabs(f.hi[a])) +
                     0.01 * (f.hi[a] - f.lo[a]) / (a ? W : H);
        for (int a = 0; a < 2; ++a) f.lo[a] -= mar[a], f.hi[a] += mar[a];
        f.bound(z_lo, z_hi);                                   // now with the margins
    }
    // cell: a quarter of the smallest footprint, coarser if the box would need more than MAX_CELLS of them; where a cell of that size
    // meets more than CELL_CAP tiles (windows overlapping in two directions) it is halved, up to three times, before the layout is refused
    double cell = std::fmax(min_ext / 4, std::sqrt((bx1 - bx0) * (by1 - by0) / (double)MAX_CELLS));
    LM_REQUIRE(cell > 0 && std::isfinite(cell), "strip_bin: empty tile footprint");
    const double zc = z_inf ? 0.0 : 0.5 * (z_lo + z_hi), zh = z_inf ? 0.0 : 0.5 * (z_hi - z_lo);
    for (int halved = 0;; ++halved) {
        long nx, ny;
        for (;;) {
            nx = (long)std::ceil((bx1 - bx0) / cell) + 1, ny = (long)std::ceil((by1 - by0) / cell) + 1;
            if (nx * ny <= MAX_CELLS) break;
            cell *= 1.05;
        }
        const float x0f = (float)bx0, y0f = (float)by0, invf = (float)(1.0 / cell);     // what the kernel computes with
        grid->x0 = x0f, grid->y0 = y0f, grid->cell = 1.0 / (double)invf, grid->nx = (int)nx, grid->ny = (int)ny;
        cells.assign((size_t)(nx * ny * CELL_CAP), (unsigned short)NO_TILE);
        const double cw = grid->cell;
        // the kernel's cell index is floor((x - x0) * inv) in fp32: relative error of a few 2^-24 on an index below max(nx, ny)
        const double slack = cw * (1e-4 + 4e-7 * (double)(nx > ny ? nx : ny));
        long full_i = -1, full_j = -1;
        for (int t = 0; t < T && full_i < 0; ++t) {
            const Footprint& f = F[(size_t)t];
            long i0 = (long)std::floor((f.bb[0] - x0f) / cw) - 1, i1 = (long)std::floor((f.bb[1] - x0f) / cw) + 1;
            long j0 = (long)std::floor((f.bb[2] - y0f) / cw) - 1, j1 = (long)std::floor((f.bb[3] - y0f) / cw) + 1;
            i0 = i0 < 0 ? 0 : i0, j0 = j0 < 0 ? 0 : j0, i1 = i1 > nx - 1 ? nx - 1 : i1, j1 = j1 > ny - 1 ? ny - 1 : j1;
            for (long j = j0; j <= j1 && full_i < 0; ++j)
                for (long i = i0; i <= i1; ++i) {
                    const double xl = x0f + i * cw - slack, xh = x0f + (i + 1) * cw + slack, yl = y0f + j * cw - slack, yh = y0f + (j + 1) * cw + slack;
                    if (xh < f.bb[0] || xl > f.bb[1] || yh < f.bb[2] || yl > f.bb[3]) continue;
                    const double cx = 0.5 * (xl + xh) - f.t[0], cy = 0.5 * (yl + yh) - f.t[1], cz = f.z_matters ? zc - f.t[2] : 0.0;
                    const double hx = 0.5 * (xh - xl), hy = 0.5 * (yh - yl), hz = f.z_matters ? zh : 0.0;
                    bool touch = true;
                    for (int a = 0; a < 2; ++a) {              // range of vx (vy) over the cell box against the window
                        const double c = f.m[3 * a] * cx + f.m[3 * a + 1] * cy + f.m[3 * a + 2] * cz;
                        const double r = std::fabs(f.m[3 * a]) * hx + std::fabs(f.m[3 * a + 1]) * hy + std::fabs(f.m[3 * a + 2]) * hz;
                        if (c + r < f.lo[a] || c - r > f.hi[a]) touch = false;
                    }
                    if (!touch) continue;
                    unsigned short* cl = cells.data() + (j * nx + i) * CELL_CAP;
                    int k = 0;
                    while (k < CELL_CAP && cl[k] != NO_TILE) ++k;
                    if (k == CELL_CAP) {
                        full_i = i, full_j = j;
                        break;
                    }
                    cl[k] = (unsigned short)t;
                }
        }
        if (full_i < 0) return LM_OK;
        LM_REQUIRE(halved < 3 && nx * ny * 4 <= MAX_CELLS,
                   "strip_bin: grid cell (%ld, %ld) of %ld x %ld (%.3g m) is touched by more than %d of the %d tiles", full_i, full_j, nx, ny, cw,
                   CELL_CAP, T);
        cell *= 0.5;
    }
}

// Host: the cell grid over the union of the T footprints.  cells (may be NULL: geometry only) receives [ny][nx][8] tile ids in
// ascending order, 0xFFFF = none; cells_cap = entries of 8 available.
LM_API int lm_strip_build_grid(const LmRasterParams* params, int T, int H, int W, double z_lo, double z_hi, LmStripGrid* grid,
                               unsigned short* cells, long cells_cap) {
    std::vector<unsigned short> v;
    if (int e = build_grid(params, T, H, W, z_lo, z_hi, grid, v)) return e;
    if (!cells) return LM_OK;
    LM_REQUIRE(cells_cap >= (long)grid->nx * grid->ny, "strip_bin: cell buffer too small (%ld cells needed)", (long)grid->nx * grid->ny);
    for (size_t i = 0; i < v.size(); ++i) cells[i] = v[i];
    return LM_OK;
}

// ---- the host path under both forms: the plan of a layout, its constants on the device, count and scan of a run of points -----------
// A plan but for its device pointers: T, H, W, the grid as the kernels take it; the grid's cells and the tile constants into t_cells, t_xf
static int plan_build(const LmRasterParams* params, int T, int H, int W, double z_lo, double z_hi, StripPlan* P) {
    LmStripGrid grid;
    if (int e = build_grid(params, T, H, W, z_lo, z_hi, &grid, t_cells)) return e;
    t_xf.resize((size_t)T);
    for (int t = 0; t < T; ++t) lm_window_xf(params[t], t_xf[(size_t)t]);
    P->magic = PLAN_MAGIC, P->T = T, P->H = H, P->W = W;
    P->G = grid_dev(grid, z_lo, z_hi);
    return LM_OK;
}

// LmWindowXf[T] | cells laid out in `consts` (DEVICE, 16-byte aligned, consts_size(T, the grid's cells) bytes or more), the plan
// pointed at them and, with `upload`, the two copies out of t_xf and t_cells enqueued
static int plan_consts(hipStream_t s, void* consts, bool upload, StripPlan* P) {
    P->d_xf = (const LmWindowXf*)consts;
    P->d_cells = (const u32x4*)((char*)consts + lm_align256((size_t)P->T * sizeof(LmWindowXf)));
    if (!upload) return LM_OK;
    LM_HIP(hipMemcpyAsync((void*)P->d_xf, t_xf.data(), (size_t)P->T * sizeof(LmWindowXf), hipMemcpyHostToDevice, s));
    LM_HIP(hipMemcpyAsync((void*)P->d_cells, t_cells.data(), t_cells.size() * 2, hipMemcpyHostToDevice, s));
    return LM_OK;
}

// count pass and scan of N > 0 points (the whole cloud, or one chunk) into their table
static int chunk_count(hipStream_t s, const StripPlan& P, const float* points_xyzi, long N, const ChunkWork& K, size_t lds, unsigned nblk) {
    if (int e = lm_ensure_dynamic_lds((const void*)strip_pass_kernel<false>, lds)) return e;
    hipLaunchKernelGGL(strip_pass_kernel<false>, dim3(nblk), dim3(SW), lds, s, reinterpret_cast<const f32x4*>(points_xyzi), N, P.d_xf, P.T,
                       P.d_cells, P.G, P.H, P.W, K.table, K.nwc, (const long*)nullptr, (f32x4*)nullptr, 0L, (unsigned*)nullptr);
    LM_LAUNCH_CHECK();
    return lm_prim_exclusive_scan_u32(s, K.table, K.table, K.L, K.scan_tmp, K.scan_bytes);
}

// the constants, their cells region sized for the largest grid (the grid is not known before the call), then a chunk's workspace
LM_API long lm_strip_bin_workspace_bytes(long N, int T) {
    if (N < 0 || T < 1 || T > MAX_T) return 0;
    return consts_size(T, MAX_CELLS) + chunk_workspace_bytes(N, T);
}

// points: device [N][4]; params: HOST [T]; counts [T], offsets [T+1]: device int64; offsets_host: HOST [T+1] (may be NULL);
// binned: device [capacity][4].  Synchronises the stream once (the total decides whether the scatter may run): refuses a capturing stream.
LM_API int lm_strip_bin_points(void* hip_stream, const float* points_xyzi, long N, const LmRasterParams* params, int T, int H, int W,
                               double z_lo, double z_hi, void* workspace, long workspace_bytes, long* counts, long* offsets,
                               long* offsets_host, float* binned, long capacity) {
    LM_NO_CAPTURE(hip_stream, "strip_bin", LM_WHY_HOST_COPY_SYNC);
    LM_REQUIRE(params && workspace && counts && offsets, "strip_bin: null pointer");
    LM_REQUIRE(T >= 1 && T <= MAX_T, "strip_bin: T=%d tiles, 1 to %d are supported", T, MAX_T);
    LM_REQUIRE(N >= 0 && N <= 2147483647L && capacity >= 0, "strip_bin: N=%ld points, at most 2^31 - 1 are supported", N);
    LM_REQUIRE(points_xyzi || N == 0, "strip_bin: null points");
    LM_REQUIRE(H > 0 && W > 0, "strip_bin: bad tile size");
    LM_REQUIRE(lm_strip_bin_workspace_bytes(N, T) <= workspace_bytes, "strip_bin: workspace too small (%ld B needed)",
               lm_strip_bin_workspace_bytes(N, T));
    static thread_local std::vector<long> h_off;
    StripPlan P;                                               // of this call alone: its constants lie at the head of the workspace
    if (int e = plan_build(params, T, H, W, z_lo, z_hi, &P)) return e;
    hipStream_t s = (hipStream_t)hip_stream;
    const ChunkWork K = chunk_work((char*)workspace + consts_size(T, MAX_CELLS), N, T);
    const size_t lds = (size_t)WAVES * T * sizeof(unsigned);
    const unsigned nblk = (unsigned)((K.nwc + WAVES - 1) / WAVES);
    if (int e = plan_consts(s, workspace, N > 0, &P)) return e;                    // (no points: nothing reads the constants)
    if (N > 0) {
        if (int e = lm_ensure_dynamic_lds((const void*)strip_pass_kernel<true>, lds)) return e;
        if (int e = chunk_count(s, P, points_xyzi, N, K, lds, nblk)) return e;
    }
    hipLaunchKernelGGL(strip_offsets_kernel, dim3(1), dim3(256), 0, s, K.table, K.nwc, T, counts, offsets);
    LM_LAUNCH_CHECK();
    h_off.resize((size_t)T + 1);
    long* hoff = offsets_host ? offsets_host : h_off.data();
    LM_HIP(hipMemcpyAsync(hoff, offsets, (size_t)(T + 1) * sizeof(long), hipMemcpyDeviceToHost, s));
    LM_HIP(hipStreamSynchronize(s));
    const long total = hoff[T];
    if (total > capacity) {
        lm_set_error("strip_bin: %ld points fall into the %d tiles, binned holds %ld", total, T, capacity);
        return LM_ERR_CAPACITY;
    }
    if (total > 0) {
        LM_REQUIRE(binned, "strip_bin: null output");
        hipLaunchKernelGGL(strip_pass_kernel<true>, dim3(nblk), dim3(SW), lds, s, reinterpret_cast<const f32x4*>(points_xyzi), N, P.d_xf, T,
                           P.d_cells, P.G, H, W, K.table, K.nwc, (const long*)offsets, reinterpret_cast<f32x4*>(binned), 0L,
                           (unsigned*)nullptr);
        LM_LAUNCH_CHECK();
    }
    return LM_OK;
}

// ---- the chunked form: a plan per layout, then count / scatter per chunk -------------------------------------------------------------
// n_cells: nx * ny of the layout's grid (lm_strip_build_grid with cells = NULL gives it)
LM_API long lm_strip_plan_consts_bytes(int T, long n_cells) {
    if (T < 1 || T > MAX_T || n_cells < 1 || n_cells > MAX_CELLS) return 0;
    return consts_size(T, n_cells);
}

// params: HOST [T]; consts: DEVICE, lm_strip_plan_consts_bytes(T, nx * ny) bytes, 16-byte aligned, the caller's, alive and untouched as
// long as the plan is used; *plan: the handle.  Builds the host grid and the tile constants and uploads both ONCE; synchronises the stream
LM_API int lm_strip_plan_create(const LmRasterParams* params, int T, int H, int W, double z_lo, double z_hi, void* consts, long consts_bytes,
                                void** plan, void* hip_stream) {
    LM_NO_CAPTURE(hip_stream, "strip_plan_create", LM_WHY_HOST_COPY_SYNC);
    LM_REQUIRE(params && plan, "strip_plan_create: null pointer (params, plan)");
    *plan = nullptr;
    LM_REQUIRE(T >= 1 && T <= MAX_T, "strip_plan_create: T=%d tiles, 1 to %d are supported", T, MAX_T);
    LM_REQUIRE(H > 0 && W > 0, "strip_plan_create: bad tile size (H=%d, W=%d)", H, W);
    LM_REQUIRE(consts && ((uintptr_t)consts & 15) == 0, "strip_plan_create: consts is null or not 16-byte aligned");
    StripPlan built;
    if (int e = plan_build(params, T, H, W, z_lo, z_hi, &built)) return e;
    const long need = lm_strip_plan_consts_bytes(T, (long)(t_cells.size() / CELL_CAP));
    LM_REQUIRE(consts_bytes >= need, "strip_plan_create: consts too small (%ld B needed)", need);
    hipStream_t s = (hipStream_t)hip_stream;
    if (int e = plan_consts(s, consts, true, &built)) return e;
    LM_HIP(hipStreamSynchronize(s));                           // the constants are on the device when the call returns
    *plan = new StripPlan(built);
    return LM_OK;
}

LM_API int lm_strip_plan_destroy(void* plan) {
    if (!plan) return LM_OK;
    StripPlan* P = (StripPlan*)plan;
    LM_REQUIRE(P->magic == PLAN_MAGIC, "strip_plan_destroy: plan is no handle of lm_strip_plan_create");
    P->magic = 0;
    delete P;
    return LM_OK;
}

LM_API long lm_strip_chunk_workspace_bytes(long N, int T) {
    if (N < 0 || T < 1 || T > MAX_T) return 0;
    return chunk_workspace_bytes(N, T);
}

// the checks both chunk entries share, and the chunk's workspace cut up
static int chunk_args(const char* who, const void* plan, const float* points_xyzi, long N, void* workspace, long workspace_bytes,
                      const StripPlan** P, ChunkWork* K) {
    LM_REQUIRE(plan && ((const StripPlan*)plan)->magic == PLAN_MAGIC, "%s: plan is no handle of lm_strip_plan_create", who);
    *P = (const StripPlan*)plan;
    LM_REQUIRE(N >= 0 && N <= 2147483647L, "%s: N=%ld points, at most 2^31 - 1 are supported in one chunk", who, N);
    LM_REQUIRE(points_xyzi || N == 0, "%s: null points", who);
    LM_REQUIRE(((uintptr_t)points_xyzi & 15) == 0, "%s: points is not 16-byte aligned", who);
    const int T = (*P)->T;
    LM_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: workspace is null or not 16-byte aligned", who);
    LM_REQUIRE(chunk_workspace_bytes(N, T) <= workspace_bytes, "%s: workspace too small (%ld B needed)", who, chunk_workspace_bytes(N, T));
    *K = chunk_work(workspace, N, T);
    return LM_OK;
}

// points: DEVICE [N][4], one chunk; counts_accum: DEVICE [T] int64, the caller's, zeroed by the caller before the first chunk.
// Asynchronous, nothing read back
LM_API int lm_strip_bin_count(const void* plan, const float* points_xyzi, long N, void* workspace, long workspace_bytes, long* counts_accum,
                              void* hip_stream) {
    const StripPlan* P;
    ChunkWork K;
    if (int e = chunk_args("strip_bin_count", plan, points_xyzi, N, workspace, workspace_bytes, &P, &K)) return e;
    LM_REQUIRE(counts_accum && ((uintptr_t)counts_accum & 7) == 0, "strip_bin_count: counts_accum is null or not 8-byte aligned");
    if (N == 0) return LM_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t lds = (size_t)WAVES * P->T * sizeof(unsigned);
    if (int e = chunk_count(s, *P, points_xyzi, N, K, lds, (unsigned)((K.nwc + WAVES - 1) / WAVES))) return e;
    hipLaunchKernelGGL(strip_advance_kernel, dim3(1), dim3(256), 0, s, K.table, K.nwc, P->T, counts_accum);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// cursors: DEVICE [T] int64, in and out: the slot of a point of tile t = cursors[t] + its rank among the chunk's points of t, and
// afterwards cursors[t] has grown by the chunk's count of t.  binned: DEVICE [capacity][4]; a slot outside [0, capacity) is not
// written, err (DEVICE, one int, zeroed by the caller) is set instead.  Asynchronous, nothing read back
LM_API int lm_strip_bin_scatter(const void* plan, const float* points_xyzi, long N, void* workspace, long workspace_bytes, long* cursors,
                                float* binned, long capacity, int* err, void* hip_stream) {
    const StripPlan* P;
    ChunkWork K;
    if (int e = chunk_args("strip_bin_scatter", plan, points_xyzi, N, workspace, workspace_bytes, &P, &K)) return e;
    LM_REQUIRE(cursors && ((uintptr_t)cursors & 7) == 0, "strip_bin_scatter: cursors is null or not 8-byte aligned");
    LM_REQUIRE(capacity >= 0, "strip_bin_scatter: capacity=%ld is negative", capacity);
    LM_REQUIRE((binned && ((uintptr_t)binned & 15) == 0) || capacity == 0, "strip_bin_scatter: binned is null or not 16-byte aligned");
    LM_REQUIRE(err && ((uintptr_t)err & 3) == 0, "strip_bin_scatter: err is null or not 4-byte aligned");
    if (N == 0) return LM_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t lds = (size_t)WAVES * P->T * sizeof(unsigned);
    const unsigned nblk = (unsigned)((K.nwc + WAVES - 1) / WAVES);
    if (int e = chunk_count(s, *P, points_xyzi, N, K, lds, nblk)) return e;
    if (int e = lm_ensure_dynamic_lds((const void*)strip_pass_kernel<true, true>, lds)) return e;
    hipLaunchKernelGGL((strip_pass_kernel<true, true>), dim3(nblk), dim3(SW), lds, s, reinterpret_cast<const f32x4*>(points_xyzi), N, P->d_xf,
                       P->T, P->d_cells, P->G, P->H, P->W, K.table, K.nwc, (const long*)cursors, reinterpret_cast<f32x4*>(binned), capacity,
                       reinterpret_cast<unsigned*>(err));
    LM_LAUNCH_CHECK();
    hipLaunchKernelGGL(strip_advance_kernel, dim3(1), dim3(256), 0, s, K.table, K.nwc, P->T, cursors);
    LM_LAUNCH_CHECK();
    return LM_OK;
}
