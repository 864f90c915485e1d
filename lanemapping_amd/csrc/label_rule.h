// The labelling rule on the device, shared by the labelling (label.hip) and the marking profile (profile.hip): the index a kernel takes,
// the candidate range of a point, the search over it, and the host check of the index arguments.  The rule itself is written out in
// label.hip and include/lanemap_hip.h.  Sources that include this are built with -ffp-contract=off (build.py EXACT_FP), so the same
// expression gives the same bits in every kernel that uses it.
#pragma once
#include "common.h"

#include <cmath>

typedef float lab_f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr long MAX_CELLS = 1L << 24;

struct IndexDev {
    const float4* seg;                   // [S][2]
    const int* cell_start;
    const int* cell_segs;
    float x0, y0, inv;
    int nx, ny;                          // nx == 0: no index (S == 0), every label 0
    float hw2, z_tol, min_inten;         // min_inten NaN: none
};

// the candidate range of a point: [a, b) into cell_segs, empty where the point is not eligible or off the grid
__device__ __forceinline__ void label_range(const float4 p, const IndexDev& I, int& a, int& b) {
    a = b = 0;
    // (a NaN fails the comparisons; +-Inf fails one of them)
    bool ok = fabsf(p.x) <= 3.4028234664e38f && fabsf(p.y) <= 3.4028234664e38f && fabsf(p.z) <= 3.4028234664e38f;
    if (I.min_inten == I.min_inten) ok = ok && p.w >= I.min_inten;
    const float fx = (p.x - I.x0) * I.inv, fy = (p.y - I.y0) * I.inv;
    ok = ok && fx >= 0.f && fx < (float)I.nx && fy >= 0.f && fy < (float)I.ny;
    if (ok) {
        const int c = (int)fy * I.nx + (int)fx;
        a = I.cell_start[c];
        b = I.cell_start[c + 1];
    }
}

// the rule over the candidates [a, b): -> label (0: none), d2 of the winner (+inf: none); WIN: also the winning segment (-1: none) and
// the clamped t of the point on it
template <bool WIN>
__device__ __forceinline__ int label_search_t(const float4 p, const IndexDev& I, int a, int b, float& best, int& win, float& t_win) {
    best = INFINITY;
    int line = 0;
    if (WIN) win = -1, t_win = 0.f;
    for (int k = a; k < b; ++k) {                        // segment indices ascend inside a cell
        const int s = I.cell_segs[k];
        const float4 A = I.seg[2 * s], D = I.seg[2 * s + 1];          // ax ay az dx | dy dz inv line
        const float px = p.x - A.x, py = p.y - A.y;
        const float t = fminf(fmaxf((px * A.w + py * D.x) * D.z, 0.f), 1.f);
        const float ex = px - t * A.w, ey = py - t * D.x, d2 = ex * ex + ey * ey;
        const float zl = A.z + t * D.y;
        const int ln = __float_as_int(D.w);
        const bool hit = d2 <= I.hw2 && fabsf(p.z - zl) <= I.z_tol;
        if (hit && (d2 < best || (d2 == best && ln < line))) {       // (a hit has a finite d2: the first one beats +inf)
            best = d2;
            line = ln;
            if (WIN) win = s, t_win = t;
        }
    }
    return line;
}

__device__ __forceinline__ int label_search(const float4 p, const IndexDev& I, int a, int b, float& best) {
    int win;
    float t;
    return label_search_t<false>(p, I, a, b, best, win, t);
}

inline int check_index(const char* who, const LmLineGrid* grid, long S, const void* segments, const void* cell_start, const void* cell_segs,
                       float half_width, float z_tol, IndexDev& I) {
    LM_REQUIRE(half_width >= 0.f && half_width < INFINITY, "%s: half_width=%g must be a finite number >= 0", who, (double)half_width);
    LM_REQUIRE(z_tol >= 0.f, "%s: z_tol=%g must be a number >= 0", who, (double)z_tol);
    LM_REQUIRE(S >= 0 && S <= 2147483647L / 2, "%s: S=%ld segments, at most 2^30 - 1 are supported", who, S);
    I = IndexDev{};
    I.hw2 = half_width * half_width;
    I.z_tol = z_tol;
    if (S == 0) return LM_OK;
    LM_REQUIRE(grid && segments && cell_start && cell_segs, "%s: null pointer (segments, grid, cell_start, cell_segs)", who);
    LM_REQUIRE(grid->n_segments == S, "%s: grid was built for %ld segments, S=%ld", who, grid->n_segments, S);
    LM_REQUIRE(grid->half_width == half_width, "%s: grid was built for half_width=%g, not %g", who, (double)grid->half_width,
               (double)half_width);
    LM_REQUIRE(grid->nx >= 1 && grid->ny >= 1 && (long)grid->nx * grid->ny <= MAX_CELLS && grid->cell > 0, "%s: bad grid (%d x %d cells)", who,
               grid->nx, grid->ny);
    LM_REQUIRE(((uintptr_t)segments & 15) == 0, "%s: segments is not 16-byte aligned", who);
    LM_REQUIRE(((uintptr_t)cell_start & 3) == 0, "%s: cell_start is not 4-byte aligned", who);
    LM_REQUIRE(((uintptr_t)cell_segs & 3) == 0, "%s: cell_segs is not 4-byte aligned", who);
    I.seg = reinterpret_cast<const float4*>(segments);
    I.cell_start = reinterpret_cast<const int*>(cell_start);
    I.cell_segs = reinterpret_cast<const int*>(cell_segs);
    I.x0 = (float)grid->x0, I.y0 = (float)grid->y0, I.inv = (float)(1.0 / grid->cell);
    I.nx = grid->nx, I.ny = grid->ny;
    return LM_OK;
}

// The paint table on the device (LmPaintTable, the rule: include/lanemap_hip.h): a threshold per station window of every line, looked up
// for a return once its winner is known.  What the _local entries and the windowed histogram take beside the index.
struct TableDev {
    const float* thr;                    // [n_rows], or null in the entries that do not read it
    const int* paint_iq;                 // [n_rows], the cross entry alone
    const int* win_start;                // [L + 1]
    const float4* stations;              // [S]: s0 len rlen 0
    float inv_window;
    int L, n_rows;
};

// the row of the table for a point whose winner is segment s of line ln at t, -1: none.  The station and its window are the marking
// profile's st and b with bin = window.  win_start and stations are device tables the host cannot see: whatever they hold, a row outside
// [0, n_rows) is never returned and win_start is never read outside [0, L].
__device__ __forceinline__ int table_row(const TableDev& T, int ln, int s, float t) {
    if (ln <= 0 || ln > T.L) return -1;
    const int base = T.win_start[ln - 1], nw = T.win_start[ln] - base;
    if (base < 0 || nw <= 0 || nw > T.n_rows - base) return -1;
    const float4 St = T.stations[s];
    const float st = St.x + t * St.y;
    int w = (int)(st * T.inv_window);
    w = w < nw - 1 ? w : nw - 1;
    w = w > 0 ? w : 0;
    return base + w;
}

// whether a return of intensity i whose winner is (ln, s, t) passes its row's threshold: i >= thr[row], plain f32, a NaN fails; without a
// row nothing passes.  (i >= thr_min is label_range's test, with min_inten = thr_min.)
__device__ __forceinline__ bool table_pass(const TableDev& T, float i, int ln, int s, float t) {
    const int row = table_row(T, ln, s, t);
    return row >= 0 && i >= T.thr[row];
}

// an LmPaintTable checked on the host before anything is launched -> D.  THR: the entry reads thr (every stage but the cross-sections);
// IQ: it reads paint_iq (the cross-sections); neither: the windowed histogram, which reads the windows alone.
inline int check_table(const char* who, const LmPaintTable* T, int L, long S, bool THR, bool IQ, TableDev& D) {
    LM_REQUIRE(T, "%s: null pointer (table)", who);
    LM_REQUIRE(T->window > 0 && T->window < HUGE_VAL, "%s: table.window=%g must be a finite length > 0", who, T->window);
    LM_REQUIRE(std::fabs(T->thr_min) < INFINITY, "%s: table.thr_min=%g must be a finite number", who, (double)T->thr_min);
    LM_REQUIRE(L >= 0, "%s: L=%d lines", who, L);
    LM_REQUIRE(T->win_start_host, "%s: null pointer (table.win_start_host)", who);
    LM_REQUIRE(T->win_start_host[0] == 0, "%s: table.win_start[0]=%d must be 0", who, T->win_start_host[0]);
    for (int k = 0; k < L; ++k)
        LM_REQUIRE(T->win_start_host[k + 1] >= T->win_start_host[k], "%s: table.win_start[%d]=%d is below table.win_start[%d]=%d", who, k + 1,
                   T->win_start_host[k + 1], k, T->win_start_host[k]);
    LM_REQUIRE(T->n_rows == (long)T->win_start_host[L], "%s: table.n_rows=%ld, but table.win_start[L]=%d", who, T->n_rows, T->win_start_host[L]);
    LM_REQUIRE(S == 0 || (T->win_start && T->stations), "%s: null pointer (table.win_start, table.stations)", who);
    LM_REQUIRE(!THR || T->n_rows == 0 || T->thr, "%s: null pointer (table.thr)", who);
    LM_REQUIRE(!IQ || T->n_rows == 0 || T->paint_iq, "%s: null pointer (table.paint_iq): the cross-sections read it", who);
    LM_REQUIRE(IQ || !T->paint_iq, "%s: table.paint_iq is given, but only the cross-sections read it", who);
    LM_REQUIRE(((uintptr_t)T->thr & 3) == 0, "%s: table.thr is not 4-byte aligned", who);
    LM_REQUIRE(((uintptr_t)T->paint_iq & 3) == 0, "%s: table.paint_iq is not 4-byte aligned", who);
    LM_REQUIRE(((uintptr_t)T->win_start & 3) == 0, "%s: table.win_start is not 4-byte aligned", who);
    LM_REQUIRE(((uintptr_t)T->stations & 15) == 0, "%s: table.stations is not 16-byte aligned", who);
    D = TableDev{THR ? T->thr : nullptr, IQ ? T->paint_iq : nullptr, T->win_start, reinterpret_cast<const float4*>(T->stations),
                 (float)(1.0 / T->window), L, (int)T->n_rows};
    return LM_OK;
}

// the cloud of an entry whose only per-point buffer is points_xyzi (lm_label_points and lm_residue_keys name a second one in the same
// refusal: their checks stay with them)
inline int check_points(const char* who, const float* points_xyzi, long N) {
    LM_REQUIRE(N >= 0 && N <= 2147483647L, "%s: N=%ld points, at most 2^31 - 1 are supported", who, N);
    LM_REQUIRE(N == 0 || points_xyzi, "%s: null pointer (points_xyzi)", who);
    LM_REQUIRE(((uintptr_t)points_xyzi & 15) == 0, "%s: points_xyzi is not 16-byte aligned", who);
    return LM_OK;
}

}  // namespace
