// Labelling the returns of a strip by the lane lines found in it: which points are the paint of line k, and the strip's LAS records
// back with the markings classified.  The way back of the cloud -> map route: lines in the LAS frame (what infer_las_*_to_map returns)
// against every point of the cloud.
//
// The rule (one definition: the two kernels here and tests/label_ref.py).  The lines are cut into segments on the host
// (las_io.line_segments): rows ax, ay, az, dx, dy, dz, inv, line of float32, inv = 1 / (dx^2 + dy^2) or 0, line = the int32 bits of
// (line index + 1).  Point (x, y, z, i) against a segment, plain float32, no contraction (build.py EXACT_FP):
//     px = x - ax;  py = y - ay
//     t  = fminf(fmaxf((px*dx + py*dy) * inv, 0), 1)
//     ex = px - t*dx;  ey = py - t*dy;  d2 = ex*ex + ey*ey
//     zl = az + t*dz
//     hit = d2 <= hw2  &&  fabsf(z - zl) <= z_tol
// A point is eligible when x, y, z are finite and (a min_intensity given) i >= min_intensity.  Its label is the line of the hit with the
// smallest d2, ties to the smaller line, then to the smaller segment index; no hit or not eligible: 0.  The label depends on the point and
// the index alone: no atomic decides it, every run writes the same bits.
//
// Which segments a point is tested against comes from a uniform grid built on the host (lm_line_index_build): CSR lists of the
// segments that can hit a point of the cell, a superset with margins two orders above the float32 rounding of the cell computation and of
// the distance.  The grid decides the cost, never the result.  Most points of a strip lie in cells without a segment: a wave whose 64
// points all do so skips the candidate loop.  Both kernels are streaming: 16 B read and 4 to 8 B written per point, or 2 record_len per
// record; the segment table (32 B a segment) and the lists are small and served from L2.
#include "common.h"
#include "label_rule.h"
#include "las_record.h"

#include <cmath>
#include <type_traits>
#include <vector>

namespace {

constexpr int PER = 4;                   // points per lane of label_points_kernel: four 16-byte loads in flight
constexpr int CHUNK = 256 * PER;         // points per workgroup
constexpr int HIST = 1024;               // labels counted in LDS; a larger label adds to HBM directly

// IndexDev, label_range and label_search: label_rule.h

// grid: ceil(N / 1024) workgroups
__global__ __launch_bounds__(256) void label_points_kernel(const lab_f32x4* __restrict__ pts, long N, IndexDev I, int* __restrict__ line,
                                                           float* __restrict__ dist2) {
    const long first = (long)blockIdx.x * CHUNK;
    const long left = N - first;                               // >= 1
    float4 p[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const long i = (long)j * 256 + threadIdx.x;
        const lab_f32x4 v = __builtin_nontemporal_load(pts + first + (i < left ? i : left - 1));   // unconditional, tail lanes masked below
        p[j] = float4{v[0], v[1], v[2], v[3]};
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const long i = (long)j * 256 + threadIdx.x;
        const bool valid = i < left;
        int a = 0, b = 0;
        if (valid) label_range(p[j], I, a, b);
        float best = INFINITY;
        int ln = 0;
        if (__ballot(b > a)) ln = label_search(p[j], I, a, b, best);       // wave-uniform: a wave beside the lines leaves here
        if (valid) {
            line[first + i] = ln;
            if (dist2) dist2[first + i] = best;
        }
    }
}

// grid: min(blocks of 256 records, the workgroups resident at once) workgroups; dynamic LDS = 256 records.  Per block: stage, decode + label + patch the staged
// record, store the staged words back.  counts: labels below HIST in an LDS histogram, flushed once per workgroup.  LOCAL: I.min_inten is
// the paint table's thr_min, the search also yields the winner's segment and t, and a return below its row's threshold (table_pass,
// label_rule.h) gets label 0 like one below min_intensity; T is the last argument, so the others keep their places.
struct NoTable {};
template <bool LOCAL>
__global__ __launch_bounds__(256) void las_label_kernel(const unsigned* rec, int record_len, long n, long nblk, LasXf X, LasSel S,
                                                        int use_sel, IndexDev I, int fmt6, unsigned marking_class, int write_id,
                                                        unsigned* out, int* __restrict__ line, unsigned long long* __restrict__ counts,
                                                        int L, std::conditional_t<LOCAL, TableDev, NoTable> T) {   // (out may be rec: no restrict)
    extern __shared__ unsigned lab_stage[];
    __shared__ unsigned hist[HIST];
    if (counts)
        for (int k = threadIdx.x; k < HIST; k += 256) hist[k] = 0u;       // (the barrier of the first staging orders this before the adds)
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int cnt = las_stage_block(rec, record_len, n, blk, lab_stage);
        const bool valid = (int)threadIdx.x < cnt;
        unsigned char* r = reinterpret_cast<unsigned char*>(lab_stage) + (int)threadIdx.x * record_len;
        bool pass = false;
        float4 p = {0.f, 0.f, 0.f, 0.f};
        int a = 0, b = 0;
        if (valid) {
            unsigned cls;
            if (use_sel) pass = las_record_keep(r, X, S, cls, p);
            else p = las_record_xyzi(r, X), pass = true;
            if (pass) label_range(p, I, a, b);
        }
        float best;
        int ln = 0;
        if constexpr (LOCAL) {
            if (__ballot(b > a)) {
                int s;
                float t;
                ln = label_search_t<true>(p, I, a, b, best, s, t);
                if (ln > 0 && !table_pass(T, p.w, ln, s, t)) ln = 0;
            }
        } else {
            if (__ballot(b > a)) ln = label_search(p, I, a, b, best);
        }
        if (ln > 0) {                                                      // this lane's own bytes of the stage
            if (fmt6) r[16] = (unsigned char)marking_class;
            else r[15] = (unsigned char)((r[15] & 0xE0u) | marking_class);
            if (write_id) {
                const int o = fmt6 ? 20 : 18;
                r[o] = (unsigned char)(ln & 255), r[o + 1] = (unsigned char)(ln >> 8);
            }
        }
        if (valid && line) line[blk * 256 + threadIdx.x] = ln;
        if (counts) {
            const unsigned long long none = __ballot(pass && ln == 0);
            if ((threadIdx.x & 63) == 0 && none) atomicAdd(&hist[0], (unsigned)__popcll(none));
            if (ln > 0) {
                if (ln < HIST) atomicAdd(&hist[ln], 1u);
                else if (ln <= L) atomicAdd(&counts[ln], 1ull);            // (the host checked the table's lines against L: never past counts)
            }
        }
        __syncthreads();
        const int words = (cnt * record_len + 3) / 4;
        unsigned* dst = out + blk * 256 * record_len / 4;
        for (int w = threadIdx.x; w < words; w += 256) dst[w] = lab_stage[w];
        __syncthreads();                                                   // the stage is free for the next block
    }
    if (counts)                                                            // integer adds: exact whatever the order
        for (int k = threadIdx.x; k < HIST && k <= L; k += 256)
            if (hist[k]) atomicAdd(&counts[k], (unsigned long long)hist[k]);
}

// distance in the plane from the point c to the segment a + t d, t in [0, 1] (double)
double seg_dist(double cx, double cy, double ax, double ay, double dx, double dy) {
    const double l2 = dx * dx + dy * dy;
    double t = l2 > 0 ? ((cx - ax) * dx + (cy - ay) * dy) / l2 : 0.0;
    t = t < 0 ? 0 : t > 1 ? 1 : t;
    return std::hypot(cx - ax - t * dx, cy - ay - t * dy);
}

}  // namespace

// HOST: the segment index.  segments: HOST [S][8] f32 (las_io.line_segments).  cell = 0: the default, max(1 m, 2 half_width); if the box
// of the segments, inflated by half_width, would need more than 2^24 cells the cell grows.  With cell_start == NULL and cell_segs == NULL
// only *grid is filled (n_entries = the list entries needed); otherwise cell_start [nx ny + 1] and cell_segs [n_entries] are written,
// the capacities counted in elements.  S = 0: an empty grid (nx = ny = 0).
LM_API int lm_line_index_build(const float* segments, long S, float half_width, double cell, LmLineGrid* grid, int* cell_start,
                               long cell_start_cap, int* cell_segs, long cell_segs_cap) {
    LM_REQUIRE(grid && (segments || S == 0), "line_index_build: null pointer");
    LM_REQUIRE(S >= 0 && S <= 2147483647L / 2, "line_index_build: S=%ld segments, at most 2^30 - 1 are supported", S);
    LM_REQUIRE(half_width >= 0.f && half_width < INFINITY, "line_index_build: half_width=%g must be a finite number >= 0", (double)half_width);
    LM_REQUIRE(cell >= 0 && cell < HUGE_VAL, "line_index_build: cell=%g must be a finite size > 0, or 0 for the default", cell);
    LM_REQUIRE((cell_start == nullptr) == (cell_segs == nullptr) || S == 0, "line_index_build: cell_start and cell_segs go together");
    *grid = LmLineGrid{};
    grid->half_width = half_width;
    if (S == 0) {
        if (cell_start) {
            LM_REQUIRE(cell_start_cap >= 1, "line_index_build: cell_start holds %ld entries, 1 needed", cell_start_cap);
            cell_start[0] = 0;
        }
        return LM_OK;
    }
    const double hw = half_width;
    double bx0 = HUGE_VAL, bx1 = -HUGE_VAL, by0 = HUGE_VAL, by1 = -HUGE_VAL, mar_max = 0;
    int lo = 2147483647, hi = 0;
    for (long s = 0; s < S; ++s) {
        const float* g = segments + 8 * s;
        for (int k = 0; k < 7; ++k) LM_REQUIRE(std::isfinite(g[k]), "line_index_build: segments[%ld][%d] is not finite", s, k);
        int ln;
        __builtin_memcpy(&ln, g + 7, 4);
        LM_REQUIRE(ln >= 1, "line_index_build: segments[%ld] carries line %d, lines count from 1", s, ln);
        lo = ln < lo ? ln : lo, hi = ln > hi ? ln : hi;
        const double ax = g[0], ay = g[1], ex = (double)g[0] + g[3], ey = (double)g[1] + g[4];
        bx0 = std::fmin(bx0, std::fmin(ax, ex)), bx1 = std::fmax(bx1, std::fmax(ax, ex));
        by0 = std::fmin(by0, std::fmin(ay, ey)), by1 = std::fmax(by1, std::fmax(ay, ey));
        // the float32 distance of a point near the segment: a few ulp of its largest term; 1e-5 relative is two orders above that
        mar_max = std::fmax(mar_max, 1e-5 * (std::fabs((double)g[3]) + std::fabs((double)g[4]) + hw));
    }
    const double ext = std::fmax(bx1 - bx0, by1 - by0);
    const double pad = hw + mar_max + 1e-3 * std::fmax(ext, hw) +
                       1e-6 * std::fmax(std::fmax(std::fabs(bx0), std::fabs(bx1)), std::fmax(std::fabs(by0), std::fabs(by1))) + 1e-9;
    bx0 -= pad, bx1 += pad, by0 -= pad, by1 += pad;
    LM_REQUIRE(std::isfinite(bx1 - bx0) && std::isfinite(by1 - by0), "line_index_build: the segments have no finite box");
    double cw = cell > 0 ? cell : std::fmax(1.0, 2.0 * hw);
    cw = std::fmax(cw, std::sqrt((bx1 - bx0) * (by1 - by0) / (double)MAX_CELLS));
    const float x0f = (float)bx0, y0f = (float)by0;                    // what the kernel computes with
    // (the box starts at the float corner: rounding it up must not leave a true hit below the grid - pad covers 1e-6 of the coordinate)
    long nx, ny;
    float invf;
    for (;;) {
        invf = (float)(1.0 / cw);
        const double c = 1.0 / (double)invf;
        nx = (long)std::ceil((bx1 - x0f) / c), ny = (long)std::ceil((by1 - y0f) / c);
        nx = nx < 1 ? 1 : nx, ny = ny < 1 ? 1 : ny;
        if (nx * ny <= MAX_CELLS && nx < (1L << 24) && ny < (1L << 24)) break;      // (an index must be exact in float32)
        cw *= 1.05;
    }
    cw = 1.0 / (double)invf;
    grid->x0 = x0f, grid->y0 = y0f, grid->cell = cw, grid->nx = (int)nx, grid->ny = (int)ny;
    grid->min_line = lo, grid->max_line = hi, grid->n_segments = S;
    // the kernel's cell index is floor((x - x0) * inv) in fp32: relative error of a few 2^-24 on an index below max(nx, ny)
    const double slack = cw * (1e-4 + 4e-7 * (double)(nx > ny ? nx : ny));
    const double half = 0.5 * cw + slack, diag = half * std::sqrt(2.0);
    std::vector<int> count((size_t)(nx * ny) + 1, 0);
    std::vector<int> fill;
    for (int pass = 0; pass < 2; ++pass) {
        long entries = 0;
        for (long s = 0; s < S; ++s) {
            const float* g = segments + 8 * s;
            const double ax = g[0], ay = g[1], dx = g[3], dy = g[4];
            const double reach = hw + 1e-5 * (std::fabs(dx) + std::fabs(dy) + hw) + 1e-5 * hw;
            const double sx0 = std::fmin(ax, ax + dx) - reach - slack, sx1 = std::fmax(ax, ax + dx) + reach + slack;
            const double sy0 = std::fmin(ay, ay + dy) - reach - slack, sy1 = std::fmax(ay, ay + dy) + reach + slack;
            long i0 = (long)std::floor((sx0 - x0f) / cw), i1 = (long)std::floor((sx1 - x0f) / cw);
            long j0 = (long)std::floor((sy0 - y0f) / cw), j1 = (long)std::floor((sy1 - y0f) / cw);
            i0 = i0 < 0 ? 0 : i0, j0 = j0 < 0 ? 0 : j0, i1 = i1 > nx - 1 ? nx - 1 : i1, j1 = j1 > ny - 1 ? ny - 1 : j1;
            for (long j = j0; j <= j1; ++j)
                for (long i = i0; i <= i1; ++i) {
                    // every point of the cell (with its slack) lies within `diag` of the centre
                    if (seg_dist(x0f + (i + 0.5) * cw, y0f + (j + 0.5) * cw, ax, ay, dx, dy) > reach + diag) continue;
                    const size_t c = (size_t)(j * nx + i);
                    if (pass == 0) ++count[c];
                    else cell_segs[fill[c]++] = (int)s;                // s ascends: the lists come out ascending
                    ++entries;
                }
        }
        if (pass == 0) {
            LM_REQUIRE(entries <= 2147483647L, "line_index_build: %ld list entries, at most 2^31 - 1 are supported (choose a larger cell)", entries);
            grid->n_entries = entries;
            if (!cell_start) return LM_OK;
            LM_REQUIRE(cell_start_cap >= nx * ny + 1, "line_index_build: cell_start holds %ld entries, %ld needed", cell_start_cap, nx * ny + 1);
            LM_REQUIRE(cell_segs_cap >= entries, "line_index_build: cell_segs holds %ld entries, %ld needed", cell_segs_cap, entries);
            fill.resize((size_t)(nx * ny));
            int run = 0;
            for (size_t c = 0; c < (size_t)(nx * ny); ++c) {
                cell_start[c] = fill[c] = run;
                run += count[c];
            }
            cell_start[nx * ny] = run;
        }
    }
    return LM_OK;
}

// points_xyzi: DEVICE [N][4] f32; segments / cell_start / cell_segs: DEVICE copies of what lm_line_index_build took and wrote; grid: HOST.
// line [N] int32, dist2 [N] f32 or NULL.  Asynchronous, no workspace.
LM_API int lm_label_points(void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                           const int* cell_start, const int* cell_segs, float half_width, float z_tol, float min_intensity, int* line,
                           float* dist2) {
    IndexDev I;
    if (int e = check_index("label_points", grid, S, segments, cell_start, cell_segs, half_width, z_tol, I)) return e;
    LM_REQUIRE(N >= 0 && N <= 2147483647L, "label_points: N=%ld points, at most 2^31 - 1 are supported", N);
    LM_REQUIRE(N == 0 || (points_xyzi && line), "label_points: null pointer (points_xyzi, line)");
    LM_REQUIRE(((uintptr_t)points_xyzi & 15) == 0, "label_points: points_xyzi is not 16-byte aligned");
    LM_REQUIRE(((uintptr_t)line & 3) == 0, "label_points: line is not 4-byte aligned");
    LM_REQUIRE(((uintptr_t)dist2 & 3) == 0, "label_points: dist2 is not 4-byte aligned");
    I.min_inten = min_intensity;
    if (N == 0) return LM_OK;
    hipLaunchKernelGGL(label_points_kernel, dim3((unsigned)lm_cdivl(N, CHUNK)), dim3(256), 0, (hipStream_t)hip_stream,
                       reinterpret_cast<const lab_f32x4*>(points_xyzi), N, I, line, dist2);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

namespace {

// The two record entries.  LOCAL: `table` (the paint table, checked after everything the scalar entry refuses) takes the place of
// min_intensity.
template <bool LOCAL>
int las_label_records(const char* who, void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                      const double* scale, const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                      const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width, float z_tol, float min_intensity,
                      const LmPaintTable* table, int marking_class, int write_line_id, unsigned char* records_out, int* line,
                      unsigned long* counts, int L) {
    if (int e = las_check_records(who, point_format, record_len, n)) return e;
    LM_REQUIRE(marking_class >= 0 && marking_class <= (point_format >= 6 ? 255 : 31),
               "%s: marking_class=%d does not fit format %d (0 .. %d)", who, marking_class, point_format, point_format >= 6 ? 255 : 31);
    LM_REQUIRE(L >= 0, "%s: L=%d lines", who, L);
    LM_REQUIRE(!(write_line_id && L > 65535), "%s: write_line_id with L=%d lines: the point source ID holds 16 bits", who, L);
    IndexDev I;
    if (int e = check_index(who, grid, S, segments, cell_start, cell_segs, half_width, z_tol, I)) return e;
    LM_REQUIRE(S == 0 || (grid->min_line >= 1 && grid->max_line <= L), "%s: segments carry lines %d .. %d, outside 1 .. L=%d", who,
               S ? grid->min_line : 0, S ? grid->max_line : 0, L);
    LM_REQUIRE(scale && offset && (n == 0 || (records && records_out)), "%s: null pointer (scale, offset, records, records_out)", who);
    LM_REQUIRE(((uintptr_t)records & 3) == 0, "%s: records is not 4-byte aligned", who);
    LM_REQUIRE(((uintptr_t)records_out & 3) == 0, "%s: records_out is not 4-byte aligned", who);
    LM_REQUIRE(((uintptr_t)line & 3) == 0, "%s: line is not 4-byte aligned", who);
    LM_REQUIRE(((uintptr_t)counts & 7) == 0, "%s: counts is not 8-byte aligned", who);
    LasSel Sel;
    if (int e = las_check_select(who, "select ", select, point_format, Sel)) return e;
    I.min_inten = min_intensity;
    std::conditional_t<LOCAL, TableDev, NoTable> T{};
    if constexpr (LOCAL) {
        if (int e = check_table(who, table, L, S, true, false, T)) return e;
        I.min_inten = table->thr_min;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const long nblk = (n + 255) / 256;
    const size_t lds = las_stage_bytes(record_len);
    // every workgroup walks its share of the blocks: as many workgroups as the device holds at once, so that none waits for a slot while
    // the others are half way through (registers and LDS decide how many that is)
    long resident = 0;
    if (n > 0)
        if (int e = resident_groups(las_label_kernel<LOCAL>, lds, resident)) return e;
    if (counts) LM_HIP(lm_zero_async(counts, ((size_t)L + 1) * sizeof(unsigned long), s));
    if (n == 0) return LM_OK;
    const LasXf X = las_xf(scale, offset, shift, 0.f, 1.f, 0);         // raw intensity
    const unsigned groups = (unsigned)(nblk < resident ? nblk : resident);
    hipLaunchKernelGGL(las_label_kernel<LOCAL>, dim3(groups), dim3(256), lds, s, reinterpret_cast<const unsigned*>(records), record_len, n, nblk, X,
                       Sel, select ? 1 : 0, I, point_format >= 6 ? 1 : 0, (unsigned)marking_class, write_line_id ? 1 : 0,
                       reinterpret_cast<unsigned*>(records_out), line, reinterpret_cast<unsigned long long*>(counts), L, T);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

}  // namespace

// records / records_out: DEVICE, n record_len bytes rounded up to a multiple of 4, 4-byte aligned; records_out == records is allowed, any
// other overlap is not.  line [n] int32 or NULL; counts: DEVICE [L + 1] u64 or NULL, zeroed by the call on the stream.
LM_API int lm_las_label_records(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                                const double* scale, const double* offset, const double* shift, const LmLasSelect* select,
                                const float* segments, long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs,
                                float half_width, float z_tol, float min_intensity, int marking_class, int write_line_id,
                                unsigned char* records_out, int* line, unsigned long* counts, int L) {
    return las_label_records<false>("las_label_records", hip_stream, records, record_len, point_format, n, scale, offset, shift, select, segments,
                                    S, grid, cell_start, cell_segs, half_width, z_tol, min_intensity, nullptr, marking_class, write_line_id,
                                    records_out, line, counts, L);
}

// as above with the paint table (the rule: include/lanemap_hip.h) in place of min_intensity; the stream comes LAST.
LM_API int lm_las_label_records_local(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                      const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                                      const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width, float z_tol,
                                      const LmPaintTable* table, int marking_class, int write_line_id, unsigned char* records_out, int* line,
                                      unsigned long* counts, int L, void* hip_stream) {
    return las_label_records<true>("las_label_records_local", hip_stream, records, record_len, point_format, n, scale, offset, shift, select,
                                   segments, S, grid, cell_start, cell_segs, half_width, z_tol, NAN, table, marking_class, write_line_id,
                                   records_out, line, counts, L);
}
