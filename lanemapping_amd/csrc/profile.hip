// The marking profile: every lane line profiled from the returns that the labelling rule gives it - per station bin along the line the
// number of returns, their summed intensity, and the sum, sum of squares, minimum and maximum of their lateral offset.  What a lane map's
// user asks next after the labels: which lines are dashed, how wide the paint is, how bright (las_io.marking_summary is the host policy on
// top of the bins).
//
// The rule (one definition: the two kernels here, include/lanemap_hip.h and tests/profile_ref.py).  Eligibility, the hit test and the
// winner are label.hip's (label_rule.h).  Beside the segment table the host cuts a station table (las_io.line_stations): rows s0, len,
// rlen, 0 of float32 in the order of the segments - s0 the arc length of the line up to the segment, len its length in the plane, rlen
// 1 / len or 0 - and bin_start [L + 1], the CSR table of the bins each line owns.  For a point whose winner is segment s of line k, with
// the clamped t and px, py of the labelling rule, plain float32, no contraction (build.py EXACT_FP):
//     st = s0 + t*len
//     b  = min((int)(st * inv_bin), nb_k - 1)                        inv_bin = (float)(1 / bin), nb_k = bin_start[k] - bin_start[k-1]
//     o  = (dx*py - dy*px) * rlen                                    the signed offset, left of the line positive
//     q  = (int)rintf(o * 1024.f)
//     iq = (unsigned)fminf(fmaxf(rintf(i), 0.f), 65535.f)            a NaN intensity: 0
// and bins[bin_start[k-1] + b] takes n += 1, sum iq, sum q, sum q*q, min q, max q.  Everything is an integer sum, minimum or maximum: the
// result does not depend on the order of the points or of the adds, and every run writes the same bits.  No float atomic anywhere.
//
// Where the time goes.  Reads and search are label.hip's; the new part is the accumulation.  Paint returns arrive in scanner order: the
// lanes of a wave that hit anything mostly hit the same one to three bins, and most waves hit nothing and leave through the same
// wave-uniform exit as the label kernels.  So the lanes are merged inside the wave before anything goes to memory: loop over the distinct
// bins present in the wave (ballot, first set lane), reduce the six quantities across the lanes of that bin, and lanes 0 .. 5 issue the
// six 64-bit integer atomics of the bin's row (48 contiguous bytes).  A bin held by one lane alone skips the reduction.
//
// The colour of the markings (lm_las_line_colour_records).  Point formats 2, 3, 5, 7, 8 and 10 carry a 16-bit R, G, B triple per return
// (at byte 20, 28, 28, 30, 30, 30).  For a return that lands in a bin the same pass over the records also fills colours[bin] = n_c, sum R,
// sum G, sum B, n_yellow, n_black: a triple of three zeros is BLACK (no camera saw the point) and adds 1 to n_black and nothing else; any
// other triple is COLOURED and votes yellow when 2048 B < blue_q (R + G), blue_q in 1 .. 1024 (both sides fit 32 bits; equality is not
// yellow; the test does not depend on the scale of the triple).  Integer sums again: the same bits in every run.
// las_profile_kernel is a template for this: <false> is the profile kernel as it was, instruction for instruction; <true> reads the three
// colour words of the lane's staged record before the barrier that frees the stage and runs a second wave merge after profile_merge.  One
// kernel name, because every kernel with LDS owns a case in the LDS-state tests under its name; a separate colour pass would also read
// every record twice.
//
// Cross-sections along every line (lm_line_cross_points, lm_las_line_cross_records; the rule: include/lanemap_hip.h).  The same pass with a
// finer target: per station bin a row of nl lateral cells of n, n_paint, sum iq, sum zq over EVERY finite return of the band (no
// min_intensity).  cross_row is the one device function for the per-point terms; cross_points_kernel has profile_points_kernel's
// streaming shape and no LDS, las_profile_kernel<false, true> is the record kernel's third instantiation - <false> and <true> compile to
// the instructions they had before it existed.  Here the lanes of a wave do not share one to three bins: a wave crossing a marking hits
// about a dozen distinct rows, so cross_add's loop runs about a dozen times; it still beats four atomics per hit lane (cross_add).
//
// The paint / asphalt histograms (lm_line_hist_points, lm_las_line_hist_records; the rule: include/lanemap_hip.h).  The same search, no
// min_intensity and no station bin: per line and per lateral ring r = min(|q|, hq) / ring_q a histogram of iq >> bin_shift, one count per
// return.  hist_cell is the one device function for the per-point terms; hist_points_kernel has cross_points_kernel's streaming shape and
// no LDS, las_profile_kernel<false, false, true> is the record kernel's fourth instantiation - the other three compile to the
// instructions they had before it existed.  How a wave's counts go to memory was measured both ways: one atomic per hit lane won (hist_add).
//
// Paint thresholds per line and station window (the rule: include/lanemap_hip.h; table_row and table_pass: label_rule.h).  LOCAL is a
// fourth template parameter of las_profile_kernel: the instantiation's argument is its kind's with the paint table appended
// (WithTable), so the layouts of the four older instantiations do not move and they compile to the instructions they had.  Profile and
// colour: a return that fails its row's threshold lands in no bin; cross: a return is paint by its row's paint_iq; histogram
// (lm_las_line_hist_window_records): the row is the return's station window instead of its line.
#include "common.h"
#include "label_rule.h"
#include "las_record.h"

#include <cmath>
#include <type_traits>

namespace {

constexpr int PER = 4;                   // points per lane of profile_points_kernel, as label_points_kernel
constexpr int CHUNK = 256 * PER;
constexpr float MAX_HALF_WIDTH = 16.f;   // |q| <= 16 * 1024 + 1: q*q < 2^29, and 2^31 of them stay far inside 64 bits
constexpr long MAX_CROSS_ROWS = 1L << 27;   // rows of 32 bytes: the cross-section table stays within 4 GiB
constexpr long MAX_HIST_CELLS = 1L << 27;   // counts of 8 bytes: the histograms stay within 1 GiB and a cell fits an int

struct ProfDev {
    const float4* stations;              // [S]: s0 len rlen 0
    const int* bin_start;                // [L + 1]
    long long* bins;                     // [n_bins][6]
    int L, n_bins;
    float inv_bin;
};

struct ColourDev : ProfDev {             // what las_profile_kernel<true> takes instead
    long long* colours;                  // [n_bins][6]
    int rgb_off;                         // byte offset of R in a record
    unsigned blue_q;                     // 1 .. 1024
};

struct CrossDev : ProfDev {              // what las_profile_kernel<false, true> and cross_points_kernel take; bins: the cells [n_bins nl][4]
    int hq, lateral_q, nl;               // ceil(half_width 1024); the cell width in 1/1024 m; 2 hq / lateral_q + 1 cells per station bin
    unsigned paint_iq;                   // 0 .. 65536
};

struct HistDev {                         // what las_profile_kernel<false, false, true> and hist_points_kernel take
    const float* stations;               // [S][4]: only rlen, column 2, is read
    long long* hist;                     // [L][Z][NB]
    int L, hq, ring_q, Z, bin_shift;     // ceil(half_width 1024); the ring width in 1/1024 m; hq / ring_q + 1 rings; NB = 65536 >> bin_shift
};

template <class Base>
struct WithTable : Base {                // what a LOCAL instantiation takes: its kind's arguments, then the paint table (label_rule.h)
    TableDev T;
};

template <bool COLOUR, bool CROSS = false, bool HIST = false>
using ProfBase = std::conditional_t<HIST, HistDev, std::conditional_t<CROSS, CrossDev, std::conditional_t<COLOUR, ColourDev, ProfDev>>>;
template <bool COLOUR, bool CROSS = false, bool HIST = false, bool LOCAL = false>
using ProfArg = std::conditional_t<LOCAL, WithTable<ProfBase<COLOUR, CROSS, HIST>>, ProfBase<COLOUR, CROSS, HIST>>;

// the bin (absolute, -1: none), q and iq of a point whose winner is segment s of line ln at t.  bin_start and stations are device tables
// the host cannot see: whatever they hold, a bin outside [0, n_bins) is never returned and bin_start is never read outside [0, L].
__device__ __forceinline__ int profile_bin(const float4 p, const IndexDev& I, const ProfDev& P, int ln, int s, float t, int& q, unsigned& iq) {
    q = 0, iq = 0u;
    if (ln <= 0 || ln > P.L) return -1;
    const int base = P.bin_start[ln - 1], nb = P.bin_start[ln] - base;
    if (base < 0 || nb <= 0 || nb > P.n_bins - base) return -1;
    const float4 A = I.seg[2 * s], D = I.seg[2 * s + 1], T = P.stations[s];
    const float px = p.x - A.x, py = p.y - A.y;
    const float st = T.x + t * T.y;
    int b = (int)(st * P.inv_bin);
    b = b < nb - 1 ? b : nb - 1;
    b = b > 0 ? b : 0;                                                 // (st >= 0 in a table of las_io.line_stations)
    const float o = (A.w * py - D.x * px) * T.z;
    q = (int)rintf(o * 1024.f);
    iq = (unsigned)fminf(fmaxf(rintf(p.w), 0.f), 65535.f);
    return base + b;
}

// Wave-uniform: every lane of the wave calls it, B = -1 where the lane has nothing.  Per distinct bin of the wave one reduction and
// one row of six atomics.
__device__ __forceinline__ void profile_merge(long long* __restrict__ bins, int B, int q, unsigned iq) {
    const int lane = (int)__lane_id();
    unsigned long long todo = __ballot(B >= 0);
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const int lb = __shfl(B, leader);
        const bool mine = B == lb;
        const unsigned long long m = __ballot(mine);
        unsigned long long n = 1, siq, sqq;
        long long sq;
        int mn, mx;
        if (__popcll(m) == 1) {                                        // one lane alone: its values, read off the leader
            const int ql = __shfl(q, leader);
            siq = (unsigned)__shfl((int)iq, leader);
            sq = ql, sqq = (unsigned long long)((long long)ql * ql), mn = mx = ql;
        } else {
            n = (unsigned long long)__popcll(m);
            unsigned a_iq = mine ? iq : 0u;                            // 64 * 65535 and 64 * 16385 fit 32 bits; q*q needs 64
            int a_q = mine ? q : 0;
            unsigned long long a_qq = mine ? (unsigned long long)((long long)q * q) : 0ull;
            mn = mine ? q : 2147483647, mx = mine ? q : (-2147483647 - 1);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                a_iq += (unsigned)__shfl_xor((int)a_iq, d);
                a_q += __shfl_xor(a_q, d);
                a_qq += (unsigned long long)__shfl_xor((long long)a_qq, d);
                const int on = __shfl_xor(mn, d), ox = __shfl_xor(mx, d);
                mn = on < mn ? on : mn, mx = ox > mx ? ox : mx;
            }
            siq = a_iq, sq = a_q, sqq = a_qq;
        }
        long long* row = bins + (long)lb * 6;
        if (lane < 4) {
            const unsigned long long v = lane == 0 ? n : lane == 1 ? siq : lane == 2 ? (unsigned long long)sq : sqq;
            atomicAdd(reinterpret_cast<unsigned long long*>(row) + lane, v);
        } else if (lane == 4) {
            atomicMin(row + 4, (long long)mn);
        } else if (lane == 5) {
            atomicMax(row + 5, (long long)mx);
        }
        todo &= ~m;
    }
}

// Wave-uniform like profile_merge, for the colour row: r, g, b the triple of the lane's return (anything where B = -1).  The three sums by
// __shfl_xor (64 * 65535 fits 32 bits; a black return adds three zeros), the three counts by ballots; lanes 0 .. 5 issue the row's
// atomics, an add of 0 is left out.
__device__ __forceinline__ void colour_merge(long long* __restrict__ colours, int B, unsigned r, unsigned g, unsigned b, unsigned blue_q) {
    const int lane = (int)__lane_id();
    const bool black = (r | g | b) == 0u;
    const bool yellow = !black && 2048u * b < blue_q * (r + g);       // <= 2048 * 65535 and <= 1024 * 131070: no overflow
    unsigned long long todo = __ballot(B >= 0);
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const int lb = __shfl(B, leader);
        const bool mine = B == lb;
        const unsigned long long m = __ballot(mine);
        const unsigned long long nk = (unsigned long long)__popcll(__ballot(mine && black));
        const unsigned long long ny = (unsigned long long)__popcll(__ballot(mine && yellow));
        const unsigned long long nc = (unsigned long long)__popcll(m) - nk;
        unsigned sr, sg, sb;
        if (__popcll(m) == 1) {                                        // one lane alone: its triple, read off the leader
            sr = (unsigned)__shfl((int)r, leader), sg = (unsigned)__shfl((int)g, leader), sb = (unsigned)__shfl((int)b, leader);
        } else {
            sr = mine ? r : 0u, sg = mine ? g : 0u, sb = mine ? b : 0u;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                sr += (unsigned)__shfl_xor((int)sr, d);
                sg += (unsigned)__shfl_xor((int)sg, d);
                sb += (unsigned)__shfl_xor((int)sb, d);
            }
        }
        if (lane < 6) {
            const unsigned long long v = lane == 0 ? nc : lane == 1 ? sr : lane == 2 ? sg : lane == 3 ? sb : lane == 4 ? ny : nk;
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(colours + (long)lb * 6) + lane, v);
        }
        todo &= ~m;
    }
}

// The cross-section's per-point terms (one definition: the two kernels and include/lanemap_hip.h) for a point whose winner is segment s of
// line ln at t: -> the row of its cell in the table (-1: none), iq and zq.  The station bin, q and iq are profile_bin's, unchanged; the
// lateral cell c <= 2 hq / lateral_q = nl - 1 by the clamp of u, so a row outside [0, n_bins nl) is never returned.
__device__ __forceinline__ int cross_row(const float4 p, const IndexDev& I, const CrossDev& P, int ln, int s, float t, unsigned& iq, int& zq) {
    int q;
    zq = 0;
    const int B = profile_bin(p, I, P, ln, s, t, q, iq);
    if (B < 0) return -1;
    const float4 A = I.seg[2 * s], D = I.seg[2 * s + 1];
    const float zl = A.z + t * D.y;
    zq = (int)rintf((p.z - zl) * 1024.f);
    int u = q + P.hq;
    u = u > 0 ? u : 0;
    u = u < 2 * P.hq ? u : 2 * P.hq;
    return B * P.nl + u / P.lateral_q;
}

// Wave-uniform like profile_merge: every lane of the wave calls it, row = -1 where the lane has nothing.  Per distinct row of the wave the
// two counts by ballots and the two sums by cross-lane adds, then lanes 0 .. 3 issue the row's four 64-bit atomics (32 contiguous bytes;
// an add of 0 is left out).  A row held by one lane alone skips the reduction.  LOCAL: the return is paint by its row of the paint table (table_paint), not by P.paint_iq.  The plain form - every hit lane adding its own four
// values, zeros left out - was measured beside this one and is slower wherever a wave's lanes share rows (profiles/cross_section.txt).
template <bool LOCAL = false>
__device__ __forceinline__ void cross_add(const CrossDev& P, int row, unsigned iq, int zq, bool table_paint = false) {
    long long* __restrict__ cells = P.bins;
    const bool paint = LOCAL ? table_paint : iq >= P.paint_iq;
    const int lane = (int)__lane_id();
    unsigned long long todo = __ballot(row >= 0);
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const int lr = __shfl(row, leader);
        const bool mine = row == lr;
        const unsigned long long m = __ballot(mine);
        const unsigned long long n = (unsigned long long)__popcll(m), np = (unsigned long long)__popcll(__ballot(mine && paint));
        unsigned siq;
        int sz;
        if (n == 1) {
            siq = (unsigned)__shfl((int)iq, leader), sz = __shfl(zq, leader);
        } else {
            siq = mine ? iq : 0u, sz = mine ? zq : 0;                  // 64 * 65535 and 64 * 16385 fit 32 bits
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                siq += (unsigned)__shfl_xor((int)siq, d);
                sz += __shfl_xor(sz, d);
            }
        }
        if (lane < 4) {
            const unsigned long long v = lane == 0 ? n : lane == 1 ? np : lane == 2 ? siq : (unsigned long long)(long long)sz;
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(cells) + (long)lr * 4 + lane, v);
        }
        todo &= ~m;
    }
}

// The histogram's per-point terms (one definition: the two kernels and include/lanemap_hip.h) for a point whose winner is segment s of line
// ln: -> its cell in the table, -1: none.  q and iq are profile_bin's expressions, unchanged.  The ring r <= hq / ring_q = Z - 1 by the clamp
// of |q|, ib <= 65535 >> bin_shift = NB - 1 by the clamp of iq and ln <= L is checked: whatever the device tables hold, a cell outside
// [0, L Z NB) is never returned.
// hist_cell_at: the same for row `row` of the table, which the caller has checked - line ln - 1, or a window's row.
__device__ __forceinline__ int hist_cell_at(const float4 p, const IndexDev& I, const HistDev& H, int row, int s) {
    const float4 A = I.seg[2 * s], D = I.seg[2 * s + 1];
    const float rlen = H.stations[4 * (long)s + 2];
    const float px = p.x - A.x, py = p.y - A.y;
    const float o = (A.w * py - D.x * px) * rlen;
    const int q = (int)rintf(o * 1024.f);
    const unsigned iq = (unsigned)fminf(fmaxf(rintf(p.w), 0.f), 65535.f);
    unsigned aq = q < 0 ? 0u - (unsigned)q : (unsigned)q;              // |q|, also of -2^31
    aq = aq < (unsigned)H.hq ? aq : (unsigned)H.hq;
    const int r = (int)(aq / (unsigned)H.ring_q), NB = 65536 >> H.bin_shift;
    return (row * H.Z + r) * NB + (int)(iq >> H.bin_shift);
}
__device__ __forceinline__ int hist_cell(const float4 p, const IndexDev& I, const HistDev& H, int ln, int s) {
    if (ln <= 0 || ln > H.L) return -1;
    return hist_cell_at(p, I, H, ln - 1, s);
}

// One no-return 64-bit atomic add per hit lane (cell = -1: the lane has nothing).  Unlike the rows of cross_add a hit here is one count in
// one of Z NB cells, and the lanes of a wave rarely share one: on the bench's cloud in cell order a wave's 43.8 hit lanes fall into 42.4
// distinct cells.  The merged form - cross_add's loop over the distinct cells of the wave, the leader adding the popcount - was measured
// beside this one and is 10 to 24 % slower in all six rows of profiles/paint_threshold.txt.
__device__ __forceinline__ void hist_add(const HistDev& H, int cell) {
    if (cell >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(H.hist) + cell, 1ull);
}

// grid: ceil(n_bins * 6 / 256)
__global__ __launch_bounds__(256) void profile_init_kernel(long long* __restrict__ bins, long words) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < words) {
        const int c = (int)(i % 6);
        bins[i] = c < 4 ? 0LL : c == 4 ? 2147483647LL : -2147483648LL;
    }
}

// grid: ceil(words / 256)
__global__ __launch_bounds__(256) void colour_init_kernel(long long* __restrict__ colours, long words) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < words) colours[i] = 0LL;
}

// grid: ceil(N / 1024) workgroups
__global__ __launch_bounds__(256) void profile_points_kernel(const lab_f32x4* __restrict__ pts, long N, IndexDev I, ProfDev P) {
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
        int a = 0, b = 0;
        if (i < left) label_range(p[j], I, a, b);
        if (__ballot(b > a) == 0) continue;                    // wave-uniform: a wave beside the lines leaves here
        float best, t;
        int s;
        const int ln = label_search_t<true>(p[j], I, a, b, best, s, t);
        int q = 0, B = -1;
        unsigned iq = 0u;
        if (ln > 0) B = profile_bin(p[j], I, P, ln, s, t, q, iq);
        profile_merge(P.bins, B, q, iq);
    }
}

// grid: ceil(N / 1024) workgroups.  profile_points_kernel's streaming shape with the cross-section's accumulation; no LDS.
__global__ __launch_bounds__(256) void cross_points_kernel(const lab_f32x4* __restrict__ pts, long N, IndexDev I, CrossDev P) {
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
        int a = 0, b = 0;
        if (i < left) label_range(p[j], I, a, b);
        if (__ballot(b > a) == 0) continue;                    // wave-uniform: a wave beside the lines leaves here
        float best, t;
        int s;
        const int ln = label_search_t<true>(p[j], I, a, b, best, s, t);
        int row = -1, zq = 0;
        unsigned iq = 0u;
        if (ln > 0) row = cross_row(p[j], I, P, ln, s, t, iq, zq);
        cross_add(P, row, iq, zq);
    }
}

// grid: ceil(N / 1024) workgroups.  cross_points_kernel's streaming shape with the histogram's accumulation; no LDS.
__global__ __launch_bounds__(256) void hist_points_kernel(const lab_f32x4* __restrict__ pts, long N, IndexDev I, HistDev H) {
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
        int a = 0, b = 0;
        if (i < left) label_range(p[j], I, a, b);
        if (__ballot(b > a) == 0) continue;                    // wave-uniform: a wave beside the lines leaves here
        float best, t;
        int s;
        const int ln = label_search_t<true>(p[j], I, a, b, best, s, t);
        hist_add(H, ln > 0 ? hist_cell(p[j], I, H, ln, s) : -1);
    }
}

// grid: min(blocks of 256 records, the workgroups resident at once) workgroups; dynamic LDS = 256 records.  Per block: stage, decode into
// registers, barrier (the stage is free again), search and accumulate.  The records are only read.  COLOUR: P is a ColourDev, the lane also
// takes the R, G, B of its own staged record into registers before the barrier, and the colour row is merged after the profile's.  CROSS: P
// is a CrossDev, and after the search the cross-section's cell is accumulated instead of the profile's bin.  HIST: P is a HistDev, and the
// histogram's cell takes its place.  LOCAL: P ends in the paint table P.T (the rule: include/lanemap_hip.h).  Profile and colour: I.min_inten is
// thr_min and a return below its row's threshold lands in no bin; cross: a return is paint by its row's paint_iq; HIST: the histogram's row
// is the return's window instead of its line.  The four instantiations without LOCAL compile to the instructions they had before it.
template <bool COLOUR, bool CROSS = false, bool HIST = false, bool LOCAL = false>
__global__ __launch_bounds__(256) void las_profile_kernel(const unsigned* __restrict__ rec, int record_len, long n, long nblk, LasXf X, LasSel S,
                                                          int use_sel, IndexDev I, ProfArg<COLOUR, CROSS, HIST, LOCAL> P) {
    extern __shared__ unsigned prof_stage[];
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int cnt = las_stage_block(rec, record_len, n, blk, prof_stage);
        float4 p = {0.f, 0.f, 0.f, 0.f};
        int a = 0, b = 0;
        unsigned cr = 0u, cg = 0u, cb = 0u;
        if ((int)threadIdx.x < cnt) {
            const unsigned char* r = reinterpret_cast<const unsigned char*>(prof_stage) + (int)threadIdx.x * record_len;
            bool pass = true;
            unsigned cls;
            if (use_sel) pass = las_record_keep(r, X, S, cls, p);
            else p = las_record_xyzi(r, X);
            if (pass) label_range(p, I, a, b);                 // a record that `select` drops contributes nothing
            if constexpr (COLOUR) {                            // rgb_off + 6 <= the format's minimum record_len: inside the lane's own record
                const unsigned char* c = r + P.rgb_off;
                cr = (unsigned)c[0] | ((unsigned)c[1] << 8), cg = (unsigned)c[2] | ((unsigned)c[3] << 8), cb = (unsigned)c[4] | ((unsigned)c[5] << 8);
            }
        }
        __syncthreads();                                       // every record is in registers: the next block may be staged
        if (__ballot(b > a) == 0) continue;
        float best, t;
        int s;
        const int ln = label_search_t<true>(p, I, a, b, best, s, t);
        if constexpr (HIST && LOCAL) {
            const int w = ln > 0 && ln <= P.L ? table_row(P.T, ln, s, t) : -1;
            hist_add(P, w >= 0 ? hist_cell_at(p, I, P, w, s) : -1);
        } else if constexpr (HIST) {
            hist_add(P, ln > 0 ? hist_cell(p, I, P, ln, s) : -1);
        } else if constexpr (CROSS) {
            int row = -1, zq = 0;
            unsigned iq = 0u;
            if (ln > 0) row = cross_row(p, I, P, ln, s, t, iq, zq);
            if constexpr (LOCAL) {
                const int w = row >= 0 ? table_row(P.T, ln, s, t) : -1;
                cross_add<true>(P, row, iq, zq, w >= 0 && (int)iq >= P.T.paint_iq[w]);
            } else {
                cross_add(P, row, iq, zq);
            }
        } else {
            int q = 0, B = -1;
            unsigned iq = 0u;
            if (ln > 0) B = profile_bin(p, I, P, ln, s, t, q, iq);
            if constexpr (LOCAL)
                if (B >= 0 && !table_pass(P.T, p.w, ln, s, t)) B = -1;
            profile_merge(P.bins, B, q, iq);
            if constexpr (COLOUR) colour_merge(P.colours, B, cr, cg, cb, P.blue_q);
        }
    }
}

// What the entries take, grouped by what it describes; an LM_API entry fills these from its parameters.
struct LineArgs {                        // the lines: the index of lm_label_points and the station and bin tables on top of it
    const float* segments;
    long S;
    const LmLineGrid* grid;
    const int *cell_start, *cell_segs;
    float half_width, z_tol;
    const float* stations;
    const int *bin_start, *bin_start_host;
    int L;
    double bin;
    int accumulate;
};

struct RecordArgs {                      // the records of a file, and what decodes and selects them
    const unsigned char* records;
    int record_len, point_format;
    long n;
    const double *scale, *offset, *shift;
    const LmLasSelect* select;
};

struct TableArgs {                       // where the result goes: an entry sets the members of its kind, the others stay zero
    float min_intensity;                 // profile, colour (the cross-sections count every finite return: NaN)
    long* bins;                          // profile, colour
    long n_bins;
    long* colours;                       // colour
    int blue_q;
    long* cells;                         // cross-sections
    long n_cells;
    int lateral_q, paint_iq;
    long* hist;                          // histograms
    long n_hist;
    int ring_q, bin_shift;
    const LmPaintTable* table;           // the _local entries: the paint table in place of min_intensity / paint_iq
    const int *win_start, *win_start_host;   // the windowed histogram: its rows
    double window;
};

// the lines, up to the host copy of the bin table -> I, and P but for its table
int check_lines(const char* who, const LineArgs& A, IndexDev& I, ProfDev& P) {
    if (int e = check_index(who, A.grid, A.S, A.segments, A.cell_start, A.cell_segs, A.half_width, A.z_tol, I)) return e;
    LM_REQUIRE(A.half_width <= MAX_HALF_WIDTH, "%s: half_width=%g, at most %g m is supported (the offsets are summed in 1/1024 m)", who,
               (double)A.half_width, (double)MAX_HALF_WIDTH);
    LM_REQUIRE(A.bin > 0 && A.bin < HUGE_VAL, "%s: bin=%g must be a finite length > 0", who, A.bin);
    LM_REQUIRE(A.accumulate == 0 || A.accumulate == 1, "%s: accumulate=%d is neither 0 nor 1", who, A.accumulate);
    LM_REQUIRE(A.L >= 0, "%s: L=%d lines", who, A.L);
    LM_REQUIRE(A.S == 0 || (A.grid->min_line >= 1 && A.grid->max_line <= A.L), "%s: segments carry lines %d .. %d, outside 1 .. L=%d", who,
               A.S ? A.grid->min_line : 0, A.S ? A.grid->max_line : 0, A.L);
    LM_REQUIRE(A.bin_start_host, "%s: null pointer (bin_start_host)", who);
    LM_REQUIRE(A.bin_start_host[0] == 0, "%s: bin_start[0]=%d must be 0", who, A.bin_start_host[0]);
    for (int k = 0; k < A.L; ++k)
        LM_REQUIRE(A.bin_start_host[k + 1] >= A.bin_start_host[k], "%s: bin_start[%d]=%d is below bin_start[%d]=%d", who, k + 1,
                   A.bin_start_host[k + 1], k, A.bin_start_host[k]);
    P = ProfDev{reinterpret_cast<const float4*>(A.stations), A.bin_start, nullptr, A.L, A.bin_start_host[A.L], (float)(1.0 / A.bin)};
    return LM_OK;
}

// the two device tables of the lines: there, and aligned (two steps: the profile refuses a null `bins` between them)
int check_line_tables(const char* who, const LineArgs& A) {
    LM_REQUIRE(A.S == 0 || (A.stations && A.bin_start), "%s: null pointer (stations, bin_start)", who);
    return LM_OK;
}
int check_line_tables_aligned(const char* who, const LineArgs& A) {
    LM_REQUIRE(((uintptr_t)A.stations & 15) == 0, "%s: stations is not 16-byte aligned", who);
    LM_REQUIRE(((uintptr_t)A.bin_start & 3) == 0, "%s: bin_start is not 4-byte aligned", who);
    return LM_OK;
}

// the arguments of the profile and colour entries, checked before anything is launched or written; fills I and P
int check_profile(const char* who, const LineArgs& A, long* bins, long n_bins, IndexDev& I, ProfDev& P) {
    if (int e = check_lines(who, A, I, P)) return e;
    LM_REQUIRE(n_bins == (long)P.n_bins, "%s: n_bins=%ld, but bin_start[L]=%d", who, n_bins, P.n_bins);
    if (int e = check_line_tables(who, A)) return e;
    LM_REQUIRE(n_bins == 0 || bins, "%s: null pointer (bins)", who);
    if (int e = check_line_tables_aligned(who, A)) return e;
    LM_REQUIRE(((uintptr_t)bins & 7) == 0, "%s: bins is not 8-byte aligned", who);
    P.bins = reinterpret_cast<long long*>(bins);
    return LM_OK;
}

// the arguments of the two cross-section entries, checked likewise; fills I and P
int check_cross(const char* who, const LineArgs& A, int lateral_q, int paint_iq, long* cells, long n_cells, IndexDev& I, CrossDev& P) {
    if (int e = check_lines(who, A, I, P)) return e;
    if (int e = check_line_tables(who, A)) return e;
    if (int e = check_line_tables_aligned(who, A)) return e;
    LM_REQUIRE(((uintptr_t)cells & 7) == 0, "%s: cells is not 8-byte aligned", who);
    LM_REQUIRE(A.z_tol <= MAX_HALF_WIDTH, "%s: z_tol=%g, at most %g m is supported (the heights are summed in 1/1024 m)", who, (double)A.z_tol,
               (double)MAX_HALF_WIDTH);
    LM_REQUIRE(lateral_q >= 1, "%s: lateral_q=%d must be a cell width >= 1 (in 1/1024 m)", who, lateral_q);
    LM_REQUIRE(paint_iq >= 0 && paint_iq <= 65536, "%s: paint_iq=%d must lie in 0 .. 65536", who, paint_iq);
    P.hq = (int)std::ceil((double)A.half_width * 1024.0);              // <= 16384
    P.lateral_q = lateral_q, P.nl = 2 * P.hq / lateral_q + 1, P.paint_iq = (unsigned)paint_iq;
    const long rows = (long)P.n_bins * P.nl;
    LM_REQUIRE(rows <= MAX_CROSS_ROWS, "%s: %d bins of nl=%d cells are %ld rows, at most 2^27 are supported (choose a larger bin or lateral_q)",
               who, P.n_bins, P.nl, rows);
    LM_REQUIRE(n_cells == rows, "%s: n_cells=%ld, but bin_start[L]=%d bins of nl=%d cells are %ld", who, n_cells, P.n_bins, P.nl, rows);
    LM_REQUIRE(n_cells == 0 || cells, "%s: null pointer (cells)", who);
    P.bins = reinterpret_cast<long long*>(cells);
    return LM_OK;
}

// the arguments of the two histogram entries, checked likewise: what the cross entries refuse of the arguments they share (no bin, no
// bin_start), then the histogram's own; fills I and H.  rows: L, or (windows) the rows of the windowed histogram
int check_hist(const char* who, const LineArgs& A, int ring_q, int bin_shift, long* hist, long n_hist, long rows, bool windows, IndexDev& I, HistDev& H) {
    if (int e = check_index(who, A.grid, A.S, A.segments, A.cell_start, A.cell_segs, A.half_width, A.z_tol, I)) return e;
    LM_REQUIRE(A.half_width <= MAX_HALF_WIDTH, "%s: half_width=%g, at most %g m is supported (the offsets are taken in 1/1024 m)", who,
               (double)A.half_width, (double)MAX_HALF_WIDTH);
    LM_REQUIRE(A.accumulate == 0 || A.accumulate == 1, "%s: accumulate=%d is neither 0 nor 1", who, A.accumulate);
    LM_REQUIRE(A.L >= 0, "%s: L=%d lines", who, A.L);
    LM_REQUIRE(A.S == 0 || (A.grid->min_line >= 1 && A.grid->max_line <= A.L), "%s: segments carry lines %d .. %d, outside 1 .. L=%d", who,
               A.S ? A.grid->min_line : 0, A.S ? A.grid->max_line : 0, A.L);
    LM_REQUIRE(A.S == 0 || A.stations, "%s: null pointer (stations)", who);
    LM_REQUIRE(((uintptr_t)A.stations & 15) == 0, "%s: stations is not 16-byte aligned", who);
    LM_REQUIRE(((uintptr_t)hist & 7) == 0, "%s: hist is not 8-byte aligned", who);
    LM_REQUIRE(A.z_tol <= MAX_HALF_WIDTH, "%s: z_tol=%g, at most %g m is supported", who, (double)A.z_tol, (double)MAX_HALF_WIDTH);
    LM_REQUIRE(ring_q >= 1, "%s: ring_q=%d must be a ring width >= 1 (in 1/1024 m)", who, ring_q);
    LM_REQUIRE(bin_shift >= 0 && bin_shift <= 8, "%s: bin_shift=%d must lie in 0 .. 8", who, bin_shift);
    H = HistDev{};
    H.stations = A.stations, H.L = A.L, H.hq = (int)std::ceil((double)A.half_width * 1024.0);   // <= 16384
    H.ring_q = ring_q, H.Z = H.hq / ring_q + 1, H.bin_shift = bin_shift;
    const long NB = 65536L >> bin_shift, cells = rows * H.Z * NB;                                // < 2^31 2^15 2^16
    const char* unit = windows ? "windows" : "lines";
    LM_REQUIRE(cells <= MAX_HIST_CELLS, "%s: n_hist: %ld %s of Z=%d rings of NB=%ld counts are %ld, at most 2^27 are supported (choose a larger "
               "ring_q or bin_shift%s)", who, rows, unit, H.Z, NB, cells, windows ? ", or a longer window" : "");
    LM_REQUIRE(n_hist == cells, "%s: n_hist=%ld, but %ld %s of Z=%d rings of NB=%ld counts are %ld", who, n_hist, rows, unit, H.Z, NB, cells);
    LM_REQUIRE(n_hist == 0 || hist, "%s: null pointer (hist)", who);
    H.hist = reinterpret_cast<long long*>(hist);
    return LM_OK;
}

int init_bins(const ProfDev& P, hipStream_t s) {
    const long words = (long)P.n_bins * 6;
    if (words == 0) return LM_OK;
    hipLaunchKernelGGL(profile_init_kernel, dim3((unsigned)lm_cdivl(words, 256)), dim3(256), 0, s, P.bins, words);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// zeroes a table of `words` int64: the colours [n_bins][6], the cells [n_bins nl][4]
int zero_table(long long* table, long words, hipStream_t s) {
    if (words == 0) return LM_OK;
    hipLaunchKernelGGL(colour_init_kernel, dim3((unsigned)lm_cdivl(words, 256)), dim3(256), 0, s, table, words);
    LM_LAUNCH_CHECK();
    return LM_OK;
}
int zero_cells(const CrossDev& P, hipStream_t s) { return zero_table(P.bins, (long)P.n_bins * P.nl * 4, s); }

}  // namespace

// points_xyzi: DEVICE [N][4] f32; the index arguments of lm_label_points; stations DEVICE [S][4] f32, bin_start DEVICE [L + 1] int32,
// bin_start_host its HOST copy (what the call checks); bins DEVICE [n_bins][6] int64.  Asynchronous, no workspace.
LM_API int lm_line_profile_points(void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                                  const int* cell_start, const int* cell_segs, float half_width, const float* stations,
                                  const int* bin_start, const int* bin_start_host, int L, double bin, float z_tol, float min_intensity,
                                  int accumulate, long* bins, long n_bins) {
    IndexDev I;
    ProfDev P;
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, bin_start, bin_start_host, L, bin, accumulate};
    if (int e = check_profile("line_profile_points", A, bins, n_bins, I, P)) return e;
    if (int e = check_points("line_profile_points", points_xyzi, N)) return e;
    I.min_inten = min_intensity;
    hipStream_t s = (hipStream_t)hip_stream;
    if (!accumulate)
        if (int e = init_bins(P, s)) return e;
    if (N == 0 || S == 0 || n_bins == 0) return LM_OK;
    hipLaunchKernelGGL(profile_points_kernel, dim3((unsigned)lm_cdivl(N, CHUNK)), dim3(256), 0, s, reinterpret_cast<const lab_f32x4*>(points_xyzi),
                       N, I, P);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

namespace {

// the windows of the windowed histogram, checked like the bin table of check_lines; -> the rows, and D (the windows alone: no thr)
int check_windows(const char* who, const LineArgs& A, const TableArgs& T, TableDev& D, long& rows) {
    LM_REQUIRE(T.window > 0 && T.window < HUGE_VAL, "%s: window=%g must be a finite length > 0", who, T.window);
    LM_REQUIRE(A.L >= 0, "%s: L=%d lines", who, A.L);
    LM_REQUIRE(T.win_start_host, "%s: null pointer (win_start_host)", who);
    LM_REQUIRE(T.win_start_host[0] == 0, "%s: win_start[0]=%d must be 0", who, T.win_start_host[0]);
    for (int k = 0; k < A.L; ++k)
        LM_REQUIRE(T.win_start_host[k + 1] >= T.win_start_host[k], "%s: win_start[%d]=%d is below win_start[%d]=%d", who, k + 1,
                   T.win_start_host[k + 1], k, T.win_start_host[k]);
    LM_REQUIRE(A.S == 0 || T.win_start, "%s: null pointer (win_start)", who);
    LM_REQUIRE(((uintptr_t)T.win_start & 3) == 0, "%s: win_start is not 4-byte aligned", who);
    rows = T.win_start_host[A.L];
    D = TableDev{nullptr, nullptr, T.win_start, reinterpret_cast<const float4*>(A.stations), (float)(1.0 / T.window), A.L, (int)rows};
    return LM_OK;
}

// The record entries.  COLOUR: blue_q and colours are checked after everything the profile entry refuses, both tensors are initialised,
// and las_profile_kernel<true> fills both in its one pass over the records.  CROSS: the cells take the place of the bins.  HIST: the
// histograms do.  LOCAL: the paint table T.table is checked after the scalar entry's arguments and rides at the end of P; with HIST the
// table is the windows alone and the histogram has a row per window.
template <bool COLOUR, bool CROSS, bool HIST = false, bool LOCAL = false>
int las_profile_records(const char* who, void* hip_stream, const RecordArgs& R, const LineArgs& A, const TableArgs& T) {
    static const int rgb_off[11] = {-1, -1, 20, 28, -1, 28, -1, 30, 30, -1, 30};      // rgb_off + 6 <= las_min_len wherever there is colour
    if (int e = las_check_records(who, R.point_format, R.record_len, R.n)) return e;
    IndexDev I;
    ProfArg<COLOUR, CROSS, HIST, LOCAL> P;
    long n_table;                                                      // the table's rows: without one there is nothing to launch
    if constexpr (HIST && LOCAL) {
        long rows = 0;
        if (int e = check_windows(who, A, T, P.T, rows)) return e;
        if (int e = check_hist(who, A, T.ring_q, T.bin_shift, T.hist, T.n_hist, rows, true, I, P)) return e;
    } else if constexpr (HIST) {
        if (int e = check_hist(who, A, T.ring_q, T.bin_shift, T.hist, T.n_hist, A.L, false, I, P)) return e;
    } else if constexpr (CROSS) {
        if (int e = check_cross(who, A, T.lateral_q, LOCAL ? 0 : T.paint_iq, T.cells, T.n_cells, I, P)) return e;
    } else {
        if (int e = check_profile(who, A, T.bins, T.n_bins, I, P)) return e;
    }
    if constexpr (HIST) n_table = T.n_hist;
    else n_table = P.n_bins;
    LM_REQUIRE(R.scale && R.offset && (R.n == 0 || R.records), "%s: null pointer (scale, offset, records)", who);
    LM_REQUIRE(((uintptr_t)R.records & 3) == 0, "%s: records is not 4-byte aligned", who);
    LasSel Sel;
    if (int e = las_check_select(who, "select ", R.select, R.point_format, Sel)) return e;
    if constexpr (COLOUR) {
        LM_REQUIRE(rgb_off[R.point_format] >= 0, "%s: point_format=%d carries no RGB (formats 2, 3, 5, 7, 8 and 10 do)", who, R.point_format);
        LM_REQUIRE(T.blue_q >= 1 && T.blue_q <= 1024, "%s: blue_q=%d must lie in 1 .. 1024", who, T.blue_q);
        LM_REQUIRE(T.n_bins == 0 || T.colours, "%s: null pointer (colours)", who);
        LM_REQUIRE(((uintptr_t)T.colours & 7) == 0, "%s: colours is not 8-byte aligned", who);
        const uintptr_t b0 = (uintptr_t)T.bins, c0 = (uintptr_t)T.colours, bytes = (uintptr_t)T.n_bins * 48;
        LM_REQUIRE(T.n_bins == 0 || b0 + bytes <= c0 || c0 + bytes <= b0, "%s: colours overlaps bins", who);
        P.colours = reinterpret_cast<long long*>(T.colours), P.rgb_off = rgb_off[R.point_format], P.blue_q = (unsigned)T.blue_q;
    }
    I.min_inten = T.min_intensity;
    if constexpr (LOCAL && !HIST) {
        if (int e = check_table(who, T.table, A.L, A.S, !CROSS, CROSS, P.T)) return e;
        if constexpr (!CROSS) {
            I.min_inten = T.table->thr_min;
            if (P.T.n_rows == 0) n_table = 0;                           // no row: nothing passes - the initialised table
        }
    }
    hipStream_t s = (hipStream_t)hip_stream;
    const bool work = R.n > 0 && A.S > 0 && n_table > 0;
    const long nblk = (R.n + 255) / 256;
    const size_t lds = las_stage_bytes(R.record_len);
    long resident = 0;
    if (work)
        if (int e = resident_groups(las_profile_kernel<COLOUR, CROSS, HIST, LOCAL>, lds, resident)) return e;
    if (!A.accumulate) {
        if constexpr (HIST) {
            LM_HIP(lm_zero_async(P.hist, (size_t)T.n_hist * sizeof(long long), s));
        } else if constexpr (CROSS) {
            if (int e = zero_cells(P, s)) return e;
        } else {
            if (int e = init_bins(P, s)) return e;
            if constexpr (COLOUR)
                if (int e = zero_table(P.colours, (long)P.n_bins * 6, s)) return e;
        }
    }
    if (!work) return LM_OK;
    const LasXf X = las_xf(R.scale, R.offset, R.shift, 0.f, 1.f, 0);  // raw intensity
    const unsigned groups = (unsigned)(nblk < resident ? nblk : resident);
    hipLaunchKernelGGL((las_profile_kernel<COLOUR, CROSS, HIST, LOCAL>), dim3(groups), dim3(256), lds, s, reinterpret_cast<const unsigned*>(R.records),
                       R.record_len, R.n, nblk, X, Sel, R.select ? 1 : 0, I, P);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

}  // namespace

// records: DEVICE, n record_len bytes rounded up to a multiple of 4, 4-byte aligned, only read; the rest as above.
LM_API int lm_las_line_profile_records(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                                       const double* scale, const double* offset, const double* shift, const LmLasSelect* select,
                                       const float* segments, long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs,
                                       float half_width, const float* stations, const int* bin_start, const int* bin_start_host, int L,
                                       double bin, float z_tol, float min_intensity, int accumulate, long* bins, long n_bins) {
    const RecordArgs R{records, record_len, point_format, n, scale, offset, shift, select};
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, bin_start, bin_start_host, L, bin, accumulate};
    TableArgs T{};
    T.min_intensity = min_intensity, T.bins = bins, T.n_bins = n_bins;
    return las_profile_records<false, false>("las_line_profile_records", hip_stream, R, A, T);
}

// as above, point formats 2, 3, 5, 7, 8, 10; colours DEVICE [n_bins][6] int64, disjoint from bins.  One pass over the records fills both.
LM_API int lm_las_line_colour_records(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                                      const double* scale, const double* offset, const double* shift, const LmLasSelect* select,
                                      const float* segments, long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs,
                                      float half_width, const float* stations, const int* bin_start, const int* bin_start_host, int L,
                                      double bin, float z_tol, float min_intensity, int blue_q, int accumulate, long* bins, long* colours,
                                      long n_bins) {
    const RecordArgs R{records, record_len, point_format, n, scale, offset, shift, select};
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, bin_start, bin_start_host, L, bin, accumulate};
    TableArgs T{};
    T.min_intensity = min_intensity, T.bins = bins, T.n_bins = n_bins, T.colours = colours, T.blue_q = blue_q;
    return las_profile_records<true, false>("las_line_colour_records", hip_stream, R, A, T);
}

// The cross-sections along every line (the rule: include/lanemap_hip.h).  The arguments of lm_line_profile_points without min_intensity -
// every finite return counts -, then lateral_q, paint_iq; cells DEVICE [n_cells][4] int64, n_cells = bin_start_host[L] nl.
LM_API int lm_line_cross_points(void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                                const int* cell_start, const int* cell_segs, float half_width, const float* stations, const int* bin_start,
                                const int* bin_start_host, int L, double bin, float z_tol, int lateral_q, int paint_iq, int accumulate,
                                long* cells, long n_cells) {
    IndexDev I;
    CrossDev P;
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, bin_start, bin_start_host, L, bin, accumulate};
    if (int e = check_cross("line_cross_points", A, lateral_q, paint_iq, cells, n_cells, I, P)) return e;
    if (int e = check_points("line_cross_points", points_xyzi, N)) return e;
    I.min_inten = NAN;
    hipStream_t s = (hipStream_t)hip_stream;
    if (!accumulate)
        if (int e = zero_cells(P, s)) return e;
    if (N == 0 || S == 0 || n_cells == 0) return LM_OK;
    hipLaunchKernelGGL(cross_points_kernel, dim3((unsigned)lm_cdivl(N, CHUNK)), dim3(256), 0, s, reinterpret_cast<const lab_f32x4*>(points_xyzi),
                       N, I, P);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// as above on the records of a file: the inputs of lm_las_line_profile_records.  las_profile_kernel<false, true>: one pass, records only read.
LM_API int lm_las_line_cross_records(void* hip_stream, const unsigned char* records, int record_len, int point_format, long n,
                                     const double* scale, const double* offset, const double* shift, const LmLasSelect* select,
                                     const float* segments, long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs,
                                     float half_width, const float* stations, const int* bin_start, const int* bin_start_host, int L,
                                     double bin, float z_tol, int lateral_q, int paint_iq, int accumulate, long* cells, long n_cells) {
    const RecordArgs R{records, record_len, point_format, n, scale, offset, shift, select};
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, bin_start, bin_start_host, L, bin, accumulate};
    TableArgs T{};
    T.min_intensity = NAN, T.cells = cells, T.n_cells = n_cells, T.lateral_q = lateral_q, T.paint_iq = paint_iq;
    return las_profile_records<false, true>("las_line_cross_records", hip_stream, R, A, T);
}

// The paint / asphalt histograms (the rule: include/lanemap_hip.h): per line and lateral ring a histogram of the intensities of the returns
// the labelling rule gives the line, without a min_intensity.  The index arguments of lm_label_points, then stations (only rlen is read),
// L, z_tol, ring_q, bin_shift; hist DEVICE [L][Z][NB] int64, n_hist = L Z NB.  The stream comes LAST (the note in the header says why).
LM_API int lm_line_hist_points(const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid, const int* cell_start,
                               const int* cell_segs, float half_width, const float* stations, int L, float z_tol, int ring_q, int bin_shift,
                               int accumulate, long* hist, long n_hist, void* hip_stream) {
    IndexDev I;
    HistDev H;
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, nullptr, nullptr, L, 0.0, accumulate};
    if (int e = check_hist("line_hist_points", A, ring_q, bin_shift, hist, n_hist, L, false, I, H)) return e;
    if (int e = check_points("line_hist_points", points_xyzi, N)) return e;
    I.min_inten = NAN;
    hipStream_t s = (hipStream_t)hip_stream;
    if (!accumulate) LM_HIP(lm_zero_async(hist, (size_t)n_hist * sizeof(long long), s));
    if (N == 0 || S == 0 || n_hist == 0) return LM_OK;
    hipLaunchKernelGGL(hist_points_kernel, dim3((unsigned)lm_cdivl(N, CHUNK)), dim3(256), 0, s, reinterpret_cast<const lab_f32x4*>(points_xyzi),
                       N, I, H);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// as above on the records of a file: the inputs of lm_las_line_cross_records.  las_profile_kernel<false, false, true>: one pass, records
// only read.
LM_API int lm_las_line_hist_records(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                    const double* offset, const double* shift, const LmLasSelect* select, const float* segments, long S,
                                    const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                    const float* stations, int L, float z_tol, int ring_q, int bin_shift, int accumulate, long* hist,
                                    long n_hist, void* hip_stream) {
    const RecordArgs R{records, record_len, point_format, n, scale, offset, shift, select};
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, nullptr, nullptr, L, 0.0, accumulate};
    TableArgs T{};
    T.min_intensity = NAN, T.hist = hist, T.n_hist = n_hist, T.ring_q = ring_q, T.bin_shift = bin_shift;
    return las_profile_records<false, false, true>("las_line_hist_records", hip_stream, R, A, T);
}

// The windowed histogram (the rule: include/lanemap_hip.h): lm_las_line_hist_records with a row per station window of every line instead
// of one per line.  hist DEVICE [R][Z][NB] int64, R = win_start_host[L].  las_profile_kernel<false, false, true, true>.
LM_API int lm_las_line_hist_window_records(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                           const double* offset, const double* shift, const LmLasSelect* select, const float* segments,
                                           long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                           const float* stations, int L, float z_tol, int ring_q, int bin_shift, int accumulate, long* hist,
                                           long n_hist, const int* win_start, const int* win_start_host, double window, void* hip_stream) {
    const RecordArgs R{records, record_len, point_format, n, scale, offset, shift, select};
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, nullptr, nullptr, L, 0.0, accumulate};
    TableArgs T{};
    T.min_intensity = NAN, T.hist = hist, T.n_hist = n_hist, T.ring_q = ring_q, T.bin_shift = bin_shift;
    T.win_start = win_start, T.win_start_host = win_start_host, T.window = window;
    return las_profile_records<false, false, true, true>("las_line_hist_window_records", hip_stream, R, A, T);
}

// The three _local record entries of this file (the rule: include/lanemap_hip.h): the scalar entry's arguments with the paint table in
// place of min_intensity / paint_iq, and the scalar entry's kernel with LOCAL set.
LM_API int lm_las_line_profile_records_local(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                             const double* offset, const double* shift, const LmLasSelect* select, const float* segments,
                                             long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                             const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin,
                                             float z_tol, const LmPaintTable* table, int accumulate, long* bins, long n_bins,
                                             void* hip_stream) {
    const RecordArgs R{records, record_len, point_format, n, scale, offset, shift, select};
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, bin_start, bin_start_host, L, bin, accumulate};
    TableArgs T{};
    T.min_intensity = NAN, T.bins = bins, T.n_bins = n_bins, T.table = table;
    return las_profile_records<false, false, false, true>("las_line_profile_records_local", hip_stream, R, A, T);
}

LM_API int lm_las_line_colour_records_local(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                            const double* offset, const double* shift, const LmLasSelect* select, const float* segments,
                                            long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                            const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin,
                                            float z_tol, const LmPaintTable* table, int blue_q, int accumulate, long* bins, long* colours,
                                            long n_bins, void* hip_stream) {
    const RecordArgs R{records, record_len, point_format, n, scale, offset, shift, select};
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, bin_start, bin_start_host, L, bin, accumulate};
    TableArgs T{};
    T.min_intensity = NAN, T.bins = bins, T.n_bins = n_bins, T.colours = colours, T.blue_q = blue_q, T.table = table;
    return las_profile_records<true, false, false, true>("las_line_colour_records_local", hip_stream, R, A, T);
}

LM_API int lm_las_line_cross_records_local(const unsigned char* records, int record_len, int point_format, long n, const double* scale,
                                           const double* offset, const double* shift, const LmLasSelect* select, const float* segments,
                                           long S, const LmLineGrid* grid, const int* cell_start, const int* cell_segs, float half_width,
                                           const float* stations, const int* bin_start, const int* bin_start_host, int L, double bin,
                                           float z_tol, int lateral_q, const LmPaintTable* table, int accumulate, long* cells, long n_cells,
                                           void* hip_stream) {
    const RecordArgs R{records, record_len, point_format, n, scale, offset, shift, select};
    const LineArgs A{segments, S, grid, cell_start, cell_segs, half_width, z_tol, stations, bin_start, bin_start_host, L, bin, accumulate};
    TableArgs T{};
    T.min_intensity = NAN, T.cells = cells, T.n_cells = n_cells, T.lateral_q = lateral_q, T.table = table;
    return las_profile_records<false, true, false, true>("las_line_cross_records_local", hip_stream, R, A, T);
}
