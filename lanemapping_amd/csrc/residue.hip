// The paint no lane line explains: the bright, road-level returns of a strip that lie near a line the call found but not on one - stop
// bars, crossing bars, arrows, hatching, a line the network missed - put on a sparse map-frame grid, its connected blobs found, and every
// blob described by exact integer footprint statistics.  las_io.residue_summary is the host policy on top (centre, area, length, width,
// fill, heading against the nearest line); naming a blob is left to the user.
//
// The rule (one definition: include/lanemap_hip.h; the kernels here and tests/residue_ref.py restate it).  Per point, plain float32, no
// contraction (build.py EXACT_FP), against a LineIndex built with half_width = reach and a finite min_intensity:
//     ln, d2 = the labelling rule's winner and its squared distance (label_rule.h: eligibility, hit test and z_tol are that rule's)
//     residue = ln > 0 && d2 > clear2                                clear2 = clear * clear, squared once in f32
//     cx = (int)((x - x0) * inv);  cy = (int)((y - y0) * inv)         x0, y0 the index grid's f32 origin, inv = (f32)(1 / cell)
//     key = (int64)cy * nx + cx      for a residue point with 0 <= cx < nx and 0 <= cy < ny, else -1
//     iq  = (unsigned)fminf(fmaxf(rintf(i), 0.f), 65535.f)            for a point with a key >= 0, else 0
// The cells are the distinct keys >= 0 in ascending order; two cells are joined when they are neighbours on (cx, cy) under the
// connectivity (8 or 4); root[m] is the smallest cell index of the component of cell m.  The statistics of a component are integer sums,
// minima and maxima over its cells (each once) and over the points in them.  Nothing depends on the order of points, cells or adds.
//
// Three entries, all without LDS (wave-private cross-lane operations and ballots only) and without a workspace:
//   lm_residue_keys      label_points_kernel's streaming shape - four 16-byte loads in flight per lane, 16 B read and 8 to 12 B written
//                        per point; a wave with no candidate leaves through the ballot.
//   lm_cell_components   THE UNION-FIND FORM: init (parent[m] = m), one union launch, one compression launch.  A lane per cell looks its
//                        "earlier" neighbours (smaller key: 4 of 8, or 2 of 4) up by binary search in keys[0, m) and joins what it finds by
//                        a lock-free union-find that only ever hooks a larger root under a smaller one with atomicMin.  parent[x] <= x
//                        holds at every moment, so a chase descends strictly and the final root of a tree is its smallest index whatever
//                        the interleaving.  No lane waits for another: every loop advances by the lane's own action.  Every loop carries a
//                        cap derived from M (a chase: at most M links; the hook: every retry lowers the larger of the two indices, at
//                        most 2 M times); a lane that exhausts one sets err[0] with an atomic and leaves.  Inside the union and the
//                        compression launch every word of `parent` is read with an agent-scope atomic load or as the return value of an
//                        atomic and written only with atomics (one L2 per XCD: a plain load may be served from another CU's stale
//                        line); kernel boundaries publish between the three launches.  The entry reads nothing back: err stays on the
//                        device for the caller.
//   lm_residue_stats     one pass over the cells, a lane per cell; the lanes of a wave that share a component are merged by cross-lane
//                        adds before one row of twelve 64-bit integer atomics per distinct component goes to memory, as
//                        las_profile_kernel merges per distinct bin.  The cells are sorted by key, so the lanes of a wave mostly share a
//                        component.
#include "common.h"
#include "label_rule.h"

#include <cmath>
#include <type_traits>

namespace {

constexpr int PER = 4;                   // points per lane of residue_keys_kernel, as label_points_kernel
constexpr int CHUNK = 256 * PER;
constexpr int MAX_SIDE = 1 << 20;        // nx, ny: a cell index stays exact in f32
constexpr long MAX_OCCUPIED = 1L << 22;  // cells of one statistics call: sum cx^2 < 2^22 * 2^40 = 2^62
constexpr float MAX_REACH = 16.f;

struct ResDev {
    float clear2, inv;
    int nx, ny;
};

// grid: ceil(N / 1024) workgroups.  LOCAL: I.min_inten is the paint table's thr_min, the search also yields the winner's segment and t, and
// a return below its row's threshold (table_pass, label_rule.h) is no residue, like one below min_intensity; T is the last argument.
struct NoTable {};
template <bool LOCAL>
__global__ __launch_bounds__(256) void residue_keys_kernel(const lab_f32x4* __restrict__ pts, long N, IndexDev I, ResDev R,
                                                           long long* __restrict__ key, int* __restrict__ iq,
                                                           std::conditional_t<LOCAL, TableDev, NoTable> T) {
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
        if constexpr (LOCAL) {
            if (__ballot(b > a)) {
                int s;
                float t;
                ln = label_search_t<true>(p[j], I, a, b, best, s, t);
                if (ln > 0 && !table_pass(T, p[j].w, ln, s, t)) ln = 0;
            }
        } else {
            if (__ballot(b > a)) ln = label_search(p[j], I, a, b, best);   // wave-uniform: a wave beside the lines leaves here
        }
        long long k = -1;
        int q = 0;
        if (ln > 0 && best > R.clear2) {
            const int cx = (int)((p[j].x - I.x0) * R.inv), cy = (int)((p[j].y - I.y0) * R.inv);
            if (cx >= 0 && cx < R.nx && cy >= 0 && cy < R.ny) {            // (holds for the host's nx, ny: they cover the index grid's box)
                k = (long long)cy * R.nx + cx;
                q = (int)(unsigned)fminf(fmaxf(rintf(p[j].w), 0.f), 65535.f);
            }
        }
        if (valid) {
            key[first + i] = k;
            if (iq) iq[first + i] = q;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- components
__device__ __forceinline__ int parent_load(int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x: at most `cap` links (parent[x] <= x, so the chase descends strictly); -1 and err[0] = 1 when the cap runs out
__device__ __forceinline__ int chase(int* parent, int x, long cap, int* err) {
    for (long it = 0; it <= cap; ++it) {
        const int p = parent_load(parent, x);
        if (p == x) return x;
        x = p;
    }
    atomicOr(err, 1);
    return -1;
}

// join the trees of a and b: find both roots, order them, hook the larger under the smaller with atomicMin; where the larger was no root
// any more (old != a) go on with what it pointed to.  Every retry lowers the larger index: at most 2 M of them.
__device__ __forceinline__ void unite(int* parent, int a, int b, long M, int* err) {
    for (long tries = 0; tries <= 2 * M; ++tries) {
        a = chase(parent, a, M, err);
        b = chase(parent, b, M, err);
        if (a < 0 || b < 0 || a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(parent + a, b);                          // (device scope)
        if (old == a) return;                                              // a was a root and now hangs under b
        a = old;                                                           // a hung under old < a already: join old and b
    }
    atomicOr(err, 1);
}

// the index in keys[0, hi) that holds k, or -1: at most 32 halvings whatever keys holds
__device__ __forceinline__ int find_key(const long long* __restrict__ keys, int hi, long long k) {
    int lo = 0;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid: ceil(M / 256)
__global__ __launch_bounds__(256) void components_init_kernel(int* __restrict__ parent, int M) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m < M) parent[m] = (int)m;
}

// grid: ceil(M / 256); a lane per cell
__global__ __launch_bounds__(256) void components_union_kernel(const long long* __restrict__ keys, int M, int nx, int ny, int eight, int* parent,
                                                               int* err) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const long long k = keys[m];
    if (k < 0 || k >= (long long)nx * ny) return;                          // (not a key of this grid: joined with nothing)
    const int cx = (int)(k % nx), cy = (int)(k / nx);
    // the neighbours with a smaller key: W; then SW, S, SE of the row below (4-connectivity: W and S)
    const int count = eight ? 4 : 2;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (n >= count) break;
        const int x = cx + (n == 0 || n == 2 ? -1 : n == 3 ? 1 : 0), y = cy - (n == 0 ? 0 : 1);
        if (x < 0 || x >= nx || y < 0) continue;                           // neighbourhood is tested on (cx, cy), not on the key
        const long long want = (long long)y * nx + x;
        const int j = find_key(keys, (int)m, want);                        // in [0, m]
        if (j < (int)m && keys[j] == want) unite(parent, (int)m, j, M, err);
    }
}

// grid: ceil(M / 256); every lane writes its own entry only, and whatever another lane reads of it - the old parent or the root - is an
// ancestor of the cell
__global__ __launch_bounds__(256) void components_compress_kernel(int* parent, int M, int* err) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int r = chase(parent, (int)m, M, err);
    if (r >= 0) __hip_atomic_store(parent + m, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// grid: ceil(K * 12 / 256)
__global__ __launch_bounds__(256) void stats_init_kernel(long long* __restrict__ stats, long words) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < words) {
        const int c = (int)(i % 12);
        stats[i] = c < 8 ? 0LL : (c == 8 || c == 10) ? 2147483647LL : -2147483648LL;
    }
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// grid: ceil(M / 256); a lane per cell.  comp and keys are device tables the host cannot see: a component outside [0, K) or a key outside
// the grid contributes nothing, so stats is never written outside [0, K).
__global__ __launch_bounds__(256) void residue_stats_kernel(const int* __restrict__ comp, const long long* __restrict__ keys, int nx, int ny,
                                                            const long long* __restrict__ cell_points, const long long* __restrict__ cell_iq,
                                                            int M, int K, long long* __restrict__ stats) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)__lane_id();
    int c = -1, cx = 0, cy = 0;
    long long np = 0, si = 0;
    if (m < M) {
        const long long k = keys[m];
        const int cc = comp[m];
        if (cc >= 0 && cc < K && k >= 0 && k < (long long)nx * ny) {
            c = cc, cx = (int)(k % nx), cy = (int)(k / nx);
            np = cell_points[m], si = cell_iq[m];
        }
    }
    unsigned long long todo = __ballot(c >= 0);
    while (todo) {                                                         // per distinct component of the wave
        const int leader = __ffsll(todo) - 1;
        const int lc = __shfl(c, leader);
        const bool mine = c == lc;
        const unsigned long long mask = __ballot(mine);
        long long v[8];
        int x0, x1, y0, y1;
        if (__popcll(mask) == 1) {                                         // one lane alone: its values, read off the leader
            const int lx = __shfl(cx, leader), ly = __shfl(cy, leader);
            v[0] = 1, v[1] = __shfl(np, leader), v[2] = __shfl(si, leader), v[3] = lx, v[4] = ly;
            v[5] = (long long)lx * lx, v[6] = (long long)lx * ly, v[7] = (long long)ly * ly;
            x0 = x1 = lx, y0 = y1 = ly;
        } else {
            const long long X = mine ? cx : 0, Y = mine ? cy : 0;
            v[0] = __popcll(mask);
            v[1] = wave_sum(mine ? np : 0), v[2] = wave_sum(mine ? si : 0);
            v[3] = wave_sum(X), v[4] = wave_sum(Y);
            v[5] = wave_sum(X * X), v[6] = wave_sum(X * Y), v[7] = wave_sum(Y * Y);
            x0 = mine ? cx : 2147483647, x1 = mine ? cx : (-2147483647 - 1);
            y0 = mine ? cy : 2147483647, y1 = mine ? cy : (-2147483647 - 1);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const int a0 = __shfl_xor(x0, d), a1 = __shfl_xor(x1, d), b0 = __shfl_xor(y0, d), b1 = __shfl_xor(y1, d);
                x0 = a0 < x0 ? a0 : x0, x1 = a1 > x1 ? a1 : x1, y0 = b0 < y0 ? b0 : y0, y1 = b1 > y1 ? b1 : y1;
            }
        }
        long long* row = stats + (long)lc * 12;
        if (lane < 8) {
            long long add = v[0];
#pragma unroll
            for (int q = 1; q < 8; ++q) add = lane == q ? v[q] : add;
            atomicAdd(reinterpret_cast<unsigned long long*>(row) + lane, (unsigned long long)add);
        } else if (lane == 8) {
            atomicMin(row + 8, (long long)x0);
        } else if (lane == 9) {
            atomicMax(row + 9, (long long)x1);
        } else if (lane == 10) {
            atomicMin(row + 10, (long long)y0);
        } else if (lane == 11) {
            atomicMax(row + 11, (long long)y1);
        }
        todo &= ~mask;
    }
}

int check_side(const char* who, int nx, int ny) {
    LM_REQUIRE(nx >= 0 && nx <= MAX_SIDE, "%s: nx=%d cells, at most 2^20 are supported (choose a larger cell)", who, nx);
    LM_REQUIRE(ny >= 0 && ny <= MAX_SIDE, "%s: ny=%d cells, at most 2^20 are supported (choose a larger cell)", who, ny);
    return LM_OK;
}

}  // namespace

namespace {

// The two key entries.  LOCAL: `table` (the paint table of L lines, checked after everything the scalar entry refuses) takes the place
// of min_intensity.
template <bool LOCAL>
int residue_keys(const char* who, void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                 const int* cell_start, const int* cell_segs, float half_width, float z_tol, float min_intensity, const LmPaintTable* table,
                 int L, float clear, double cell, int nx, int ny, long* key, int* iq) {
    IndexDev I;
    if (int e = check_index(who, grid, S, segments, cell_start, cell_segs, half_width, z_tol, I)) return e;
    LM_REQUIRE(half_width <= MAX_REACH, "%s: half_width=%g (the reach), at most %g m is supported", who, (double)half_width, (double)MAX_REACH);
    LM_REQUIRE(LOCAL || std::fabs(min_intensity) < INFINITY, "%s: min_intensity=%g must be a finite number (without one the whole road is one blob)",
               who, (double)min_intensity);
    LM_REQUIRE(clear >= 0.f && clear < half_width, "%s: clear=%g must lie in 0 <= clear < half_width=%g (the reach)", who, (double)clear,
               (double)half_width);
    LM_REQUIRE(cell > 0 && cell < HUGE_VAL, "%s: cell=%g must be a finite size > 0", who, cell);
    if (int e = check_side(who, nx, ny)) return e;
    LM_REQUIRE(S == 0 || (nx >= 1 && ny >= 1), "%s: nx=%d, ny=%d: a grid of at least one cell is needed", who, nx, ny);
    LM_REQUIRE(N >= 0 && N <= 2147483647L, "%s: N=%ld points, at most 2^31 - 1 are supported", who, N);
    LM_REQUIRE(N == 0 || (points_xyzi && key), "%s: null pointer (points_xyzi, key)", who);
    LM_REQUIRE(((uintptr_t)points_xyzi & 15) == 0, "%s: points_xyzi is not 16-byte aligned", who);
    LM_REQUIRE(((uintptr_t)key & 7) == 0, "%s: key is not 8-byte aligned", who);
    LM_REQUIRE(((uintptr_t)iq & 3) == 0, "%s: iq is not 4-byte aligned", who);
    I.min_inten = min_intensity;
    std::conditional_t<LOCAL, TableDev, NoTable> T{};
    if constexpr (LOCAL) {
        LM_REQUIRE(S == 0 || (grid->min_line >= 1 && grid->max_line <= L), "%s: segments carry lines %d .. %d, outside 1 .. L=%d", who,
                   S ? grid->min_line : 0, S ? grid->max_line : 0, L);
        if (int e = check_table(who, table, L, S, true, false, T)) return e;
        I.min_inten = table->thr_min;
    }
    if (N == 0) return LM_OK;
    const ResDev R{clear * clear, (float)(1.0 / cell), nx, ny};
    hipLaunchKernelGGL(residue_keys_kernel<LOCAL>, dim3((unsigned)lm_cdivl(N, CHUNK)), dim3(256), 0, (hipStream_t)hip_stream,
                       reinterpret_cast<const lab_f32x4*>(points_xyzi), N, I, R, reinterpret_cast<long long*>(key), iq, T);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

}  // namespace

// points_xyzi: DEVICE [N][4] f32; the index arguments of lm_label_points, half_width = the reach the grid was built for.  key [N] int64,
// iq [N] int32 or NULL.  Asynchronous, no workspace, nothing read back.
LM_API int lm_residue_keys(void* hip_stream, const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                           const int* cell_start, const int* cell_segs, float half_width, float z_tol, float min_intensity, float clear,
                           double cell, int nx, int ny, long* key, int* iq) {
    return residue_keys<false>("residue_keys", hip_stream, points_xyzi, N, segments, S, grid, cell_start, cell_segs, half_width, z_tol,
                               min_intensity, nullptr, 0, clear, cell, nx, ny, key, iq);
}

// as above with the paint table of L lines (the rule: include/lanemap_hip.h) in place of min_intensity; the stream comes LAST.
LM_API int lm_residue_keys_local(const float* points_xyzi, long N, const float* segments, long S, const LmLineGrid* grid,
                                 const int* cell_start, const int* cell_segs, float half_width, float z_tol, const LmPaintTable* table, int L,
                                 float clear, double cell, int nx, int ny, long* key, int* iq, void* hip_stream) {
    return residue_keys<true>("residue_keys_local", hip_stream, points_xyzi, N, segments, S, grid, cell_start, cell_segs, half_width, z_tol,
                              NAN, table, L, clear, cell, nx, ny, key, iq);
}

// keys: DEVICE [M] int64, ascending and distinct (what the host cannot check: anything else gives garbage inside root[0, M)); root DEVICE
// [M] int32; err DEVICE [1] int32, zeroed by the call on the stream, non-zero afterwards when a loop cap ran out.  Asynchronous.
LM_API int lm_cell_components(void* hip_stream, const long* keys, long M, int nx, int ny, int connectivity, int* root, int* err) {
    if (int e = check_side("cell_components", nx, ny)) return e;
    LM_REQUIRE(connectivity == 4 || connectivity == 8, "cell_components: connectivity=%d is neither 4 nor 8", connectivity);
    LM_REQUIRE(M >= 0 && M <= 2147483647L / 2, "cell_components: M=%ld cells, at most 2^30 - 1 are supported", M);
    LM_REQUIRE(err && (M == 0 || (keys && root)), "cell_components: null pointer (keys, root, err)");
    LM_REQUIRE(((uintptr_t)keys & 7) == 0, "cell_components: keys is not 8-byte aligned");
    LM_REQUIRE(((uintptr_t)root & 3) == 0, "cell_components: root is not 4-byte aligned");
    LM_REQUIRE(((uintptr_t)err & 3) == 0, "cell_components: err is not 4-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    LM_HIP(lm_zero_async(err, sizeof(int), s));
    if (M == 0) return LM_OK;
    const dim3 groups((unsigned)lm_cdivl(M, 256));
    hipLaunchKernelGGL(components_init_kernel, groups, dim3(256), 0, s, root, (int)M);
    LM_LAUNCH_CHECK();
    hipLaunchKernelGGL(components_union_kernel, groups, dim3(256), 0, s, reinterpret_cast<const long long*>(keys), (int)M, nx, ny,
                       connectivity == 8 ? 1 : 0, root, err);
    LM_LAUNCH_CHECK();
    hipLaunchKernelGGL(components_compress_kernel, groups, dim3(256), 0, s, root, (int)M, err);
    LM_LAUNCH_CHECK();
    return LM_OK;
}

// comp DEVICE [M] int32 (dense component ids 0 .. K-1), keys DEVICE [M] int64 with the grid's nx, ny, cell_points and cell_iq DEVICE [M]
// int64; stats DEVICE [K][12] int64, initialised by the call on the stream.  Asynchronous, no workspace, nothing read back.
LM_API int lm_residue_stats(void* hip_stream, const int* comp, const long* keys, int nx, int ny, const long* cell_points, const long* cell_iq,
                            long M, long K, long* stats) {
    if (int e = check_side("residue_stats", nx, ny)) return e;
    LM_REQUIRE(M >= 0 && M <= MAX_OCCUPIED, "residue_stats: M=%ld occupied cells, at most 2^22 are supported (the sums of squares stay in 64 bits)", M);
    LM_REQUIRE(K >= 0 && K <= M, "residue_stats: K=%ld components of M=%ld cells", K, M);
    LM_REQUIRE(M == 0 || (comp && keys && cell_points && cell_iq), "residue_stats: null pointer (comp, keys, cell_points, cell_iq)");
    LM_REQUIRE(K == 0 || stats, "residue_stats: null pointer (stats)");
    LM_REQUIRE(((uintptr_t)comp & 3) == 0, "residue_stats: comp is not 4-byte aligned");
    LM_REQUIRE(((uintptr_t)keys & 7) == 0, "residue_stats: keys is not 8-byte aligned");
    LM_REQUIRE(((uintptr_t)cell_points & 7) == 0, "residue_stats: cell_points is not 8-byte aligned");
    LM_REQUIRE(((uintptr_t)cell_iq & 7) == 0, "residue_stats: cell_iq is not 8-byte aligned");
    LM_REQUIRE(((uintptr_t)stats & 7) == 0, "residue_stats: stats is not 8-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    if (K == 0) return LM_OK;
    const long words = K * 12;
    hipLaunchKernelGGL(stats_init_kernel, dim3((unsigned)lm_cdivl(words, 256)), dim3(256), 0, s, reinterpret_cast<long long*>(stats), words);
    LM_LAUNCH_CHECK();
    hipLaunchKernelGGL(residue_stats_kernel, dim3((unsigned)lm_cdivl(M, 256)), dim3(256), 0, s, comp, reinterpret_cast<const long long*>(keys), nx, ny,
                       reinterpret_cast<const long long*>(cell_points), reinterpret_cast<const long long*>(cell_iq), (int)M, (int)K,
                       reinterpret_cast<long long*>(stats));
    LM_LAUNCH_CHECK();
    return LM_OK;
}
