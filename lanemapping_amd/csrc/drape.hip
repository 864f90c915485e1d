// Vertex heights read off the points: a pixel-scale ground model around the polyline vertices of every tile.  Input is the (points,
// tile_offsets, params) triple lm_bev_raster_batch takes plus, per tile, a list of vertex pixels (vr, vc), walked with the scaffold of
// tile_points.h (tile constants, workgroup -> tile, streaming loop, key of a height, host prologue).  Membership is the rule of
// ground.hip: a point counts for tile b exactly when raster.hip would keep it for b and its tile-frame height vz is finite.
// With R = radius_px and S = (2R + 1)^2:
//   (a) window minima  vertex v owns S slots; slot (i, j), i, j in -R..R, holds the smallest lm_key_of(vz) (-0.0 < +0.0, 0xFFFFFFFF =
//                      empty) over the tile's points of pixel (vr + i, vc + j).  A workgroup streams one chunk of DCHUNK = 16,384
//                      points of one tile (lm_stream_points: 256 lanes x 64 loads, 8 in flight per lane) and keeps the tile's vertices
//                      in LDS as a row-band index: the entries (vr, vc, vertex id) sorted by band = vr / 8 (the head's row pitch)
//                      and the first entry of every band.  The host sorts (stable); the
//                      workgroup derives the band starts from the sorted entries while it copies them.  A point of row r walks the
//                      entries of bands (r - R) / 8 .. (r + R) / 8, one contiguous range, and sends its key with an integer atomic min
//                      straight to the slot in global memory for every vertex with |r - vr| <= R and |c - vc| <= R: one point serves
//                      every window that holds its pixel (overlapping windows, duplicate vertices).  Slots are memset to 0xFF and only
//                      ever lowered by atomic min: order independent, the same bits every run.
//   (b) median         one wave per vertex: z = the lower median (element (k - 1) / 2 of the k non-empty slots in ascending key order,
//                      by rank counting with ties ranked by position), npix = k, z = NaN for k = 0.
// Tiles without points or without vertices get no workgroup.  HBM traffic of (a): 16 N read.
#include "common.h"
#include "tile_points.h"

#include <cmath>
#include <vector>

namespace {

constexpr int DT = 256;                      // threads per workgroup, both kernels
constexpr int D_PER_THREAD = 64;
constexpr int DCHUNK = DT * D_PER_THREAD;    // points per workgroup of (a)
constexpr int LB = 8;                        // loads in flight per lane
constexpr int BAND = 8;                      // rows per band of the vertex index
constexpr int MAX_R = 8;
constexpr int MAX_SLOTS = (2 * MAX_R + 1) * (2 * MAX_R + 1);
constexpr int MAX_TILE_VERTICES = 16384;     // 128 KB of LDS entries
constexpr int MAX_HW = 32768;                // vr and vc are packed into 16 bits each; at most 4097 band starts (16 KB of LDS)

struct DrapeTile : LmTileRange {
    int vbase, nv;                           // vertex range of the tile
};
static_assert(sizeof(DrapeTile) == 96 && alignof(DrapeTile) == 16, "96 bytes per tile: lm_drape_workspace_bytes");

struct DrapeEntry {
    unsigned rc;                             // vr << 16 | vc
    unsigned id;                             // index of the vertex in the call's concatenated list
};

// (a) grid: sum over the tiles with vertices of ceil(count / DCHUNK); dynamic LDS = nb1 band starts (nb1 = bands + 1 rounded up to even)
// + the entries of the largest tile
__global__ __launch_bounds__(DT) void drape_min_kernel(const f32x4* __restrict__ pts, const DrapeTile* __restrict__ tiles, int B,
                                                       const DrapeEntry* __restrict__ entries, unsigned* __restrict__ slots, int H, int W,
                                                       int R, int nb, int nb1) {
    extern __shared__ unsigned lds[];
    unsigned* bstart = lds;                                     // [nb + 1]: first entry of every band, bstart[nb] = nv
    DrapeEntry* ent = reinterpret_cast<DrapeEntry*>(lds + nb1);
    const int tid = threadIdx.x;
    const int t = lm_tile_of(tiles, B, (long)blockIdx.x);
    const DrapeTile X = tiles[t];
    const long first = ((long)blockIdx.x - X.cbase) * DCHUNK;
    const long left = X.count - first;                          // >= 1
    const int nv = X.nv;                                        // >= 1
    const DrapeEntry* src = entries + X.vbase;
    for (int i = tid; i < nv; i += DT) {
        const DrapeEntry e = src[i];
        ent[i] = e;
        const int band = (int)(e.rc >> 16) / BAND;
        const int prev = i ? (int)(src[i - 1].rc >> 16) / BAND : -1;
        for (int b = prev + 1; b <= band; ++b) bstart[b] = (unsigned)i;      // band <= nb - 1: vr < H
        if (i == nv - 1)
            for (int b = band + 1; b <= nb; ++b) bstart[b] = (unsigned)nv;
    }
    __syncthreads();
    const int D = 2 * R + 1;
    const long S = (long)D * D;
    lm_stream_points<DT, D_PER_THREAD, LB>(pts + X.start + first, left, tid, [&](const f32x4 p, bool valid) {
        int row, col;
        float vz;
        if (!(valid && lm_point_window(p, X, H, W, row, col, vz) && fabsf(vz) < INFINITY)) return;
        const unsigned key = lm_key_of(vz);
        const int r0 = row - R > 0 ? row - R : 0, r1 = row + R < H - 1 ? row + R : H - 1;
        const unsigned e1 = bstart[r1 / BAND + 1];
        for (unsigned e = bstart[r0 / BAND]; e < e1; ++e) {
            const DrapeEntry v = ent[e];
            const unsigned di = (unsigned)(row - (int)(v.rc >> 16) + R), dj = (unsigned)(col - (int)(v.rc & 0xFFFFu) + R);
            if (di < (unsigned)D && dj < (unsigned)D) atomicMin(slots + ((long)v.id * S + (long)(di * (unsigned)D + dj)), key);
        }
    });
}

// (b) grid: ceil(V / 4) workgroups, one wave per vertex
__global__ __launch_bounds__(DT) void drape_median_kernel(const unsigned* __restrict__ slots, int V, int S, float* __restrict__ z,
                                                          int* __restrict__ npix, float* __restrict__ pixel_min) {
    __shared__ unsigned keys[DT / 64][MAX_SLOTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long v = (long)blockIdx.x * (DT / 64) + wv;
    unsigned* k = keys[wv];
    if (v < V) {
        for (int e = lane; e < S; e += 64) {
            const unsigned s = slots[v * S + e];
            k[e] = s;
            if (pixel_min) pixel_min[v * S + e] = __uint_as_float(s == LM_KEY_EMPTY ? LM_QNAN_BITS : __float_as_uint(lm_value_of(s)));
        }
    }
    __syncthreads();
    if (v >= V) return;
    int n = 0;
    for (int f = 0; f < S; ++f) n += k[f] != LM_KEY_EMPTY;
    if (n == 0) {
        if (lane == 0) z[v] = __uint_as_float(LM_QNAN_BITS), npix[v] = 0;
        return;
    }
    // the element of rank (n - 1) / 2; equal keys are ranked by their position, so exactly one element has each rank, and the empty
    // slots (the largest key) take the ranks from n on
    const int want = (n - 1) / 2;
    for (int e = lane; e < S; e += 64) {
        const unsigned mine = k[e];
        int rank = 0;
        for (int f = 0; f < S; ++f) rank += (k[f] < mine) || (f < e && k[f] == mine);
        if (rank == want) z[v] = lm_value_of(mine), npix[v] = n;
    }
}

}  // namespace

LM_API long lm_drape_workspace_bytes(long n_vertices, int B, int radius_px) {
    if (n_vertices < 0 || n_vertices > 2147483647L || B < 0 || B > LM_MAX_TILES || radius_px < 0 || radius_px > MAX_R) return 0;
    const long S = (long)(2 * radius_px + 1) * (2 * radius_px + 1);
    return (long)(lm_align256((size_t)(B > 0 ? B : 1) * sizeof(DrapeTile)) + lm_align256((size_t)n_vertices * sizeof(DrapeEntry)) +
                  lm_align256((size_t)n_vertices * (size_t)S * 4));
}

// points: device [sum N][4]; tile_offsets: HOST [B+1]; params: HOST [B]; vertices_rc: HOST [V][2] (row, col); vertex_offsets: HOST [B+1],
// vertex_offsets[0] = 0, V = vertex_offsets[B]; z [V] f32, npix [V] i32, pixel_min [V][(2R+1)^2] f32 or NULL: device.  Asynchronous, but
// copies host memory of this call to the device: refuses a capturing stream (common.h).
LM_API int lm_drape_vertices(void* hip_stream, const float* points_xyzi, const long* tile_offsets, const LmRasterParams* params, int B, int H,
                             int W, const int* vertices_rc, const long* vertex_offsets, int radius_px, void* workspace, long workspace_bytes,
                             float* z, int* npix, float* pixel_min) {
    LM_NO_CAPTURE(hip_stream, "drape_vertices", LM_WHY_HOST_COPY);
    static thread_local std::vector<DrapeTile> h_tiles;
    static thread_local std::vector<DrapeEntry> h_entries;
    static thread_local std::vector<int> h_fill;
    LM_REQUIRE(radius_px >= 0 && radius_px <= MAX_R, "drape_vertices: radius_px=%d, 0 to %d are supported", radius_px, MAX_R);
    LM_REQUIRE(H > 0 && W > 0 && H <= MAX_HW && W <= MAX_HW, "drape_vertices: bad tile size H=%d W=%d (1 to %d)", H, W, MAX_HW);
    const int nb = (int)lm_cdivl(H, BAND);
    int max_nv = 0;
    const auto tile_vertices = [&](int b, DrapeTile& T, long& wgs) -> int {
        if (b == 0) {                                           // behind the shared checks: B is refused by its own name first
            LM_REQUIRE(vertex_offsets, "drape_vertices: null pointer (vertex_offsets)");
            LM_REQUIRE(vertex_offsets[0] == 0, "drape_vertices: vertex_offsets[0] must be 0");
        }
        const long nv = vertex_offsets[b + 1] - vertex_offsets[b];
        LM_REQUIRE(nv >= 0, "drape_vertices: vertex_offsets must be non-decreasing (tile %d)", b);
        LM_REQUIRE(nv <= MAX_TILE_VERTICES, "drape_vertices: %ld vertices in tile %d, at most %d per tile are supported", nv, b,
                   MAX_TILE_VERTICES);
        LM_REQUIRE(vertex_offsets[b + 1] <= 2147483647L, "drape_vertices: more than 2^31 - 1 vertices");
        T.vbase = (int)vertex_offsets[b], T.nv = (int)nv;
        if (nv == 0) wgs = 0;                                   // nothing to find: no workgroup, whatever its points
        if (nv > max_nv) max_nv = (int)nv;
        return LM_OK;
    };
    long wg, N;
    if (int e = lm_tile_ranges("drape_vertices", tile_offsets, params, B, 0, H, W, DCHUNK, h_tiles, &wg, &N, tile_vertices)) return e;
    if (B == 0) return LM_OK;
    const long V = vertex_offsets[B];
    LM_REQUIRE(N <= 2147483647L, "drape_vertices: %ld points, at most 2^31 - 1 are supported", N);
    LM_REQUIRE(wg <= 2147483647L, "drape_vertices: too many workgroups");
    if (V == 0) return LM_OK;
    LM_REQUIRE(vertices_rc, "drape_vertices: null vertices_rc");
    // the row-band index: per tile a stable counting sort of its vertices by band = vr / 8
    h_entries.resize((size_t)V);
    for (int b = 0; b < B; ++b) {
        const long v0 = vertex_offsets[b], v1 = vertex_offsets[b + 1];
        h_fill.assign((size_t)nb + 1, 0);
        for (long v = v0; v < v1; ++v) {
            const int vr = vertices_rc[v * 2], vc = vertices_rc[v * 2 + 1];
            LM_REQUIRE(vr >= 0 && vr < H && vc >= 0 && vc < W, "drape_vertices: vertex %ld (%d, %d) of tile %d lies outside the %dx%d tile",
                       v - v0, vr, vc, b, H, W);
            ++h_fill[(size_t)(vr / BAND) + 1];
        }
        for (int i = 0; i < nb; ++i) h_fill[(size_t)i + 1] += h_fill[(size_t)i];
        for (long v = v0; v < v1; ++v) {
            const int vr = vertices_rc[v * 2], vc = vertices_rc[v * 2 + 1];
            h_entries[(size_t)(v0 + h_fill[(size_t)(vr / BAND)]++)] = DrapeEntry{(unsigned)vr << 16 | (unsigned)vc, (unsigned)v};
        }
    }
    LM_REQUIRE(workspace && z && npix, "drape_vertices: null pointer (workspace / z / npix)");
    if (int e = lm_tile_points_check("drape_vertices", points_xyzi, N, workspace)) return e;
    LM_REQUIRE(lm_drape_workspace_bytes(V, B, radius_px) <= workspace_bytes, "drape_vertices: workspace too small (%ld B needed)",
               lm_drape_workspace_bytes(V, B, radius_px));
    const int D = 2 * radius_px + 1, S = D * D;
    hipStream_t s = (hipStream_t)hip_stream;
    char* w = (char*)workspace;
    DrapeTile* d_tiles = (DrapeTile*)w;
    w += lm_align256((size_t)B * sizeof(DrapeTile));
    DrapeEntry* d_entries = (DrapeEntry*)w;
    w += lm_align256((size_t)V * sizeof(DrapeEntry));
    unsigned* slots = (unsigned*)w;
    LM_HIP(hipMemsetAsync(slots, 0xFF, (size_t)V * (size_t)S * 4, s));
    if (wg > 0) {
        LM_HIP(hipMemcpyAsync(d_tiles, h_tiles.data(), (size_t)B * sizeof(DrapeTile), hipMemcpyHostToDevice, s));
        LM_HIP(hipMemcpyAsync(d_entries, h_entries.data(), (size_t)V * sizeof(DrapeEntry), hipMemcpyHostToDevice, s));
        const int nb1 = (nb + 2) / 2 * 2;                       // nb + 1 band starts, rounded up to keep the entries 8-byte aligned
        const size_t lds = (size_t)nb1 * sizeof(unsigned) + (size_t)max_nv * sizeof(DrapeEntry);
        if (int e = lm_ensure_dynamic_lds((const void*)drape_min_kernel, lds)) return e;
        hipLaunchKernelGGL(drape_min_kernel, dim3((unsigned)wg), dim3(DT), lds, s, reinterpret_cast<const f32x4*>(points_xyzi), d_tiles, B,
                           d_entries, slots, H, W, radius_px, nb, nb1);
        LM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(drape_median_kernel, dim3((unsigned)lm_cdivl(V, DT / 64)), dim3(DT), 0, s, slots, (int)V, S, z, npix, pixel_min);
    LM_LAUNCH_CHECK();
    return LM_OK;
}
