// Gap fill of sparse BEV tiles: the stage between the rasteriser and the network for scanners that deliver fewer returns than pixels.
// A tile is u8 [H][W][3]; a pixel is EMPTY when its three bytes are 0 (the reference's rule R + G + B < 1); its VALUE is R << 16 | G << 8 | B.
//   gap   of an empty pixel p for a maximal radius Rmax: the smallest d2 = dr^2 + dc^2 over the non-empty pixels q of the same tile with
//         d2 <= Rmax^2 (a disc; pixels outside the tile do not exist).  No such q: p is FAR.
//   ring  k of an empty, non-far pixel: the smallest integer with k^2 >= gap.
//   hist  [b][0] the non-empty pixels, [b][k], k = 1..Rmax, the empty pixels of ring k, [b][Rmax + 1] the far ones: u32, a row sums to H W.
//   fill  with radius r (per tile): a non-empty pixel keeps its bytes; an empty pixel with gap <= r^2 takes the bytes of the q of smallest d2
//         within the disc of radius r, ties in d2 to the LARGEST value (brightest, then highest: the rule by which the rasteriser settles a
//         pixel); every other pixel stays empty.  Sources are pixels of the input: no cascading.  r = 0 is a copy.
// One template serves both entries, so the search cannot differ between them.  A workgroup of 256 lanes owns a block of GW x GH = 64 x 32
// pixels of one tile and stages it with a halo of R pixels (R = Rmax, or the tile's r) in LDS:
//   (1) raw     every staged row is a byte range of the tile; its 4-byte aligned inside is read as coalesced dwords, the up to 3 head and 3
//               tail bytes as bytes (3 W is not a multiple of 4 for odd W, and the tile base is unaligned then): nothing outside the
//               range is read.  The dwords land in LDS at the row's own alignment.
//   (2) values  one 32-bit value per staged pixel (0 outside the tile), pitch GP = 80, so that lane l of a wave reads dword l + const.
//   (3) search  a wave owns a block row; every lane walks TAB, the disc's offsets sorted by d2 (196 at R = 8, the centre left out), class by
//               class (a class = one d2, 29 up to 64): it takes the maximum over the class and settles at the first class that gave one.
//               TAB is a compile-time table and the walk is unrolled, so every offset is the immediate of an LDS read; it is wave uniform
//               - settled and non-empty lanes read along - and ends when no lane of the wave is open or the next d2 exceeds R^2.  A block
//               whose staged area holds no non-empty pixel, or whose own pixels hold no empty one, skips the walk.
//   (4) hist    categories are counted per wave with ballots, added to Rmax + 2 LDS counters, then one global integer atomicAdd per
//               non-zero counter: order independent, the same bits every run.
//       fill    the three bytes go to LDS at the output row's alignment; the rows leave as dwords with head and tail bytes, like (1).
// Integers only.  HBM traffic per tile: 3 H W read (plus the halo, from L2) per entry, 3 H W written by the fill.
#include "common.h"

namespace {

constexpr int GT = 256;                      // threads per workgroup
constexpr int GW = 64, GH = 32;              // pixels of a block: one wave per block row, 8 rows per wave
constexpr int MAX_R = 8;
constexpr int GP = GW + 2 * MAX_R;           // pitch of the value image (dwords)
constexpr int GS = GH + 2 * MAX_R;           // its rows
constexpr int RAWP = 64;                     // dwords per raw row: 3 GP + 3 bytes of alignment = 243 bytes at most
constexpr int MAX_B = 4096;
constexpr int MAX_HW = 32768;
constexpr int ZCHUNK = 256;                  // tiles per launch: their radii travel as 4-bit fields of a kernel argument
constexpr int NTAB = 196;                    // lattice points with 0 < d2 <= 64

struct GapTable {
    short off[NTAB];                         // (dr + MAX_R) * GP + dc + MAX_R: from the top left corner of the largest window
    short first[MAX_R * MAX_R + 2];          // class k holds the entries first[k] .. first[k + 1] - 1
    unsigned char d2[MAX_R * MAX_R + 1];     // its d2, ascending
    unsigned char ring[MAX_R * MAX_R + 1];   // smallest r with r^2 >= its d2
    int classes;
};

constexpr GapTable make_table() {
    GapTable t{};
    int n = 0, k = 0;
    for (int d2 = 1; d2 <= MAX_R * MAX_R; ++d2) {
        const int n0 = n;
        for (int dr = -MAX_R; dr <= MAX_R; ++dr)
            for (int dc = -MAX_R; dc <= MAX_R; ++dc)
                if (dr * dr + dc * dc == d2) t.off[n++] = (short)((dr + MAX_R) * GP + dc + MAX_R);
        if (n == n0) continue;               // not a sum of two squares
        int r = 0;
        while (r * r < d2) ++r;
        t.first[k] = (short)n0, t.d2[k] = (unsigned char)d2, t.ring[k] = (unsigned char)r;
        ++k;
    }
    t.first[k] = (short)n;
    t.classes = k;
    return t;
}

constexpr GapTable TAB = make_table();
static_assert(TAB.first[TAB.classes] == NTAB, "the disc of radius 8 has 196 lattice points beside its centre");

struct Radii {
    unsigned w[ZCHUNK / 8];                  // radius of tile z of the launch: (w[z / 8] >> 4 (z % 8)) & 15
};

// grid (ceil(W / GW), ceil(H / GH), tiles of the launch).  HIST: hist [B][hist_ld] is added to (zeroed before); else out is written.
template <bool HIST>
__global__ __launch_bounds__(GT) void gap_kernel(const unsigned char* __restrict__ tiles, int b0, int H, int W, Radii radii,
                                                 unsigned* __restrict__ hist, int hist_ld, unsigned char* __restrict__ out) {
    __shared__ unsigned raw[GS * RAWP];
    __shared__ unsigned val[GS * GP];
    __shared__ unsigned cnt[MAX_R + 2];
    __shared__ int flag_full, flag_hole;     // a staged pixel is non-empty / an own pixel is empty
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int z = blockIdx.z, b = b0 + z;
    const int R = (int)((radii.w[z >> 3] >> (4 * (z & 7))) & 15u);
    const int x0 = blockIdx.x * GW, y0 = blockIdx.y * GH;
    const int SH = GH + 2 * R, SP = GW + 2 * R;
    const int D = MAX_R - R;                                               // the value image keeps the origin of the largest halo
    const size_t row_bytes = (size_t)3 * (size_t)W;
    const unsigned char* tile = tiles + (size_t)b * (size_t)H * row_bytes;
    // staged columns that exist: [cx0, cx1)
    const int cx0 = x0 - R > 0 ? x0 - R : 0, cx1 = x0 + GW + R < W ? x0 + GW + R : W;
    if (tid < MAX_R + 2) cnt[tid] = 0;
    if (tid == 0) flag_full = 0, flag_hole = 0;
    // (1) raw rows
    for (int j = wv; j < SH; j += GT / 64) {
        const int gy = y0 - R + j;
        if (gy < 0 || gy >= H) continue;                                   // wave uniform
        const unsigned char* g0 = tile + (size_t)gy * row_bytes + (size_t)(3 * cx0);
        const unsigned char* g1 = g0 + 3 * (cx1 - cx0);
        const unsigned char* p = g0 - ((uintptr_t)g0 & 3) + 4 * lane;      // lane's aligned dword; 61 dwords cover the widest row
        if (p < g1) {
            unsigned v = 0;
            if (p >= g0 && p + 4 <= g1) {
                v = *reinterpret_cast<const unsigned*>(p);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (p + k >= g0 && p + k < g1) v |= (unsigned)p[k] << (8 * k);
            }
            raw[j * RAWP + lane] = v;
        }
    }
    __syncthreads();
    // (2) values
    const unsigned char* rawb = reinterpret_cast<const unsigned char*>(raw);
    for (int j = wv; j < SH; j += GT / 64) {
        const int gy = y0 - R + j;
        const bool row_ok = gy >= 0 && gy < H;
        const int shift = row_ok ? (int)((uintptr_t)(tile + (size_t)gy * row_bytes + (size_t)(3 * cx0)) & 3) : 0;
        const bool own_row = j >= R && j < R + GH;
        for (int c = lane; c < SP; c += 64) {
            const int gx = x0 - R + c;
            unsigned v = 0;
            const bool in = row_ok && gx >= 0 && gx < W;
            if (in) {
                const unsigned char* q = rawb + j * (RAWP * 4) + shift + 3 * (gx - cx0);
                v = (unsigned)q[0] << 16 | (unsigned)q[1] << 8 | (unsigned)q[2];
            }
            val[(j + D) * GP + c + D] = v;
            if (v) flag_full = 1;
            if (in && v == 0 && own_row && c >= R && c < R + GW) flag_hole = 1;
        }
    }
    __syncthreads();
    // the largest d2 to look at; workgroup uniform
    const int rr = __builtin_amdgcn_readfirstlane(flag_full != 0 && flag_hole != 0 ? R * R : 0);
    unsigned wc[MAX_R + 2];
#pragma unroll
    for (int k = 0; k < MAX_R + 2; ++k) wc[k] = 0;
    unsigned char* outb = reinterpret_cast<unsigned char*>(raw);           // (4) reuses the raw rows: their last reader is behind the barrier
    // (3) search
    for (int i = wv; i < GH; i += GT / 64) {
        const int gy = y0 + i, gx = x0 + lane;
        if (gy >= H) break;                                                // wave uniform
        const bool inside = gx < W;
        const int corner = i * GP + lane;                                  // top left of the largest window around the pixel
        const unsigned v = val[corner + MAX_R * GP + MAX_R];
        bool open = inside && v == 0;
        unsigned best = 0;
        int ring = 0;
#pragma unroll
        for (int k = 0; k < TAB.classes; ++k) {                            // unrolled: every offset is an immediate of its LDS read
            if ((int)TAB.d2[k] > rr || __ballot(open) == 0ull) break;      // wave uniform
            unsigned m = 0;
#pragma unroll
            for (int e = TAB.first[k]; e < TAB.first[k + 1]; ++e) {
                const unsigned q = val[corner + TAB.off[e]];
                m = q > m ? q : m;
            }
            if (open && m) best = m, ring = TAB.ring[k], open = false;
        }
        if (HIST) {
            const int cat = !inside ? -1 : v ? 0 : best ? ring : R + 1;
#pragma unroll
            for (int k = 0; k < MAX_R + 2; ++k)
                if (k <= R + 1) wc[k] += (unsigned)__popcll(__ballot(cat == k));
        } else if (inside) {
            const unsigned res = v | best;                                 // best is 0 for a non-empty pixel
            const int oshift = (int)((uintptr_t)(out + ((size_t)b * (size_t)H + (size_t)gy) * row_bytes + (size_t)(3 * x0)) & 3);
            unsigned char* q = outb + i * (RAWP * 4) + oshift + 3 * lane;
            q[0] = (unsigned char)(res >> 16), q[1] = (unsigned char)(res >> 8), q[2] = (unsigned char)res;
        }
    }
    if (HIST) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < MAX_R + 2; ++k)
                if (k <= R + 1 && wc[k]) atomicAdd(&cnt[k], wc[k]);
        }
        __syncthreads();
        if (tid <= R + 1 && cnt[tid]) atomicAdd(hist + (size_t)b * (size_t)hist_ld + tid, cnt[tid]);
        return;
    }
    __syncthreads();
    // (4) the filled rows leave as they came
    const int own_w = W - x0 < GW ? W - x0 : GW;
    for (int i = wv; i < GH; i += GT / 64) {
        const int gy = y0 + i;
        if (gy >= H) break;
        unsigned char* g0 = out + ((size_t)b * (size_t)H + (size_t)gy) * row_bytes + (size_t)(3 * x0);
        unsigned char* g1 = g0 + 3 * own_w;
        unsigned char* p = g0 - ((uintptr_t)g0 & 3) + 4 * lane;            // 49 dwords cover the widest row
        if (p < g1) {
            const unsigned v = raw[i * RAWP + lane];
            if (p >= g0 && p + 4 <= g1) {
                *reinterpret_cast<unsigned*>(p) = v;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (p + k >= g0 && p + k < g1) p[k] = (unsigned char)(v >> (8 * k));
            }
        }
    }
}

template <bool HIST>
int launch(hipStream_t s, const unsigned char* tiles, int B, int H, int W, const int* radius, int fixed_radius, unsigned* hist, int hist_ld,
           unsigned char* out) {
    for (int b0 = 0; b0 < B; b0 += ZCHUNK) {
        const int nz = B - b0 < ZCHUNK ? B - b0 : ZCHUNK;
        Radii rd{};
        for (int z = 0; z < nz; ++z) rd.w[z >> 3] |= (unsigned)(radius ? radius[b0 + z] : fixed_radius) << (4 * (z & 7));
        hipLaunchKernelGGL(gap_kernel<HIST>, dim3((unsigned)lm_cdiv(W, GW), (unsigned)lm_cdiv(H, GH), (unsigned)nz), dim3(GT), 0, s, tiles, b0, H,
                           W, rd, hist, hist_ld, out);
        LM_LAUNCH_CHECK();
    }
    return LM_OK;
}

int check_tiles(const char* who, const void* tiles, int B, int H, int W) {
    LM_REQUIRE(B >= 1 && B <= MAX_B, "%s: B=%d tiles, 1 to %d are supported", who, B, MAX_B);
    LM_REQUIRE(H >= 1 && H <= MAX_HW, "%s: H=%d, 1 to %d are supported", who, H, MAX_HW);
    LM_REQUIRE(W >= 1 && W <= MAX_HW, "%s: W=%d, 1 to %d are supported", who, W, MAX_HW);
    LM_REQUIRE(tiles, "%s: null pointer (tiles_hwc_u8)", who);
    return LM_OK;
}

}  // namespace

// tiles: DEVICE u8 [B][H][W][3]; hist: DEVICE u32 [B][max_radius_px + 2], zeroed here on the stream.  Asynchronous, no read-back.
LM_API int lm_tile_gap_hist(void* hip_stream, const unsigned char* tiles_hwc_u8, int B, int H, int W, int max_radius_px, unsigned* hist) {
    if (int e = check_tiles("tile_gap_hist", tiles_hwc_u8, B, H, W)) return e;
    LM_REQUIRE(max_radius_px >= 1 && max_radius_px <= MAX_R, "tile_gap_hist: max_radius_px=%d, 1 to %d are supported", max_radius_px, MAX_R);
    LM_REQUIRE(hist, "tile_gap_hist: null pointer (hist)");
    hipStream_t s = (hipStream_t)hip_stream;
    LM_HIP(lm_zero_async(hist, (size_t)B * (size_t)(max_radius_px + 2) * sizeof(unsigned), s));
    return launch<true>(s, tiles_hwc_u8, B, H, W, nullptr, max_radius_px, hist, max_radius_px + 2, nullptr);
}

// radius_px: HOST [B]; out: DEVICE u8 [B][H][W][3], a buffer of its own.  Asynchronous, no read-back.
LM_API int lm_tile_gap_fill(void* hip_stream, const unsigned char* tiles_hwc_u8, int B, int H, int W, const int* radius_px,
                            unsigned char* out_hwc_u8) {
    if (int e = check_tiles("tile_gap_fill", tiles_hwc_u8, B, H, W)) return e;
    LM_REQUIRE(radius_px && out_hwc_u8, "tile_gap_fill: null pointer (radius_px / out_hwc_u8)");
    for (int b = 0; b < B; ++b)
        LM_REQUIRE(radius_px[b] >= 0 && radius_px[b] <= MAX_R, "tile_gap_fill: radius_px[%d]=%d, 0 to %d are supported", b, radius_px[b], MAX_R);
    const size_t bytes = (size_t)B * (size_t)H * (size_t)W * 3;
    const uintptr_t a = (uintptr_t)tiles_hwc_u8, o = (uintptr_t)out_hwc_u8;
    LM_REQUIRE(o + bytes <= a || a + bytes <= o, "tile_gap_fill: out_hwc_u8 overlaps tiles_hwc_u8 (sources are pixels of the input: the output is a buffer of its own)");
    return launch<false>((hipStream_t)hip_stream, tiles_hwc_u8, B, H, W, radius_px, 0, nullptr, 0, out_hwc_u8);
}
