// The LAS point record, shared by the decode (lidar.hip), the labelling (label.hip) and the marking profile (profile.hip).  On the device:
// the decode's arithmetic on one staged record, the selection predicate of lm_las_decode_select, and the staging of 256 records in LDS.
// Sources that include this are built with -ffp-contract=off (build.py EXACT_FP), so the same expression gives the same bits in every
// kernel that uses it.  On the host (below the device part): the checks and conversions their entries run before they launch.
#pragma once
#include "common.h"

#include <map>
#include <mutex>
#include <tuple>

namespace {

struct LasXf {
    double sx, sy, sz, ox, oy, oz;
    float lo, hi;
    int normalise;
};

struct LasSel {
    unsigned cls[8];
    unsigned drop;       // LmLasSelect::drop_flags
    int returns;
    float z_lo, z_hi;
    int fmt6;            // point formats 6-10
};

// The arithmetic of las_decode_kernel on one staged record: the same operations on the same values (this file is built with
// -ffp-contract=off), hence the same bits.
__device__ __forceinline__ float4 las_record_xyzi(const unsigned char* r, const LasXf& X) {
    auto i32 = [&](int o) { return (int)((unsigned)r[o] | ((unsigned)r[o + 1] << 8) | ((unsigned)r[o + 2] << 16) | ((unsigned)r[o + 3] << 24)); };
    const double x = (double)i32(0) * X.sx + X.ox, y = (double)i32(4) * X.sy + X.oy, z = (double)i32(8) * X.sz + X.oz;
    const double raw = (double)((unsigned)r[12] | ((unsigned)r[13] << 8));
    const double it = X.normalise ? (fmin(fmax(raw, (double)X.lo), (double)X.hi) - (double)X.lo) / (double)X.hi : raw;
    return float4{(float)x, (float)y, (float)z, (float)it};
}

// the predicate of one record; cls = its classification, p = what the plain decode writes for it
__device__ __forceinline__ bool las_record_keep(const unsigned char* r, const LasXf& X, const LasSel& S, unsigned& cls, float4& p) {
    const unsigned b14 = r[14], b15 = r[15];
    unsigned rn, nr, flags;
    if (S.fmt6) {
        rn = b14 & 15u, nr = b14 >> 4, flags = b15 & 15u, cls = r[16];
    } else {
        rn = b14 & 7u, nr = (b14 >> 3) & 7u, flags = b15 >> 5, cls = b15 & 31u;      // no overlap bit: bit 3 of flags stays 0
    }
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((cls >> 5) == (unsigned)k) word = S.cls[k];
    bool keep = (word >> (cls & 31u)) & 1u;
    keep = keep && (flags & S.drop) == 0u;
    if (S.returns == 1) keep = keep && rn == 1u;
    else if (S.returns == 2) keep = keep && rn == nr;
    else if (S.returns == 3) keep = keep && nr == 1u;
    p = las_record_xyzi(r, X);
    return keep && S.z_lo <= p.z && p.z <= S.z_hi;
}

// records [256 blk, 256 blk + cnt) -> LDS with coalesced dword loads; returns cnt.  Ends with a workgroup barrier.
__device__ __forceinline__ int las_stage_block(const unsigned* __restrict__ rec, int record_len, long n, long blk, unsigned* stage) {
    const long first = blk * 256;
    const int cnt = (int)(n - first < 256 ? n - first : 256);
    const int words = (cnt * record_len + 3) / 4;
    const unsigned* src = rec + first * record_len / 4;            // first is a multiple of 256: 4-byte aligned
    for (int w = threadIdx.x; w < words; w += 256) stage[w] = src[w];
    __syncthreads();
    return cnt;
}

// ---- host: what every entry that takes LAS records does before it launches ----------------------------------------------------------

constexpr int las_min_len[11] = {20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67};   // the shortest record of point formats 0 .. 10
constexpr int REC_GROUPS = 4096;         // cap on the workgroups of a kernel that launches as many as are resident at once

// format, record length and count of an entry that knows the format of its records
inline int las_check_records(const char* who, int point_format, int record_len, long n) {
    LM_REQUIRE(point_format >= 0 && point_format <= 10, "%s: unknown point data record format point_format=%d", who, point_format);
    LM_REQUIRE(record_len >= las_min_len[point_format] && record_len <= 160, "%s: bad record_len=%d for format %d (%d .. 160)", who, record_len,
               point_format, las_min_len[point_format]);
    LM_REQUIRE(n >= 0 && n <= 2147483647L, "%s: n=%ld records, at most 2^31 - 1 are supported", who, n);
    return LM_OK;
}

// `select` (NULL: every record passes, S only carries fmt6) checked and converted.  field: how the message names a member, "" in
// lm_las_decode_select ("returns=..."), "select " in the entries that take other arguments too ("select returns=...").
inline int las_check_select(const char* who, const char* field, const LmLasSelect* select, int point_format, LasSel& S) {
    S = LasSel{};
    S.fmt6 = point_format >= 6;
    if (!select) return LM_OK;
    LM_REQUIRE(select->returns >= 0 && select->returns <= 3, "%s: %sreturns=%d is none of all (0), first (1), last (2), single (3)", who, field,
               select->returns);
    LM_REQUIRE(select->drop_flags < 16u, "%s: %sdrop_flags=%u has bits beyond synthetic | key-point | withheld | overlap", who, field,
               select->drop_flags);
    LM_REQUIRE(select->z_lo == select->z_lo && select->z_hi == select->z_hi, "%s: %sz_lo / z_hi must not be NaN", who, field);
    for (int k = 0; k < 8; ++k) S.cls[k] = select->class_mask[k];
    S.drop = select->drop_flags, S.returns = select->returns, S.z_lo = select->z_lo, S.z_hi = select->z_hi;
    return LM_OK;
}

// X * scale + (offset - shift), shift NULL: none; the intensity raw (normalise == 0) or (clip(i, lo, hi) - lo) / hi
inline LasXf las_xf(const double* scale, const double* offset, const double* shift, float lo, float hi, int normalise) {
    const double sh[3] = {shift ? shift[0] : 0.0, shift ? shift[1] : 0.0, shift ? shift[2] : 0.0};
    return LasXf{scale[0], scale[1], scale[2], offset[0] - sh[0], offset[1] - sh[1], offset[2] - sh[2], lo, hi, normalise};
}

// dynamic LDS of a kernel that stages with las_stage_block: 256 records, rounded up to whole words
inline size_t las_stage_bytes(int record_len) { return ((size_t)256 * record_len + 3) / 4 * 4; }

// Workgroups of `kernel` (256 threads, `lds` bytes of dynamic LDS) the current device holds at once, at most REC_GROUPS: asked of the
// runtime once per (device, kernel, lds) and kept.  The current device: like every entry of this library the call launches on it, so it
// must be the stream's.  The number only sizes the grid; the block loop of such a kernel is right for any.
std::mutex las_groups_mu;
std::map<std::tuple<int, const void*, size_t>, long> las_groups_known;

template <class... Args>
int resident_groups(void (*kernel)(Args...), size_t lds, long& groups) {
    int dev_id = 0;
    LM_HIP(hipGetDevice(&dev_id));
    std::lock_guard<std::mutex> lock(las_groups_mu);
    const auto key = std::make_tuple(dev_id, reinterpret_cast<const void*>(kernel), lds);
    const auto it = las_groups_known.find(key);
    if (it != las_groups_known.end()) {
        groups = it->second;
        return LM_OK;
    }
    int per_cu = 0, cus = 0;
    LM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds));
    LM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_id));
    groups = (long)(per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 256);
    groups = groups < REC_GROUPS ? groups : REC_GROUPS;
    las_groups_known[key] = groups;
    return LM_OK;
}

}  // namespace
