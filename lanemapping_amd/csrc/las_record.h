// The LAS point record on the device, shared by the decode (lidar.hip) and the labelling (label.hip): the decode's arithmetic on one
// staged record, the selection predicate of lm_las_decode_select, and the staging of 256 records in LDS.  Sources that include this are
// built with -ffp-contract=off (build.py EXACT_FP), so the same expression gives the same bits in every kernel that uses it.
#pragma once
#include "common.h"

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

}  // namespace
