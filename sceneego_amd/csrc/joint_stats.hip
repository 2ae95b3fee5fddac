// Per-joint statistics of the softmaxed volumes the soft-argmax writes: the second central moment of the voxel-centre coordinates
// about the soft-argmax joint (6 values), the entropy, and the peak (value, lowest flat index, coordinate).  HBM/MALL-bound like
// softargmax.hip: 4 B/voxel/row read once, plus the [voxels][3] coordinates (L2 resident).
//
// Two launches, split-row exactly as the soft-argmax (se_sa_splits(rows) chunks per row, the same chunk rule):
//   pass 1: grid (splits, rows), block 256: every workgroup reduces its chunk to one record of SE_JS_PART floats in scratch
//   pass 2: one wave per row folds the row's records in a fixed order (lane k takes chunks k, k + 64, ... in sequence, then a
//           butterfly over the lanes) and writes stats[row][12] and peak_index[row]
// No atomics: every sum is taken in an order that depends on the shape alone, so the result is bitwise identical from run to run.
// An empty chunk (k * chunk >= voxels) is skipped by its position, never by the value of its record.
//
// The peak is the pair (p, index) under the order "larger p first, then lower index": the combine is commutative and associative, so
// any reduction tree gives the same pair.  A NaN probability is carried in the same pair as (+inf, -1), which wins every combine:
// a row whose folded index is negative held a NaN, and all 12 floats of that row are written as NaN.
#include "common.h"

#define SE_JS_PART 12   // cxx cyy czz cxy cxz cyz entropy peak_p peak_index(int bits) pad pad pad

namespace {

struct Peak {
    float p;
    int idx;
};
__device__ __forceinline__ Peak peak_combine(Peak a, Peak b) {
    const bool take_b = b.p > a.p || (b.p == a.p && b.idx < a.idx);
    return take_b ? b : a;
}
__device__ __forceinline__ Peak wave_reduce_peak(Peak v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Peak o;
        o.p = __shfl_xor(v.p, off, 64);
        o.idx = __shfl_xor(v.idx, off, 64);
        v = peak_combine(v, o);
    }
    return v;
}

// grid (splits, rows), block 256
__global__ __launch_bounds__(256) void joint_stats_partial_kernel(const float* __restrict__ prob, const float* __restrict__ coord,
                                                                  const float* __restrict__ joints, float* __restrict__ scratch,
                                                                  int voxels, int splits) {
    __shared__ float sm[4][SE_JS_PART];
    const int row = blockIdx.y, s = blockIdx.x;
    const int chunk = (((voxels + splits - 1) / splits) + 3) & ~3;
    const int c0 = s * chunk;
    const int c1 = min(c0 + chunk, voxels);
    const float* v = prob + (size_t)row * voxels;
    const float jx = joints[row * 3 + 0], jy = joints[row * 3 + 1], jz = joints[row * 3 + 2];

    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // cxx cyy czz cxy cxz cyz entropy
    Peak pk = {-INFINITY, INT_MAX};
    bool nan = false;
    for (int i = c0 + threadIdx.x * 4; i < c1; i += 1024) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(v + i);
        const f32x4 c_a = *reinterpret_cast<const f32x4*>(coord + (size_t)i * 3);
        const f32x4 c_b = *reinterpret_cast<const f32x4*>(coord + (size_t)i * 3 + 4);
        const f32x4 c_c = *reinterpret_cast<const f32x4*>(coord + (size_t)i * 3 + 8);
        const float p[4] = {x.x, x.y, x.z, x.w};
        const float cx[4] = {c_a.x, c_a.w, c_b.z, c_c.y};
        const float cy[4] = {c_a.y, c_b.x, c_b.w, c_c.z};
        const float cz[4] = {c_a.z, c_b.y, c_c.x, c_c.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dx = cx[k] - jx, dy = cy[k] - jy, dz = cz[k] - jz;
            const float px = p[k] * dx, py = p[k] * dy, pz = p[k] * dz;
            acc[0] += px * dx; acc[1] += py * dy; acc[2] += pz * dz;
            acc[3] += px * dy; acc[4] += px * dz; acc[5] += py * dz;
            if (p[k] != 0.f) acc[6] -= p[k] * logf(p[k]);      // a voxel with p == 0 contributes 0
            if (p[k] > pk.p) { pk.p = p[k]; pk.idx = i + k; }   // indices ascend within a lane: strict > keeps the lowest
            nan |= p[k] != p[k];
        }
    }
    if (nan) { pk.p = INFINITY; pk.idx = -1; }

#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = wave_reduce_sum(acc[k]);
    pk = wave_reduce_peak(pk);
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) sm[wid][k] = acc[k];
        sm[wid][7] = pk.p;
        sm[wid][8] = __int_as_float(pk.idx);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* out = scratch + ((size_t)row * splits + s) * SE_JS_PART;
#pragma unroll
        for (int k = 0; k < 7; ++k) out[k] = (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
        Peak r = {sm[0][7], __float_as_int(sm[0][8])};
#pragma unroll
        for (int w = 1; w < 4; ++w) r = peak_combine(r, Peak{sm[w][7], __float_as_int(sm[w][8])});
        out[7] = r.p;
        out[8] = __int_as_float(r.idx);
    }
}

// grid (rows), block 64: one wave per row
__global__ __launch_bounds__(64) void joint_stats_fold_kernel(const float* __restrict__ scratch, const float* __restrict__ coord,
                                                              float* __restrict__ stats, int* __restrict__ peak_index, int voxels,
                                                              int splits) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* part = scratch + (size_t)row * splits * SE_JS_PART;
    const int chunk = (((voxels + splits - 1) / splits) + 3) & ~3;
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    Peak pk = {-INFINITY, INT_MAX};
    for (int k = lane; k < splits; k += 64) {
        if (k * chunk >= voxels) continue;   // empty chunk: its record holds the neutral element, skipped by position all the same
        const float* p = part + k * SE_JS_PART;
#pragma unroll
        for (int a = 0; a < 7; ++a) acc[a] += p[a];
        pk = peak_combine(pk, Peak{p[7], __float_as_int(p[8])});
    }
#pragma unroll
    for (int a = 0; a < 7; ++a) acc[a] = wave_reduce_sum(acc[a]);
    pk = wave_reduce_peak(pk);
    if (lane != 0) return;
    float* o = stats + (size_t)row * 12;
    if (pk.idx < 0 || pk.idx >= voxels) {   // a NaN probability somewhere in the row (>= voxels cannot happen: voxels > 0)
        const float q = __int_as_float(0x7fc00000);
#pragma unroll
        for (int a = 0; a < 12; ++a) o[a] = q;
        peak_index[row] = -1;
        return;
    }
#pragma unroll
    for (int a = 0; a < 7; ++a) o[a] = acc[a];
    o[7] = pk.p;
    o[8] = coord[(size_t)pk.idx * 3 + 0];
    o[9] = coord[(size_t)pk.idx * 3 + 1];
    o[10] = coord[(size_t)pk.idx * 3 + 2];
    o[11] = sqrtf((acc[0] + acc[1]) + acc[2]);
    peak_index[row] = pk.idx;
}

}  // namespace

extern "C" long long se_joint_stats_scratch_elems(int rows) {
    return rows > 0 ? (long long)rows * se_sa_splits(rows) * SE_JS_PART : 0;
}

extern "C" int se_joint_stats_f32(const float* prob, const float* coord, const float* joints, float* stats, int* peak_index,
                                  float* scratch, int rows, int voxels, void* stream) {
    if (rows <= 0 || rows > 65535 || voxels <= 0 || (voxels & 3)) return SE_ERR_BAD_ARG;
    if (!prob || !coord || !joints || !stats || !peak_index || !scratch) return SE_ERR_BAD_ARG;
    // the 16-byte loads of pass 1
    if ((reinterpret_cast<uintptr_t>(prob) & 15) || (reinterpret_cast<uintptr_t>(coord) & 15)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    const int splits = se_sa_splits(rows);
    hipLaunchKernelGGL(joint_stats_partial_kernel, dim3(splits, rows), dim3(256), 0, s, prob, coord, joints, scratch, voxels, splits);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(joint_stats_fold_kernel, dim3(rows), dim3(64), 0, s, scratch, coord, stats, peak_index, voxels, splits);
    SE_CHECK_LAUNCH();
    return 0;
}
