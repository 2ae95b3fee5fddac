// Per-joint statistics of the softmaxed volumes the soft-argmax writes: the second central moment of the voxel-centre coordinates
// about the soft-argmax joint (6 values), the entropy, and the peak (value, lowest flat index, coordinate).  HBM/MALL-bound like
// softargmax.hip: 4 B/voxel/row read once, plus the [voxels][3] coordinates (L2 resident).
//
// Two launches, split-row with a peak (row_reduce.h states the scheme, the peak's order and NaN marker, and why the result is bitwise
// deterministic): pass 1 writes one record of SE_JS_PART floats per chunk, pass 2 folds them and writes stats[row][12] and
// peak_index[row].  A row that held a NaN gets 12 NaNs.
#include "row_reduce.h"

#define SE_JS_PART 12   // cxx cyy czz cxy cxz cyz entropy peak_p peak_index(int bits) pad pad pad

namespace {

// grid (splits, rows), block 256
__global__ __launch_bounds__(256) void joint_stats_partial_kernel(const float* __restrict__ prob, const float* __restrict__ coord,
                                                                  const float* __restrict__ joints, float* __restrict__ scratch,
                                                                  int voxels, int splits) {
    __shared__ float sm[4][SE_JS_PART];
    const int row = blockIdx.y, s = blockIdx.x;
    const int chunk = se_row_chunk(voxels, splits);
    const int c0 = s * chunk;
    const int c1 = min(c0 + chunk, voxels);
    const float* v = prob + (size_t)row * voxels;
    const float jx = joints[row * 3 + 0], jy = joints[row * 3 + 1], jz = joints[row * 3 + 2];

    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // cxx cyy czz cxy cxz cyz entropy
    Peak pk = PEAK_NONE;
    bool nan = false;
    for (int i = c0 + threadIdx.x * 4; i < c1; i += 1024) {
        const Quad q = load_quad(v, coord, i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float p = q.p[k];
            const float dx = q.cx[k] - jx, dy = q.cy[k] - jy, dz = q.cz[k] - jz;
            const float px = p * dx, py = p * dy, pz = p * dz;
            acc[0] += px * dx; acc[1] += py * dy; acc[2] += pz * dz;
            acc[3] += px * dy; acc[4] += px * dz; acc[5] += py * dz;
            if (p != 0.f) acc[6] -= p * logf(p);               // a voxel with p == 0 contributes 0
            if (p > pk.p) { pk.p = p; pk.idx = i + k; }        // indices ascend within a lane: strict > keeps the lowest
            nan |= p != p;
        }
    }
    if (nan) pk = PEAK_NAN;
    block_fold_record<7, SE_JS_PART>(acc, pk, sm, scratch + ((size_t)row * splits + s) * SE_JS_PART);
}

// grid (rows), block 64: one wave per row
__global__ __launch_bounds__(64) void joint_stats_fold_kernel(const float* __restrict__ scratch, const float* __restrict__ coord,
                                                              float* __restrict__ stats, int* __restrict__ peak_index, int voxels,
                                                              int splits) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* part = scratch + (size_t)row * splits * SE_JS_PART;
    float acc[7];
    const Peak pk = wave_fold_chunks<7, SE_JS_PART>(part, splits, voxels, lane, acc);
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
