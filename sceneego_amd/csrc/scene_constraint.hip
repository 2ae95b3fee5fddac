// Scene-constrained joints: the free space of the voxel grid in front of a frame's depth surface, and the soft-argmax reductions over
// the free voxels alone (sceneego_amd/op.py: scene_free_mask, constrained_joints; VoxelNetwork_depth.constrain_to_scene drives them).
// No counterpart in the reference.
//
//   scene_free_mask_kernel     one thread per four voxels of one frame: the voxel's pixel (host-built sight table: pix, rng), the
//                              depth there, one float64 sum and one comparison per voxel; the four uint8 results leave as one 32-bit
//                              vector store.  Built with -ffp-contract=off: the mask has one right answer, bit for bit
//                              (tests/scene_constraint_model.py restates it).
//   masked_partial_kernel      pass 1 of a split-row reduction with a peak (row_reduce.h states the scheme, the peak's order and NaN
//                              marker, and why the result is bitwise deterministic): one record of SE_SC_PART floats per chunk.
//                              HBM/MALL-bound: 4 B/voxel/row of probabilities read once; the [voxels][3] coordinates and the frame's
//                              mask (1 B/voxel, shared by the frame's rows) stay cache-resident; one 32-bit load for four mask bytes.
//   masked_fold_kernel         pass 2: folds the row's records and writes out[row][8] and peak_index[row].  The peak is taken over the
//                              FREE voxels alone, so its neutral element survives in a row without a free voxel; a NaN probability
//                              (free or blocked) marks the row, and all 8 floats of that row are written as NaN.  No division anywhere.
#include "row_reduce.h"

#pragma clang fp contract(off)

#define SE_SC_PART 8   // free_mass sx sy sz peak_p peak_index(int bits) pad pad

namespace {

// grid (ceil(voxels / 1024), B), block 256: thread t of block g owns the voxels 4 (256 g + t) .. + 3 of frame blockIdx.y
__global__ __launch_bounds__(256) void scene_free_mask_kernel(const float* __restrict__ depth, const int* __restrict__ pix,
                                                              const float* __restrict__ rng, unsigned* __restrict__ free_words,
                                                              int dh, int dw, int H, int W, int voxels, double margin,
                                                              double max_depth) {
    const int n0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= voxels) return;                           // voxels is a multiple of 4: n0 + 3 < voxels below
    const int b = blockIdx.y;
    const int npix = H * W;
    const float* dmap = depth + (size_t)b * dh * dw;
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = pix[n0 + k];
        bool blocked = false;
        if (p >= 0 && p < npix) {                       // p >= npix: no pixel of this frame, treated as no evidence
            const int y = p / W, x = p - y * W;
            const int py = (int)(((long long)y * dh) / H), px = (int)(((long long)x * dw) / W);
            const double d = (double)dmap[(size_t)py * dw + px];
            if (d > 0.0 && d <= max_depth) blocked = d + margin < (double)rng[n0 + k];   // a NaN fails the surface test
        }
        word |= (blocked ? 0u : 1u) << (8 * k);
    }
    free_words[((size_t)b * voxels + n0) >> 2] = word;
}

// grid (splits, rows), block 256
__global__ __launch_bounds__(256) void masked_partial_kernel(const float* __restrict__ prob, const float* __restrict__ coord,
                                                             const unsigned char* __restrict__ free_mask, float* __restrict__ scratch,
                                                             int voxels, int splits, int rows_per_frame) {
    __shared__ float sm[4][SE_SC_PART];
    const int row = blockIdx.y, s = blockIdx.x;
    const int chunk = se_row_chunk(voxels, splits);
    const int c0 = s * chunk;
    const int c1 = min(c0 + chunk, voxels);
    const float* v = prob + (size_t)row * voxels;
    const unsigned char* fm = free_mask + (size_t)(row / rows_per_frame) * voxels;

    float acc[4] = {0.f, 0.f, 0.f, 0.f};   // free_mass sx sy sz
    Peak pk = PEAK_NONE;
    bool nan = false;
    for (int i = c0 + threadIdx.x * 4; i < c1; i += 1024) {
        const unsigned fw = *reinterpret_cast<const unsigned*>(fm + i);
        const Quad q = load_quad(v, coord, i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float p = q.p[k];
            nan |= p != p;
            if ((fw >> (8 * k)) & 0xffu) {
                acc[0] += p;
                acc[1] += p * q.cx[k]; acc[2] += p * q.cy[k]; acc[3] += p * q.cz[k];
                if (p > pk.p) { pk.p = p; pk.idx = i + k; }   // indices ascend within a lane: strict > keeps the lowest
            }
        }
    }
    if (nan) pk = PEAK_NAN;
    block_fold_record<4, SE_SC_PART>(acc, pk, sm, scratch + ((size_t)row * splits + s) * SE_SC_PART);
}

// grid (rows), block 64: one wave per row
__global__ __launch_bounds__(64) void masked_fold_kernel(const float* __restrict__ scratch, const float* __restrict__ coord,
                                                         float* __restrict__ out, int* __restrict__ peak_index, int voxels,
                                                         int splits) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* part = scratch + (size_t)row * splits * SE_SC_PART;
    float acc[4];
    const Peak pk = wave_fold_chunks<4, SE_SC_PART>(part, splits, voxels, lane, acc);
    if (lane != 0) return;
    float* o = out + (size_t)row * 8;
    const float q = __int_as_float(0x7fc00000);
    if (pk.idx < 0) {                        // a NaN probability somewhere in the row
#pragma unroll
        for (int a = 0; a < 8; ++a) o[a] = q;
        peak_index[row] = -1;
        return;
    }
    if (pk.idx >= voxels) {                  // the neutral element survived: no free voxel in the row
        o[0] = o[1] = o[2] = o[3] = o[4] = 0.f;
        o[5] = o[6] = o[7] = q;
        peak_index[row] = -1;
        return;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) o[a] = acc[a];
    o[4] = pk.p;
    o[5] = coord[(size_t)pk.idx * 3 + 0];
    o[6] = coord[(size_t)pk.idx * 3 + 1];
    o[7] = coord[(size_t)pk.idx * 3 + 2];
    peak_index[row] = pk.idx;
}

}  // namespace

extern "C" int se_scene_free_mask_u8(const float* depth, const int* pix, const float* rng, unsigned char* free_mask, int batch,
                                     int depth_h, int depth_w, int height, int width, int voxels, double margin, double max_depth,
                                     void* stream) {
    if (!depth || !pix || !rng || !free_mask) return SE_ERR_BAD_ARG;
    if (batch <= 0 || batch > 65535 || depth_h <= 0 || depth_w <= 0 || height <= 0 || width <= 0) return SE_ERR_BAD_ARG;
    if ((long long)height * width > 0x7fff0000ll || voxels <= 0 || (voxels & 3)) return SE_ERR_BAD_ARG;
    if (!(margin == margin) || !(max_depth > 0.0)) return SE_ERR_BAD_ARG;              // a NaN fails both
    if (reinterpret_cast<uintptr_t>(free_mask) & 3) return SE_ERR_BAD_ARG;             // the 32-bit stores
    hipStream_t s = se_stream(stream);
    const unsigned blocks = (unsigned)((voxels / 4 + 255) / 256);
    hipLaunchKernelGGL(scene_free_mask_kernel, dim3(blocks, batch), dim3(256), 0, s, depth, pix, rng,
                       reinterpret_cast<unsigned*>(free_mask), depth_h, depth_w, height, width, voxels, margin, max_depth);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" long long se_softargmax3d_masked_scratch_elems(int rows) {
    return rows > 0 ? (long long)rows * se_sa_splits(rows) * SE_SC_PART : 0;
}

extern "C" int se_softargmax3d_masked_f32(const float* prob, const float* coord, const unsigned char* free_mask, float* out,
                                          int* peak_index, float* scratch, int rows, int rows_per_frame, int voxels, void* stream) {
    if (rows <= 0 || rows > 65535 || rows_per_frame <= 0 || rows % rows_per_frame || voxels <= 0 || (voxels & 3)) return SE_ERR_BAD_ARG;
    if (!prob || !coord || !free_mask || !out || !peak_index || !scratch) return SE_ERR_BAD_ARG;
    // the 16-byte loads of pass 1, and its 32-bit load of four mask bytes
    if ((reinterpret_cast<uintptr_t>(prob) & 15) || (reinterpret_cast<uintptr_t>(coord) & 15)) return SE_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(free_mask) & 3) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    const int splits = se_sa_splits(rows);
    hipLaunchKernelGGL(masked_partial_kernel, dim3(splits, rows), dim3(256), 0, s, prob, coord, free_mask, scratch, voxels, splits,
                       rows_per_frame);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(masked_fold_kernel, dim3(rows), dim3(64), 0, s, scratch, coord, out, peak_index, voxels, splits);
    SE_CHECK_LAUNCH();
    return 0;
}
