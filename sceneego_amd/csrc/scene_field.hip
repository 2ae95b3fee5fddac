// Scene distance field: the scene of a depth map as a field on the network's own voxel grid, and any joint distribution against it
// (sceneego_amd/scene_field.py: SceneField; op.py: scene_sites, scene_distance, scene_expect; VoxelNetwork_depth.scene_field /
// scene_expectations drive them).  No counterpart in the reference.
//
//   scene_sites_kernel         one thread per pixel of one frame: the scene point of se_scene_probe_f64 (same pixel walk, same depth
//                              lookup, same drop rules), rounded half-to-even to the voxel whose centre is nearest; every writer
//                              stores the same byte 1 with an ordinary vector store, so the write order cannot matter.  float64,
//                              unfused (built with -ffp-contract=off): one right answer, bit for bit.
//   scene_edt_slab_kernel      the exact Euclidean distance transform, passes k and j: one workgroup per (frame, i) slab.  The slab's
//                              G^2 site bytes go to LDS; pass k leaves per (j, k) the nearest site position k' of the line (one byte),
//                              pass j takes per (j, k) the minimum over j' of (k - k')^2 + (j - j')^2 and writes the pair
//                              (d2, flat index) to scratch.  LDS: 2 G^2 bytes (32 KB at G = 128).
//   scene_edt_plane_kernel     pass i: one workgroup per (frame, j, tile of 32 k).  The tile's G x 32 pairs go to LDS (32 KB at
//                              G = 128), every thread takes the minimum over i' for its outputs; global accesses are contiguous
//                              along k.
//                              THE KEY of a candidate is (d2, flat index), compared lexicographically.  Inside one pass the candidates
//                              of an output come from different positions of one grid line, and the flat index of a candidate grows
//                              with its position on the line in every pass (the position is the most significant part of the index
//                              that differs).  So walking the line in ascending order and replacing on d2 < best alone keeps, among
//                              equal d2, the lowest index: the minimum of the key, in integers, with no 64-bit arithmetic.
//   expect_partial_kernel      pass 1 of a split-row reduction (row_reduce.h states the scheme and why it is bitwise deterministic):
//                              4 + 2 K float32 sums per chunk and the NaN marker, carried in the record's peak slots.  One
//                              instantiation per number of radii K = 1..8: the pass is bound by its vector arithmetic (two
//                              comparisons and two conditional additions per voxel and radius), not by the 4 B / voxel / row it reads,
//                              so the radii that are not asked for must cost nothing.
//   expect_fold_kernel         pass 2: folds the row's records and writes out[row][24].
#include "row_reduce.h"

#pragma clang fp contract(off)

#define SE_SF_PART 24      // mass blocked dist free_dist, K contact sums, K free contact sums, the NaN marker as a peak (p, index bits), pad
#define SE_SF_NONE 0x7fffffff
#define SE_SF_KT 32        // k positions per workgroup of pass i

namespace {

// grid (ceil(H W / 256), B), block 256
__global__ __launch_bounds__(256) void scene_sites_kernel(const float* __restrict__ depth, const double* __restrict__ ray_tab,
                                                          unsigned char* __restrict__ sites, int dh, int dw, int H, int W, int G,
                                                          double side, double min_z, double max_depth) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int b = blockIdx.y;
    const double* r = ray_tab + (size_t)pix * 3;
    const double rx = r[0], ry = r[1], rz = r[2];
    if (!(isfinite(rx) && isfinite(ry) && isfinite(rz))) return;
    const int y = pix / W, x = pix - y * W;
    const int py = (int)(((long long)y * dh) / H), px = (int)(((long long)x * dw) / W);
    const double d = (double)depth[((size_t)b * dh + py) * dw + px];
    if (!(d > 0.0 && d <= max_depth)) return;                       // a NaN fails
    const double sx = rx * d, sy = ry * d, sz = rz * d;
    if (!(sz > min_z)) return;
    const double half = side / 2.0, g1 = (double)(G - 1);
    const double qx = rint(((sx + half) * g1) / side);
    const double qy = rint(((sy + half) * g1) / side);
    const double qz = rint((sz * g1) / side);
    if (!(qx >= 0.0 && qx <= g1 && qy >= 0.0 && qy <= g1 && qz >= 0.0 && qz <= g1)) return;   // a NaN or an infinity fails
    const int n = ((int)qx * G + (int)qy) * G + (int)qz;            // 0 <= n < G^3 by the test above
    sites[(size_t)b * G * G * G + n] = 1;
}

// grid (G, B), block 256.  site_b[j G + k]: the slab's site bytes; near_b[j G + k]: pass k's result, the position k' of the nearest
// site of line (i, j) seen from k (the lowest among equals), 0xff without a site on the line.
__global__ __launch_bounds__(256) void scene_edt_slab_kernel(const unsigned char* __restrict__ sites, int2* __restrict__ pairs, int G) {
    __shared__ unsigned char site_b[128 * 128];
    __shared__ unsigned char near_b[128 * 128];
    const int i = blockIdx.x, b = blockIdx.y;
    const int GG = G * G;
    const size_t slab = ((size_t)b * G + i) * GG;
    for (int o = threadIdx.x; o < GG; o += 256) site_b[o] = sites[slab + o];
    __syncthreads();
    for (int o = threadIdx.x; o < GG; o += 256) {
        const int j = o / G, k = o - j * G;
        int best = SE_SF_NONE, at = 0xff;
        for (int kk = 0; kk < G; ++kk) {
            const int dk = k - kk, d2 = dk * dk;
            if (site_b[j * G + kk] != 0 && d2 < best) { best = d2; at = kk; }
        }
        near_b[o] = (unsigned char)at;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < GG; o += 256) {
        const int j = o / G, k = o - j * G;
        int best = SE_SF_NONE, idx = -1;
        for (int jj = 0; jj < G; ++jj) {
            const int kk = near_b[jj * G + k];
            const int dk = k - kk, dj = j - jj, d2 = dk * dk + dj * dj;
            if (kk != 0xff && d2 < best) { best = d2; idx = (i * G + jj) * G + kk; }
        }
        pairs[slab + o] = make_int2(best, idx);
    }
}

// grid (ceil(G / 32), G, B), block 256: tile[i' * 32 + kk] = the pair of voxel (i', j, k0 + kk) after passes k and j
__global__ __launch_bounds__(256) void scene_edt_plane_kernel(const int2* __restrict__ pairs, int* __restrict__ d2_out,
                                                              int* __restrict__ nearest, int G) {
    __shared__ int2 tile[128 * SE_SF_KT];
    const int k0 = blockIdx.x * SE_SF_KT, j = blockIdx.y, b = blockIdx.z;
    const int kw = min(SE_SF_KT, G - k0);
    const size_t frame = (size_t)b * G * G * G;
    for (int o = threadIdx.x; o < G * SE_SF_KT; o += 256) {
        const int ii = o / SE_SF_KT, kk = o - ii * SE_SF_KT;
        if (kk < kw) tile[o] = pairs[frame + ((size_t)ii * G + j) * G + k0 + kk];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < G * SE_SF_KT; o += 256) {
        const int i = o / SE_SF_KT, kk = o - i * SE_SF_KT;
        if (kk >= kw) continue;
        int best = SE_SF_NONE, idx = -1;
        for (int ii = 0; ii < G; ++ii) {
            const int2 c = tile[ii * SE_SF_KT + kk];
            const int di = i - ii;
            const int d2 = c.x == SE_SF_NONE ? SE_SF_NONE : c.x + di * di;   // c.x <= 2 * 127^2 where there is a candidate
            if (d2 < best) { best = d2; idx = c.y; }
        }
        const size_t n = frame + ((size_t)i * G + j) * G + k0 + kk;
        d2_out[n] = best;
        nearest[n] = idx;
    }
}

// grid (splits, rows), block 256
template <int K>
__global__ __launch_bounds__(256) void expect_partial_kernel(const float* __restrict__ prob, const int* __restrict__ d2,
                                                             const unsigned char* __restrict__ free_mask,
                                                             const int* __restrict__ radii2, float* __restrict__ scratch, int voxels,
                                                             int splits, int rows_per_frame) {
    constexpr int N = 4 + 2 * K;
    __shared__ float sm[4][SE_SF_PART];
    const int row = blockIdx.y, s = blockIdx.x;
    const int chunk = se_row_chunk(voxels, splits);
    const int c0 = s * chunk;
    const int c1 = min(c0 + chunk, voxels);
    const float* v = prob + (size_t)row * voxels;
    const size_t frame = (size_t)(row / rows_per_frame) * voxels;
    const int* dd = d2 + frame;
    const unsigned char* fm = free_mask + frame;
    int rad[K];
#pragma unroll
    for (int k = 0; k < K; ++k) rad[k] = radii2[k];

    float acc[N];
#pragma unroll
    for (int a = 0; a < N; ++a) acc[a] = 0.f;
    bool nan = false;
    for (int i = c0 + threadIdx.x * 4; i < c1; i += 1024) {
        const unsigned fw = *reinterpret_cast<const unsigned*>(fm + i);
        const f32x4 q = *reinterpret_cast<const f32x4*>(v + i);
        const int4 e = *reinterpret_cast<const int4*>(dd + i);
        const int ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float p = q[k];
            const int d = ev[k];
            const bool is_free = ((fw >> (8 * k)) & 0xffu) != 0;
            nan |= p != p;
            acc[0] += p;
            if (!is_free) acc[1] += p;
            if (d != SE_SF_NONE) {
                const float t = p * sqrtf((float)d);
                acc[2] += t;
                if (is_free) acc[3] += t;
            }
#pragma unroll
            for (int r = 0; r < K; ++r) {
                if (d <= rad[r]) {
                    acc[4 + r] += p;
                    if (is_free) acc[4 + K + r] += p;
                }
            }
        }
    }
    block_fold_record<N, SE_SF_PART>(acc, nan ? PEAK_NAN : PEAK_NONE, sm, scratch + ((size_t)row * splits + s) * SE_SF_PART);
}

// grid (rows), block 64: one wave per row
template <int K>
__global__ __launch_bounds__(64) void expect_fold_kernel(const float* __restrict__ scratch, float* __restrict__ out, int voxels,
                                                         int splits) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const float* part = scratch + (size_t)row * splits * SE_SF_PART;
    constexpr int N = 4 + 2 * K;
    float acc[N];
    const Peak pk = wave_fold_chunks<N, SE_SF_PART>(part, splits, voxels, lane, acc);
    if (lane != 0) return;
    float* o = out + (size_t)row * 24;
    if (pk.idx < 0) {                        // a NaN probability somewhere in the row
        const float q = __int_as_float(0x7fc00000);
#pragma unroll
        for (int a = 0; a < 24; ++a) o[a] = q;
        return;
    }
#pragma unroll
    for (int a = 0; a < 24; ++a) o[a] = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) o[a] = acc[a];
#pragma unroll
    for (int r = 0; r < K; ++r) {
        o[4 + r] = acc[4 + r];
        o[12 + r] = acc[4 + K + r];
    }
}

template <int K>
int launch_expect(const float* prob, const int* d2, const unsigned char* free_mask, const int* radii2, float* out, float* scratch,
                  int rows, int rows_per_frame, int voxels, hipStream_t s) {
    const int splits = se_sa_splits(rows);
    hipLaunchKernelGGL(expect_partial_kernel<K>, dim3(splits, rows), dim3(256), 0, s, prob, d2, free_mask, radii2, scratch, voxels,
                       splits, rows_per_frame);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(expect_fold_kernel<K>, dim3(rows), dim3(64), 0, s, scratch, out, voxels, splits);
    SE_CHECK_LAUNCH();
    return 0;
}

inline bool distance_shape_ok(int batch, int grid) { return batch > 0 && batch <= 65535 && grid >= 2 && grid <= 128; }

}  // namespace

extern "C" int se_scene_sites_u8(const float* depth, const double* ray_tab, unsigned char* sites, int batch, int depth_h, int depth_w,
                                 int height, int width, int grid, double side, double min_z, double max_depth, void* stream) {
    if (!depth || !ray_tab || !sites) return SE_ERR_BAD_ARG;
    if (batch <= 0 || batch > 65535 || depth_h <= 0 || depth_w <= 0 || height <= 0 || width <= 0) return SE_ERR_BAD_ARG;
    if ((long long)height * width > 0x7fff0000ll || grid < 2 || grid > 1024) return SE_ERR_BAD_ARG;
    if (!(side > 0.0) || !(side < __builtin_inf()) || !(min_z >= 0.0) || !(max_depth > 0.0)) return SE_ERR_BAD_ARG;   // a NaN fails each
    hipStream_t s = se_stream(stream);
    const size_t bytes = (size_t)batch * grid * grid * grid;
    const hipError_t e = hipMemsetAsync(sites, 0, bytes, s);
    if (e != hipSuccess) return (int)e;
    const unsigned blocks = (unsigned)(((long long)height * width + 255) / 256);
    hipLaunchKernelGGL(scene_sites_kernel, dim3(blocks, batch), dim3(256), 0, s, depth, ray_tab, sites, depth_h, depth_w, height, width,
                       grid, side, min_z, max_depth);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" long long se_scene_distance_scratch_bytes(int batch, int grid) {
    if (!distance_shape_ok(batch, grid)) return -1;
    return (long long)batch * grid * grid * grid * (long long)sizeof(int2);
}

extern "C" int se_scene_distance_i32(const unsigned char* sites, int* d2, int* nearest, void* scratch, long long scratch_bytes,
                                     int batch, int grid, void* stream) {
    if (!sites || !d2 || !nearest || !scratch) return SE_ERR_BAD_ARG;
    if (!distance_shape_ok(batch, grid)) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_scene_distance_scratch_bytes(batch, grid)) return SE_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) || !se_aligned({d2, nearest}, 4)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    int2* pairs = static_cast<int2*>(scratch);
    hipLaunchKernelGGL(scene_edt_slab_kernel, dim3(grid, batch), dim3(256), 0, s, sites, pairs, grid);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(scene_edt_plane_kernel, dim3((grid + SE_SF_KT - 1) / SE_SF_KT, grid, batch), dim3(256), 0, s, pairs, d2, nearest,
                       grid);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" long long se_scene_expect_scratch_elems(int rows) {
    return rows > 0 ? (long long)rows * se_sa_splits(rows) * SE_SF_PART : 0;
}

extern "C" int se_scene_expect_f32(const float* prob, const int* d2, const unsigned char* free_mask, const int* radii2, float* out,
                                   float* scratch, int rows, int rows_per_frame, int voxels, int n_radii, void* stream) {
    if (rows <= 0 || rows > 65535 || rows_per_frame <= 0 || rows % rows_per_frame || voxels <= 0 || (voxels & 3)) return SE_ERR_BAD_ARG;
    if (n_radii < 1 || n_radii > 8) return SE_ERR_BAD_ARG;
    if (!prob || !d2 || !free_mask || !radii2 || !out || !scratch) return SE_ERR_BAD_ARG;
    // the 16-byte loads of pass 1, and its 32-bit load of four mask bytes
    if (!se_aligned({prob, d2}, 16) || !se_aligned({free_mask, radii2}, 4)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    switch (n_radii) {
#define SE_SF_CASE(K) \
    case K: return launch_expect<K>(prob, d2, free_mask, radii2, out, scratch, rows, rows_per_frame, voxels, s);
        SE_SF_CASE(1) SE_SF_CASE(2) SE_SF_CASE(3) SE_SF_CASE(4) SE_SF_CASE(5) SE_SF_CASE(6) SE_SF_CASE(7) SE_SF_CASE(8)
#undef SE_SF_CASE
    }
    return SE_ERR_BAD_ARG;
}
