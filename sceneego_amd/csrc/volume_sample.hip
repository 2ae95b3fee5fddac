// Trajectory samples: forward-filter backward-sampling over the joint volumes of a sequence (sceneego_amd/volume_smoother.py:
// VolumeSmoother.sample).  No counterpart in the reference.  include/sceneego_hip.h states the definition operation by operation;
// tests/volume_sampler_model.py restates it in numpy float64 and every index, kind and carried voxel written here is compared with it
// bit for bit.  This file is built with -ffp-contract=off: one rounding per operation, every sum sequential in ascending index.
//
// Given the filtered beliefs b_t (float32, as se_volume_filter_f32 wrote them) a trajectory is drawn last frame to first, per sample
// and row:  x_T ~ b_T;  x_t ~ b_t(x) [(1 - floor) W(x -> x_{t+1}) + floor / N] where frame t is linked to t + 1;  x_t ~ b_t where not.
// W(x -> y) = w[di] w[dj] w[dk] with x = y + d: the window of y in blur3's own orientation, no tap reversal.
// Two launches per call:
//   se_draw_sums_kernel (categorical_sums.h, shared with skeleton_sample.hip)
//                     grid (G, rows, frames), block 256: one i-plane [G j][G k] of b_t staged in LDS (rows padded by one float), the row
//                     sums Rs[i][j] = sum_k b (thread j, ascending k) and the slab sum P[i] = sum_j Rs[i][j] (thread 0), in float64, to
//                     the scratch.  The one read of the beliefs that is proportional to the volume.
//   vsm_walk_kernel   grid (samples, rows), block 256: one workgroup per chain, looping over the call's frames from last to first INSIDE
//                     the launch: chains are independent, so there is no grid-wide dependency and no launch per frame.  Per frame:
//                     P of the frame into LDS and its running sums (thread 0: total_t is their last entry); where the frame is linked,
//                     the window sums r[di][dj] over the threads (one (di, dj) row of up to 33 taps each, ascending dk) and q[di] over
//                     the lanes of the second wave, in LDS; thread 0 takes the two Philox blocks of (sample, frame, row), decides step,
//                     jump or fresh draw and makes the window draw from LDS; a global draw (jump, fresh) stages Rs[i][.] and then
//                     b[i][j][.] over the threads for thread 0's two further levels.  Every level is a sequential walk of at most 128
//                     entries (categorical_draw.h).  The drawn voxel is handed from frame to frame through LDS.
// No atomics; index, kind and next are written by thread 0 of the one workgroup that owns them, with plain vector stores.
//
// BYTE MODEL.  The sums pass reads the beliefs once (4 B per frame, row and voxel) and writes 8 (G^2 + G) B per frame and row: 15.7 MB
// read and 0.5 MB written per frame at 15 x 64^3.  The walk reads per (sample, frame, row) at most (2 R + 1)^2 rows of 2 R + 1 floats
// (a linked frame: 37 KB at R = 10), G doubles of P, and for a global draw G doubles of Rs and G floats of b: proportional to the
// samples, not to the volume.  At 15 x 64^3, R = 10 and 16 samples the walk touches 8.9 MB per frame, all of it inside windows of the
// beliefs the sums pass just read.
//
// ORDER.  Every sum is sequential in ascending index and every product is rounded on its own, so the values depend on the inputs alone:
// bitwise identical from run to run, independent of how the frames are cut into calls and of how the samples are split over calls
// (the Philox counter holds the GLOBAL sample and frame index).
#include <float.h>

#include "categorical_draw.h"
#include "categorical_sums.h"    // se_draw_sums_kernel, the sums pass: shared with skeleton_sample.hip
#include "volume_grid.h"          // the limits, the shape predicate and the launch parameters: shared with volume_filter.hip

#pragma clang fp contract(off)

#define SE_VSM_WIN (2 * SE_VG_MAX_R + 1)          // the taps of an axis at most

namespace {

// grid (samples, rows), block 256.  No __restrict__ on next: read and written (by this workgroup alone).
__global__ __launch_bounds__(SE_VG_THREADS) void vsm_walk_kernel(const float* __restrict__ belief, const int* __restrict__ restarted,
                                                                 const float* __restrict__ taps, const double* __restrict__ Rs,
                                                                 const double* __restrict__ P, const int* __restrict__ have_link,
                                                                 int* next, int* __restrict__ index, int* __restrict__ kind,
                                                                 int frames, int rows, int G, int R, double keep, double uniform,
                                                                 uint32_t first_sample, uint32_t first_frame, uint32_t seed_lo,
                                                                 uint32_t seed_hi) {
    __shared__ double vals[SE_VG_MAX_G];                            // the values of one level, then their running sums
    __shared__ double cP[SE_VG_MAX_G];                              // P of the frame, then its running sums
    __shared__ double r[SE_VSM_WIN * SE_VSM_WIN];                   // r[di][dj] of the window
    __shared__ double q[SE_VSM_WIN];
    __shared__ double w[SE_VSM_WIN];
    __shared__ int sh[4];                                           // thread 0's decisions: kind, i, j, the frame's voxel
    const int t = threadIdx.x, s = blockIdx.x, row = blockIdx.y;
    const int GG = G * G, voxels = GG * G;
    if (t <= 2 * R) w[t] = (double)taps[t];
    const size_t chain = (size_t)s * rows + row;
    // y: the voxel drawn for the frame behind the one at hand where that frame is linked to it, else -1.  Uniform over the workgroup.
    int y = -1;
    if (have_link != nullptr && have_link[row] != 0) {
        y = next[chain];
        if (y < 0 || y >= voxels) y = -1;                           // an index outside the grid is never followed
    }
    for (int f = frames - 1; f >= 0; --f) {
        if (f < frames - 1 && restarted[(size_t)(f + 1) * rows + row] != 0) y = -1;
        const size_t fr = (size_t)f * rows + row;
        const float* b = belief + fr * voxels;
        const double* Pf = P + fr * G;
        const double* Rf = Rs + fr * GG;
        int yi = 0, yj = 0, yk = 0, loi = 0, loj = 0, lok = 0, ni = 0, nj = 0, nk = 0;
        __syncthreads();                                            // the taps are staged; the frame before has read its LDS
        if (t < G) cP[t] = Pf[t];
        if (y >= 0) {                                               // the window of y, clipped to the grid: x = y + d
            yi = y / GG; yj = (y / G) % G; yk = y % G;
            loi = max(-R, -yi); ni = min(R, G - 1 - yi) - loi + 1;
            loj = max(-R, -yj); nj = min(R, G - 1 - yj) - loj + 1;
            lok = max(-R, -yk); nk = min(R, G - 1 - yk) - lok + 1;
            for (int e = t; e < ni * nj; e += SE_VG_THREADS) {
                const int a = e / nj, c = e - a * nj;
                const float* src = b + ((size_t)(yi + loi + a) * G + (yj + loj + c)) * G + yk;
                double acc = 0.0;
                for (int d = lok; d < lok + nk; ++d) acc = acc + (double)src[d] * w[d + R];
                r[a * SE_VSM_WIN + c] = acc;
            }
        }
        __syncthreads();
        double total = 0.0, u2 = 0.0, u3 = 0.0;
        int lastP = -1;
        if (t == 0) total = se_draw_scan(cP, G, &lastP);            // total_t: the last running sum
        if (y >= 0 && t >= 64 && t - 64 < ni) {                     // q[di] on the second wave, beside thread 0's scan
            const int a = t - 64;
            double acc = 0.0;
            for (int c = 0; c < nj; ++c) acc = acc + r[a * SE_VSM_WIN + c] * w[loj + c + R];
            q[a] = acc;
        }
        __syncthreads();
        if (t == 0) {
            const uint32_t cs = first_sample + (uint32_t)s, cf = first_frame + (uint32_t)f;
            const SePhilox4 b0 = se_philox4x32_10(cs, cf, (uint32_t)row, 0u, seed_lo, seed_hi);
            const SePhilox4 b1 = se_philox4x32_10(cs, cf, (uint32_t)row, 1u, seed_lo, seed_hi);
            const double u0 = se_uniform53(b0.x[0], b0.x[1]), u1 = se_uniform53(b0.x[2], b0.x[3]);
            u2 = se_uniform53(b1.x[0], b1.x[1]);
            u3 = se_uniform53(b1.x[2], b1.x[3]);
            int mode = 2, x = -1;                                   // 0 a step, 1 a jump, 2 a fresh draw
            if (y >= 0) {
                double Wsum = 0.0;
                for (int a = 0; a < ni; ++a) Wsum = Wsum + q[a] * w[loi + a + R];
                const double step = keep * Wsum, jump = uniform * total, mass = step + jump;
                if (se_draw_mass_ok(mass)) mode = (u0 * mass >= step) ? 1 : 0;
            }
            if (mode == 0) {                                        // the window draw: di, then dj, then dk
                for (int a = 0; a < ni; ++a) vals[a] = q[a] * w[loi + a + R];
                const int a = se_draw(vals, ni, u1);
                if (a >= 0) {
                    for (int c = 0; c < nj; ++c) vals[c] = r[a * SE_VSM_WIN + c] * w[loj + c + R];
                    const int c = se_draw(vals, nj, u2);
                    if (c >= 0) {
                        const float* src = b + ((size_t)(yi + loi + a) * G + (yj + loj + c)) * G + yk;
                        for (int m = 0; m < nk; ++m) vals[m] = (double)src[lok + m] * w[lok + m + R];
                        const int m = se_draw(vals, nk, u3);
                        if (m >= 0) x = ((yi + loi + a) * G + (yj + loj + c)) * G + yk + lok + m;
                    }
                }
                sh[1] = -1;
            } else {                                                // the global draw: i from P
                sh[1] = se_draw_search(cP, G, lastP, total, u1);
            }
            sh[0] = mode;
            sh[3] = x;
        }
        __syncthreads();
        if (sh[0] != 0 && sh[1] >= 0) {                             // uniform: j from Rs[i][.], then k from b[i][j][.]
            const int i = sh[1];
            if (t < G) vals[t] = Rf[(size_t)i * G + t];
            __syncthreads();
            if (t == 0) sh[2] = se_draw(vals, G, u2);
            __syncthreads();
            const int j = sh[2];
            if (j >= 0) {                                           // uniform
                if (t < G) vals[t] = (double)b[((size_t)i * G + j) * G + t];
                __syncthreads();
                if (t == 0) {
                    const int k = se_draw(vals, G, u3);
                    sh[3] = k >= 0 ? (i * G + j) * G + k : -1;
                }
                __syncthreads();
            }
        }
        y = sh[3];                                                  // an invalid draw (-1) links nothing
        if (t == 0) {
            const size_t o = ((size_t)s * frames + f) * rows + row;
            index[o] = y;
            kind[o] = sh[0];
        }
    }
    if (t == 0) next[chain] = y;
}

}  // namespace

// Rs [frames][rows][G][G] and P [frames][rows][G], float64
extern "C" long long se_volume_sample_scratch_bytes(int frames, int rows, int G) {
    if (frames < 1 || !vg_shape_ok(rows, G, 0)) return 0;
    const long long per_row = ((long long)G * G + G) * 8;           // <= 132,096
    if ((long long)frames > (1LL << 62) / per_row / rows) return 0;
    return (long long)frames * rows * per_row;
}

extern "C" int se_volume_sample_f32(const float* belief, const int* restarted, const float* taps, int* next, int* index, int* kind,
                                    void* scratch, long long scratch_bytes, int frames, int rows, int voxels, int G, int radius,
                                    float floor, int samples, long long first_sample, long long first_frame, unsigned int seed_lo,
                                    unsigned int seed_hi, const int* have_link, void* stream) {
    if (!belief || !restarted || !taps || !next || !index || !kind || !scratch) return SE_ERR_BAD_ARG;
    if (!vg_args_ok(frames, rows, voxels, G, radius, floor)) return SE_ERR_BAD_ARG;
    if (samples < 1) return SE_ERR_BAD_ARG;
    // the counter words are 32 bits: every global sample and frame index of the call fits
    if (first_sample < 0 || first_sample + samples > (1LL << 32) || first_frame < 0 || first_frame + frames > (1LL << 32))
        return SE_ERR_BAD_ARG;
    if (!se_aligned({belief, restarted, taps, next, index, kind, have_link}, 4) || !se_aligned({scratch}, 8)) return SE_ERR_BAD_ARG;
    const long long need = se_volume_sample_scratch_bytes(frames, rows, G);
    if (need <= 0 || scratch_bytes < need) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    double* Rs = reinterpret_cast<double*>(scratch);
    double* P = Rs + (size_t)frames * rows * G * G;
    const VgLaunch l = vg_launch(voxels, G, floor);                 // keep and uniform in float32, as the filter's kernels form them
    const int rc = se_draw_sums_launch(belief, Rs, P, frames, rows, G, s);
    if (rc) return rc;
    hipLaunchKernelGGL(vsm_walk_kernel, dim3(samples, rows), dim3(SE_VG_THREADS), 0, s, belief, restarted, taps, Rs, P, have_link, next,
                       index, kind, frames, rows, G, radius, (double)l.keep, (double)l.uniform, (uint32_t)first_sample,
                       (uint32_t)first_frame, (uint32_t)seed_lo, (uint32_t)seed_hi);
    SE_CHECK_LAUNCH();
    return 0;
}
