// The sums pass of the samplers: the row and slab sums of [frames][rows][G^3] float32 volumes in float64, the two upper levels of the
// three-level categorical draw of categorical_draw.h (i from P, j from Rs[i][.], k from the volume's row).  volume_sample.hip (the
// filtered beliefs of a sequence, rows = the tracks) and skeleton_sample.hip (the upward products A_j of a frame, rows = the joints)
// launch it; stated once here.  tests/volume_sampler_model.py: Frame restates it (np.cumsum, ascending).
//
// Include it from a file built with -ffp-contract=off, as categorical_draw.h: every sum is one rounded float64 addition per entry.
#pragma once
#include "common.h"

#define SE_CS_THREADS 256
#define SE_CS_MAX_G 128
#define SE_CS_MAX_Z 65535                         // grid.z of the sums pass; more frames than that take turns

namespace {

// grid (G, rows, min(frames, 65535)), block 256, dynamic LDS G (G + 1) floats.  Rs [frames][rows][G][G], P [frames][rows][G].
__global__ __launch_bounds__(SE_CS_THREADS) void se_draw_sums_kernel(const float* __restrict__ belief, double* __restrict__ Rs,
                                                                     double* __restrict__ P, int frames, int rows, int G) {
    extern __shared__ __align__(16) float plane[];                  // [G j][G + 1]: a thread walks its own row, rows on distinct banks
    __shared__ double rsum[SE_CS_MAX_G];
    const int t = threadIdx.x, i = blockIdx.x, row = blockIdx.y;
    const int GG = G * G, pitch = G + 1;
    for (int f = blockIdx.z; f < frames; f += gridDim.z) {
        const size_t fr = (size_t)f * rows + row;
        const float* src = belief + (fr * G + i) * GG;
        for (int e = t; e < GG; e += SE_CS_THREADS) {
            const int j = e / G;
            plane[j * pitch + (e - j * G)] = src[e];
        }
        __syncthreads();
        if (t < G) {
            const float* p = plane + t * pitch;
            double acc = 0.0;
            for (int k = 0; k < G; ++k) acc = acc + (double)p[k];
            rsum[t] = acc;
            Rs[(fr * G + i) * G + t] = acc;
        }
        __syncthreads();
        if (t == 0) {
            double acc = 0.0;
            for (int j = 0; j < G; ++j) acc = acc + rsum[j];
            P[fr * G + i] = acc;
        }
        __syncthreads();                                            // the next frame of this workgroup writes plane and rsum again
    }
}

// the launch, for rows in 1..65535 and G in 2..128 (checked by the caller)
inline int se_draw_sums_launch(const float* belief, double* Rs, double* P, int frames, int rows, int G, hipStream_t s) {
    SE_ENSURE_LDS(se_draw_sums_kernel, SE_CS_MAX_G * (SE_CS_MAX_G + 1) * 4);
    hipLaunchKernelGGL(se_draw_sums_kernel, dim3(G, rows, min(frames, SE_CS_MAX_Z)), dim3(SE_CS_THREADS), G * (G + 1) * 4, s, belief, Rs,
                       P, frames, rows, G);
    SE_CHECK_LAUNCH();
    return 0;
}

}  // namespace
