// Pose samples: ancestral draws of whole poses from the posterior of the skeleton model (sceneego_amd/skeleton_prior.py:
// SkeletonPrior.sample).  No counterpart in the reference.  include/sceneego_hip.h states the definition operation by operation;
// tests/skeleton_sampler_model.py restates it in numpy float64 and every index and kind written here is compared with it bit for bit.
// This file is built with -ffp-contract=off: one rounding per operation, every sum sequential in ascending index.
//
// The posterior of se_skeleton_couple_f32's model is prod_j p_j(x_j) prod_c F_c(x_parent(c), x_c), normalised, with the edge factor
// F_c(x, y) = (1 - floor) w_c(y - x) + floor / N.  With the upward products A_j = p_j prod_{c in ch(j)} U_c ancestral sampling is exact:
//     x_0 ~ A_0;   x_c ~ A_c(y) F_c(x_parent(c), y)  for c = 1..J-1 ascending (parent[c] < c).
// The child is y = x + d with weight taps[c][d]: CORRELATE's own orientation, no tap reversal.
//
// se_skeleton_upward_f32 runs the upward pass on skeleton_prior.hip's own kernels (sk_upward_walk there: the third mode of sk_walk).
// se_skeleton_sample_f32 is two launches:
//   se_draw_sums_kernel (categorical_sums.h, shared with volume_sample.hip), rows = J: Rs and P of every (frame, joint) in float64.
//   sks_walk_kernel   grid (samples, frames), block 256: one workgroup per pose, looping over the joints in ascending order
//                     INSIDE the launch: poses are independent, so there is no launch per joint and no grid-wide dependency.  Per
//                     joint: P into LDS and its running sums (thread 0: total_j is their last entry); where the joint is linked (its
//                     parent's voxel x is valid) the threads take the (di, dj) rows of the clipped window - at R = 24 at most 49^2 rows
//                     of at most 49 taps - and each sums its row's products (double)A_c(x + d) (double)taps[c][d] over ascending dk
//                     into r[di][dj] in LDS (49^2 doubles, 19.2 KB; a zero tap gives exactly 0 whatever A_c holds there); the lanes of
//                     the second wave form q[di]; thread 0 takes the two Philox blocks of (sample, frame, joint), decides step, jump
//                     or fresh draw and walks q, r[di][.] and the re-formed products of the row (di, dj).  A global draw (root, jump,
//                     fresh) stages Rs[i][.] and A[i][j][.] over the threads for thread 0's two further levels, as vsm_walk_kernel
//                     does.  The drawn voxels of the pose live in LDS (32 ints).
// No atomics; index and kind are written by thread 0 of the one workgroup that owns them, with plain vector stores.
//
// LDS of the walk: r 19,208 B, q 392 B, vals and cP 1,024 B each, the pose 128 B: 21.8 KB, seven workgroups per CU.  The draws are
// called, not inlined (sks_draw, sks_scan, sks_search below): 56 VGPRs, no scratch, no spill of either kind.  A thread's row loop reads the tap and the
// value of every dk without a branch (the product is selected, not skipped), so the loads of a row can be in flight together; the row
// is a sequential chain of at most 49 float64 additions.
//
// BYTE MODEL.  The sums pass reads `upward` once and writes 8 (G^2 + G) B per frame and joint.  The walk reads per pose and linked joint
// the clipped window of A_c and of the taps, at most (2R+1)^3 floats each: 14 x 37^3 x 4 B = 2.8 MB of A per pose at 15 x 64^3, R = 18,
// out of volumes the upward pass just wrote; a global draw reads G doubles of P and Rs and G floats of A.
//
// ORDER.  Every sum is sequential in ascending index and every product is rounded on its own (the window products are exact: two
// float32 factors), so the values depend on the inputs alone: bitwise identical from run to run, independent of how the frames are
// cut into calls and of how the samples are split over calls (the Philox counter holds the GLOBAL sample and frame index).
#include <float.h>

#include "categorical_draw.h"
#include "categorical_sums.h"    // se_draw_sums_kernel, the sums pass: shared with volume_sample.hip
#include "skeleton_shell.h"      // the limits, SkTree, the tree check and sk_upward_walk: shared with skeleton_prior.hip

#pragma clang fp contract(off)

#define SKS_THREADS 256
#define SKS_WIN (2 * SK_MAX_R + 1)                // the taps of an axis at most
#define SKS_MAX_Y 65535                           // grid.y of the walk; the frames beyond go to grid.z

namespace {

// The draws of categorical_draw.h, out of line: the walk makes seven of them per joint, and inlined they keep so many loop masks and
// bounds in scalar registers beside the kernel's pointers that the compiler parks scalars in vector lanes.  One body each, called
// (no stack: every array is in LDS, and so is the scan's second result), leaves the kernel without any spill.
__device__ __noinline__ double sks_scan(double* v, int n, int* last) { return se_draw_scan(v, n, last); }
__device__ __noinline__ int sks_search(const double* c, int n, int last, double total, double u) {
    return se_draw_search(c, n, last, total, u);
}
__device__ __noinline__ int sks_draw(double* v, int n, double u) { return se_draw(v, n, u); }

// the product of one tap: exactly 0 under a zero tap, whatever the volume holds there
__device__ __forceinline__ double sks_term(float a, float w) { return w != 0.f ? (double)a * (double)w : 0.0; }

// grid (samples, min(frames, 65535), ceil(frames / 65535)), block 256: frame = y + 65535 z
__global__ __launch_bounds__(SKS_THREADS) void sks_walk_kernel(const float* __restrict__ upward, const int* __restrict__ valid,
                                                               const float* __restrict__ taps, const double* __restrict__ Rs,
                                                               const double* __restrict__ P, int* __restrict__ index,
                                                               int* __restrict__ kind, SkTree tree, int frames, int G, int R,
                                                               float keepf, float uniformf, uint32_t first_sample,
                                                               uint32_t first_frame, uint32_t seed_lo, uint32_t seed_hi) {
    __shared__ double vals[SK_MAX_G];                               // the values of one level, then their running sums
    __shared__ double cP[SK_MAX_G];                                 // P of the joint, then its running sums
    __shared__ double r[SKS_WIN * SKS_WIN];                         // r[di][dj] of the window
    __shared__ double q[SKS_WIN];
    __shared__ int pose[SK_MAX_J];                                  // the voxels drawn so far, -1 where invalid
    __shared__ int lastPs;                                          // the last m with P[m] > 0: thread 0 alone, through sks_scan
    __shared__ int sh[4];                                           // thread 0's decisions: kind, i, j, the joint's voxel
    const int t = threadIdx.x, s = blockIdx.x;
    const int J = tree.J, GG = G * G, voxels = GG * G, W = 2 * R + 1;
    {
        const int f = blockIdx.y + blockIdx.z * SKS_MAX_Y;               // uniform
        if (f >= frames) return;
        const size_t o = ((size_t)s * frames + f) * J;
        if (valid != nullptr && valid[f] == 0) {                    // uniform: nothing of `upward` is read
            if (t < J) { index[o + t] = -1; kind[o + t] = 2; }
            return;
        }
        for (int j = 0; j < J; ++j) {
            __syncthreads();                                        // pose[] of the joints before; the joint before has read its LDS
            const int x = j > 0 ? pose[tree.parent[j]] : -1;        // the parent's voxel; -1: the root, or a parent without a draw
            const size_t fj = (size_t)f * J + j;
            const float* a = upward + fj * voxels;
            const double* Pf = P + fj * G;
            const double* Rf = Rs + fj * GG;
            const float* wt = taps + j * (W * W * W);                // at most 32 x 49^3: an int
            int xi = 0, xj = 0, xk = 0, loi = 0, loj = 0, lok = 0, ni = 0, nj = 0, nk = 0;
            if (t < G) cP[t] = Pf[t];
            if (x >= 0) {                                           // the window of x, clipped to the grid: y = x + d
                xi = x / GG; xj = (x / G) % G; xk = x % G;
                loi = max(-R, -xi); ni = min(R, G - 1 - xi) - loi + 1;
                loj = max(-R, -xj); nj = min(R, G - 1 - xj) - loj + 1;
                lok = max(-R, -xk); nk = min(R, G - 1 - xk) - lok + 1;
                for (int e = t; e < ni * nj; e += SKS_THREADS) {
                    const int ai = e / nj, c = e - ai * nj;
                    const float* src = a + ((xi + loi + ai) * G + (xj + loj + c)) * G + xk;
                    const float* w = wt + ((loi + ai + R) * W + (loj + c + R)) * W + R;
                    double acc = 0.0;
#pragma unroll 4
                    for (int d = lok; d < lok + nk; ++d) acc = acc + sks_term(src[d], w[d]);
                    r[ai * SKS_WIN + c] = acc;
                }
            }
            __syncthreads();
            double total = 0.0, u2 = 0.0, u3 = 0.0;
            if (t == 0) total = sks_scan(cP, G, &lastPs);           // total_j: the last running sum
            if (x >= 0 && t >= 64 && t - 64 < ni) {                 // q[di] on the second wave, beside thread 0's scan
                const int ai = t - 64;
                double acc = 0.0;
                for (int c = 0; c < nj; ++c) acc = acc + r[ai * SKS_WIN + c];
                q[ai] = acc;
            }
            __syncthreads();
            if (t == 0) {
                const uint32_t cs = first_sample + (uint32_t)s, cf = first_frame + (uint32_t)f;
                const SePhilox4 b0 = se_philox4x32_10(cs, cf, (uint32_t)j, 0u, seed_lo, seed_hi);
                const SePhilox4 b1 = se_philox4x32_10(cs, cf, (uint32_t)j, 1u, seed_lo, seed_hi);
                const double u0 = se_uniform53(b0.x[0], b0.x[1]), u1 = se_uniform53(b0.x[2], b0.x[3]);
                u2 = se_uniform53(b1.x[0], b1.x[1]);
                u3 = se_uniform53(b1.x[2], b1.x[3]);
                int mode = 2, y = -1;                               // 0 a step, 1 a jump, 2 a fresh draw
                if (x >= 0) {
                    double Wsum = 0.0;
                    for (int ai = 0; ai < ni; ++ai) Wsum = Wsum + q[ai];
                    const double step = (double)keepf * Wsum, jump = (double)uniformf * total, mass = step + jump;
                    if (se_draw_mass_ok(mass)) mode = (u0 * mass >= step) ? 1 : 0;
                }
                // the window draw: di, then dj, then dk (each level only where the one before gave a draw)
                int ai = -1, c = -1, m = -1;
                if (mode == 0) {
                    for (int e = 0; e < ni; ++e) vals[e] = q[e];
                    ai = sks_draw(vals, ni, u1);
                }
                if (ai >= 0) {
                    for (int e = 0; e < nj; ++e) vals[e] = r[ai * SKS_WIN + e];
                    c = sks_draw(vals, nj, u2);
                }
                if (c >= 0) {
                    const float* src = a + ((xi + loi + ai) * G + (xj + loj + c)) * G + xk;
                    const float* w = wt + ((loi + ai + R) * W + (loj + c + R)) * W + R;
                    for (int e = 0; e < nk; ++e) vals[e] = sks_term(src[lok + e], w[lok + e]);
                    m = sks_draw(vals, nk, u3);
                }
                if (m >= 0) y = ((xi + loi + ai) * G + (xj + loj + c)) * G + xk + lok + m;
                sh[1] = mode == 0 ? -1 : sks_search(cP, G, lastPs, total, u1);   // the global draw: i from P
                sh[0] = mode;
                sh[3] = y;
            }
            __syncthreads();
            if (sh[0] != 0 && sh[1] >= 0) {                         // uniform: j from Rs[i][.], then k from A[i][j][.]
                const int i = sh[1];
                if (t < G) vals[t] = Rf[i * G + t];
                __syncthreads();
                if (t == 0) sh[2] = sks_draw(vals, G, u2);
                __syncthreads();
                const int jj = sh[2];
                if (jj >= 0) {                                      // uniform
                    if (t < G) vals[t] = (double)a[(i * G + jj) * G + t];
                    __syncthreads();
                    if (t == 0) {
                        const int k = sks_draw(vals, G, u3);
                        sh[3] = k >= 0 ? (i * G + jj) * G + k : -1;
                    }
                    __syncthreads();
                }
            }
            if (t == 0) {                                           // an invalid draw (-1) links nothing below it
                pose[j] = sh[3];
                index[o + j] = sh[3];
                kind[o + j] = sh[0];
            }
        }
    }
}
static_assert(SK_MAX_J <= SKS_THREADS && SK_MAX_G <= SKS_THREADS && SKS_WIN <= 64, "a thread per joint, per entry of a level, a lane per q");

}  // namespace

extern "C" long long se_skeleton_upward_scratch_bytes(int frames, int J, int G, int R) { return sk_upward_scratch_bytes(frames, J, G, R); }

extern "C" int se_skeleton_upward_f32(const float* prob, const float* taps, const int* parent, float* upward, float* sums, int* valid,
                                      void* scratch, long long scratch_bytes, int frames, int J, int voxels, int G, int R, float floor,
                                      void* stream) {
    if (!prob || !taps || !parent || !upward || !sums || !valid || !scratch) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, taps, upward, sums, valid, scratch}, 4) || prob == upward) return SE_ERR_BAD_ARG;
    const long long need = sk_upward_scratch_bytes(frames, J, G, R);
    if (need <= 0 || scratch_bytes < need) return SE_ERR_BAD_ARG;
    return sk_upward_walk(prob, taps, parent, upward, sums, valid, scratch, frames, J, voxels, G, R, floor, stream);
}

// Rs [frames][J][G][G] and P [frames][J][G], float64
extern "C" long long se_skeleton_sample_scratch_bytes(int frames, int J, int G) {
    if (frames < 1 || J < 1 || J > SK_MAX_J || G < 2 || G > SK_MAX_G) return 0;
    const long long per_row = ((long long)G * G + G) * 8;           // <= 132,096
    if ((long long)frames > (1LL << 62) / per_row / J) return 0;
    return (long long)frames * J * per_row;
}

extern "C" int se_skeleton_sample_f32(const float* upward, const int* valid, const float* taps, const int* parent, int* index, int* kind,
                                      void* scratch, long long scratch_bytes, int frames, int J, int voxels, int G, int R, float floor,
                                      int samples, long long first_sample, long long first_frame, unsigned int seed_lo,
                                      unsigned int seed_hi, void* stream) {
    if (!upward || !taps || !parent || !index || !kind || !scratch) return SE_ERR_BAD_ARG;
    if (frames < 1 || samples < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R)) return SE_ERR_BAD_ARG;
    if ((long long)G * G * G != (long long)voxels) return SE_ERR_BAD_ARG;
    if (!(floor >= 0.f && floor <= 1.f)) return SE_ERR_BAD_ARG;     // a NaN fails
    SkTree tree{};
    int depth[SK_MAX_J], deepest;
    if (!sk_build_tree(parent, J, tree, depth, deepest)) return SE_ERR_BAD_ARG;
    // the counter words are 32 bits: every global sample and frame index of the call fits
    if (first_sample < 0 || first_sample + samples > (1LL << 32) || first_frame < 0 || first_frame + frames > (1LL << 32))
        return SE_ERR_BAD_ARG;
    if (!se_aligned({upward, valid, taps, index, kind}, 4) || !se_aligned({scratch}, 8)) return SE_ERR_BAD_ARG;
    const long long need = se_skeleton_sample_scratch_bytes(frames, J, G);
    if (need <= 0 || scratch_bytes < need) return SE_ERR_BAD_ARG;
    hipStream_t st = se_stream(stream);
    double* Rs = reinterpret_cast<double*>(scratch);
    double* P = Rs + (size_t)frames * J * G * G;
    const float keep = 1.0f - floor, uniform = floor / (float)voxels; // float32, as the coupling forms them
    const int rc = se_draw_sums_launch(upward, Rs, P, frames, J, G, st);
    if (rc) return rc;
    hipLaunchKernelGGL(sks_walk_kernel, dim3(samples, min(frames, SKS_MAX_Y), (frames + SKS_MAX_Y - 1) / SKS_MAX_Y), dim3(SKS_THREADS), 0, st, upward, valid, taps, Rs, P, index,
                       kind, tree, frames, G, R, keep, uniform, (uint32_t)first_sample, (uint32_t)first_frame,
                       (uint32_t)seed_lo, (uint32_t)seed_hi);
    SE_CHECK_LAUNCH();
    return 0;
}
