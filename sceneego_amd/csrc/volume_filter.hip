// Grid Bayes filter over the softmaxed joint volumes of a sequence (sceneego_amd/volume_filter.py: VolumeFilter;
// VoxelNetwork_depth.volume_filter returns one).  No counterpart in the reference.  include/sceneego_hip.h states the definition;
// tests/volume_filter_model.py restates it in float64.
//
// Per frame and row (one joint of one track), with the belief b of the frame before in `state`:
//     q = blur3(b)                    separable, taps w[-R..R], along k, then j, then i; zero-padded
//     u = (1 - floor) q + floor / N
//     a = p u,  Z = sum a,  b' = a / Z          or, without a prior or with a Z that is not a finite number > 0:  b' = p (restart)
// The frames of a call run one after the other on the stream: three launches per frame.
//   vf_blur_kj_kernel   grid (G, rows), block 256: one i-plane [G j][G k] of b staged in LDS, blurred along k into a second LDS
//                       plane, blurred along j from there and written to q (scratch).  2 G^2 floats of LDS: 32 KB at 64^3, 128 KB at 128^3.
//   vf_update_kernel    grid (G, rows), block 256: the slab [G i][G k] of q at one j staged in LDS (G^2 floats), blurred along i, then the
//                       floor and the product with p; a overwrites q in place (a workgroup writes only what it staged itself).  The
//                       workgroup's sums Z, sum a c (3) and sum p c (3, the joint of a restart) go to one record of 8 floats.
//   vf_finish_kernel    grid (chunks, rows), block 256: every workgroup folds the row's G records in the same fixed order (so all of them
//                       hold the same Z, bit for bit), decides the restart and writes its share of b' = a / Z, or of the copy of p,
//                       to `state` and `belief_out`; chunk 0 also writes joints, evidence and restarted.
// A thread owns column k of the staged plane and every (256 / W)-th row of it, W the power of two >= G: any G in 2..128, no vector access
// in the two plane kernels (rows of G floats are read whole by neighbouring lanes).  The finish pass moves 16 bytes per lane when
// voxels is a multiple of 4 and one float otherwise.
//
// BYTE MODEL per frame, row and voxel (float32): blur_kj reads b and writes q (8 B); update reads q and p and writes a (12 B; the
// coordinates, 12 B per voxel, are shared by all rows and stay in L2); finish reads a and writes b' (8 B): 28 B, and 4 B more when
// the beliefs are returned.  The records are G x 32 B per row.  At 64^3 and 15 rows that is 110 MB per frame over a working set
// (b, q, p: 47 MB) that does not fit the L2 but largely fits the Infinity Cache.  A restarted row reads p instead of a in the finish pass.
//
// SUMMATION ORDER.  No atomics.  A thread adds its voxels in ascending row order (G W / 256 <= 64 terms); the workgroup fold and the
// record fold are those of row_reduce.h: the wave folds by a butterfly (6), the four waves as (0 + 1) + (2 + 3) (2); the finish pass
// gives lane l the records l and l + 64 (2) and folds the lanes by a butterfly (6).  L = 64 + 6 + 2 + 2 + 6 = 80 sequential float32
// additions on the longest path of Z and of the joint sums (SE_VF_CHAIN; G = 128).  Every order depends on the shape alone: the
// results are bitwise identical from run to run, and since a frame sees only `state` and its own p they do not depend on how the
// frames are cut into calls.
//
// THE SMOOTHER (se_volume_smooth_f32; sceneego_amd/volume_smoother.py: VolumeSmoother; tests/volume_smoother_model.py) walks the frames
// of a call from last to first with a backward belief r in `state`.  Frame t is LINKED to t + 1 unless restarted[t + 1] is set (for the
// call's last frame: unless have_link says so); with b_t the filtered belief and blur3T the blur with the taps reversed (the adjoint):
//     u = (1 - floor) blur3T(r_{t+1}) + floor / N
//     g = b_t u,  S = sum g,  gamma_t = g / S         or, unlinked or with an S that is not a finite number > 0:  gamma_t = b_t (a copy)
//     a = p_t u,  s = sum a,  r_t = a / s             or, unlinked or with an s that is not a finite number > 0:  r_t = p_t (a copy)
// Three launches per frame again, after one launch per call (vs_prep_kernel) that writes the reversed taps into the scratch:
//   vf_blur_kj_kernel   the kernel above on r with the reversed taps; its have_prior is the frame's link flags.
//   vs_update_kernel    vf_update_kernel with two products from the one u: a overwrites q in place, g goes to a second array (only when
//                       gamma is asked for); the record holds s, S, sum g c (3) and sum b c (3, the joint of an unlinked row).
//   vs_finish_kernel    folds the records, decides the two fallbacks apart, writes r_t to `state` and gamma_t to `smoothed_out` (which may
//                       be `belief` itself: the frame's b was read by the update pass, and a copy onto itself is skipped); chunk 0 also
//                       writes joints, agreement, smoothed and the link flags of the frame processed next (!restarted[t], two arrays in
//                       turn so that no workgroup of this launch reads what another writes).
// BYTE MODEL per frame, row and voxel: blur_kj 8 B (r, q); update reads q, p and b and writes a (16 B), and g (4 B) when gamma is asked for;
// finish reads a and writes r (8 B), and reads g and writes gamma (8 B) when asked for: 32 B, 44 B with the smoothed beliefs, over a
// working set of r, q, p, b (and g): 63 MB (79 MB) at 64^3 and 15 rows, 126 MB (173 MB) moved per frame.
// SUMMATION ORDER: that of the filter, for s, S and the joint sums alike: L = 80 (SE_VS_CHAIN).  A frame sees only `state`, its link
// flags and its own p and b, so the results do not depend on how the frames are cut into calls.
//
// THE TRANSITION STATISTICS (se_volume_transition_stats_f32; sceneego_amd/motion_fit.py: MotionModelFit; tests/motion_fit_model.py) are
// the smoother's backward walk with the E-step sums of a Baum-Welch fit of (sigma, floor) in place of gamma.  With w' the reversed taps,
// m'[d] = (float)(d d) w'[d] and blur3(x; wk, wj, wi) the blur with a tap vector per axis, for a linked frame t:
//     q0 = blur3(r_{t+1}; w', w', w')
//     q2 = blur3(r_{t+1}; m', w', w') + blur3(r_{t+1}; w', m', w') + blur3(r_{t+1}; w', w', m')       the squared step, voxels^2
//     u = (1 - floor) q0 + floor / N,  a = p_t u,  s = sum a,  r_t = a / s       the smoother's, bit for bit
//     stats = { S = sum b_t u,  s,  A0 = sum b_t q0,  A2 = sum b_t q2,  Bsum = sum b_t,  Rsum = sum r_{t+1} }
// Three launches per frame, after one per call (ts_prep_kernel: w' and m' into the scratch):
//   ts_blur_kj_kernel   grid (G, rows), block 256: vf_blur_kj_kernel with two outputs per i-plane, P0 = blur_j(w') blur_k(w') r (the
//                       smoother's q) and P1 = blur_j(w') blur_k(m') r + blur_j(m') blur_k(w') r.  The staged plane and the two k-blurred
//                       planes are 3 G^2 floats: 48 KB at 64^3.  Above G = 116 that passes the 160 KB of a CU, and the k-blurred planes
//                       are formed for one half of the columns at a time ((G + 2 ceil(G / 2)) G floats: 128 KB at 128^3); a column's
//                       values do not depend on the split.  The plane's sum (Rsum) goes to slot 5 of record i of the row.
//   ts_update_kernel    grid (G, rows), block 256: the slabs of P0 and P1 at one j staged in LDS (2 G^2 floats), q0 = blur_i(w') P0 and
//                       q2 = blur_i(m') P0 + blur_i(w') P1, then the floor and the products; a overwrites P0 in place; the record
//                       holds s, S, A0, A2, Bsum in slots 0..4 (record j of the row; slot 5 is the blur pass's).
//   ts_finish_kernel    folds the records, decides the fallback, writes r_t to `state`; chunk 0 also writes the six stats (NaN for an
//                       unlinked row), `linked` and the link flags of the frame processed next.
// An unlinked row is skipped by the first two launches and copied (r_t = p_t) by the third.
// BYTE MODEL per frame, row and voxel: blur_kj reads r and writes P0 and P1 (12 B); update reads P0, P1, p and b and writes a (20 B);
// finish reads a and writes r (8 B): 40 B, the smoother's 32 B plus P1 written and read, over a working set of r, P0, P1, p, b: 79 MB at
// 64^3 and 15 rows, 157 MB moved per frame.
// SUMMATION ORDER: that of the filter for all six sums: L = 80 (SE_TS_CHAIN).  s and S are the sums of the same values in the same
// order as the smoother's, so `state` and S equal the smoother's `state` and `agreement` bit for bit.
#include <float.h>

#include "row_reduce.h"
#include "volume_grid.h"          // the limits, the shape predicate, the launch parameters and the argument gate: shared with volume_viterbi.hip

#define SE_VF_PART 8              // Z, sum a c (x y z), sum p c (x y z), pad
#define SE_VF_CHAIN 80            // L of the header comment
#define SE_VS_CHAIN 80            // the smoother's: the same fold over the same records
#define SE_TS_CHAIN 80            // the transition statistics': likewise
#define SE_TS_STATS 6             // S, s, A0, A2, Bsum, Rsum
#define SE_TS_LDS_MAX (160 * 1024 - 1024)   // the most dynamic LDS of a workgroup: a CU's 160 KB less 1 KB for the static arrays (392 B)

namespace {

__device__ __forceinline__ bool vf_has_prior(const int* __restrict__ have_prior, int prior_all, int row) {
    return prior_all || (have_prior != nullptr && have_prior[row] != 0);
}

// What the update kernels of the filter and of the smoother share.  Thread t owns column k = t & (W - 1) of the slab and the rows
// ir, ir + RP, ... of it (ir = t >> wshift, RP = 256 >> wshift).
// The slab [G i][G k] of q at one j and the taps, staged by the whole workgroup; the caller's __syncthreads() follows.
__device__ __forceinline__ void vf_stage_slab(const float* __restrict__ q, const float* __restrict__ taps, float* __restrict__ slab,
                                              float* __restrict__ w, size_t base, int j, int G, int R, int t, int k, int ir, int RP) {
    if (k < G)
        for (int i = ir; i < G; i += RP) slab[i * G + k] = q[base + ((size_t)i * G + j) * G + k];
    if (t <= 2 * R) w[t] = taps[t];
}
// u of voxel (i, k) of the staged slab: the blur along i over the taps that stay inside the grid, in ascending d, then the floor
__device__ __forceinline__ float vf_blur_i_floor(const float* __restrict__ slab, const float* __restrict__ w, int i, int k, int G, int R,
                                                 float keep, float uniform) {
    const int lo = max(-R, -i), hi = min(R, G - 1 - i);
    const float* s = slab + i * G + k;
    float u = 0.f;
    for (int d = lo; d <= hi; ++d) u = fmaf(w[d + R], s[d * G], u);
    return fmaf(keep, u, uniform);
}

// What the finish kernels share.
// Wave 0 folds the first NV values of the row's G records into fin[]; every thread of the workgroup may read fin[] on return.
template <int NV>
__device__ __forceinline__ void vf_fold_records(const float* __restrict__ part, int row, int G, int t, float* __restrict__ fin) {
    if (t < 64) {
        float acc[NV];
#pragma unroll
        for (int x = 0; x < NV; ++x) acc[x] = 0.f;
        wave_fold_records<NV, SE_VF_PART>(part, (size_t)row * G, G, t, acc);
        if (t == 0) {
#pragma unroll
            for (int x = 0; x < NV; ++x) fin[x] = acc[x];
        }
    }
    __syncthreads();
}
// The row pass of a finish kernel: this workgroup's share of a row of `voxels` floats, for each of NS streams dst = src / Z (scale) or
// the copy of src, bit for bit; `out` (or NULL) receives the same values; a stream without src is skipped.  16 bytes per lane (VEC)
// or one float at a time.  The streams take turns inside one loop, so that the loads of the smoother's two are in flight together.
struct VfStream {
    const float* src;
    bool scale;
    float Z;
    float* dst;
    float* out;
};
template <bool VEC, int NS>
__device__ __forceinline__ void vf_scale_or_copy(const VfStream (&st)[NS], int voxels, int t) {
    for (int n = (blockIdx.x * SE_VG_THREADS + t) * 4; n < voxels; n += gridDim.x * SE_VG_THREADS * 4) {
        if (VEC) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (!st[s].src) continue;
                f32x4 x = *reinterpret_cast<const f32x4*>(st[s].src + n);
                if (st[s].scale) { x.x = x.x / st[s].Z; x.y = x.y / st[s].Z; x.z = x.z / st[s].Z; x.w = x.w / st[s].Z; }
                *reinterpret_cast<f32x4*>(st[s].dst + n) = x;
                if (st[s].out) *reinterpret_cast<f32x4*>(st[s].out + n) = x;
            }
        } else {
            for (int e = n; e < min(n + 4, voxels); ++e) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (!st[s].src) continue;
                    float x = st[s].src[e];
                    if (st[s].scale) x = x / st[s].Z;
                    st[s].dst[e] = x;
                    if (st[s].out) st[s].out[e] = x;
                }
            }
        }
    }
}

// grid (G, rows), block 256, dynamic LDS 2 G^2 floats
__global__ __launch_bounds__(SE_VG_THREADS) void vf_blur_kj_kernel(const float* __restrict__ state, const float* __restrict__ taps,
                                                                   const int* __restrict__ have_prior, int prior_all,
                                                                   float* __restrict__ q, int G, int voxels, int R, int wshift) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float w[2 * SE_VG_MAX_R + 1];
    const int t = threadIdx.x, i = blockIdx.x, row = blockIdx.y;
    if (!vf_has_prior(have_prior, prior_all, row)) return;          // uniform: the row restarts, q is not read
    const int GG = G * G;
    float* A = lds;
    float* Bk = lds + GG;
    const size_t base = (size_t)row * voxels + (size_t)i * GG;
    for (int e = t; e < GG; e += SE_VG_THREADS) A[e] = state[base + e];
    if (t <= 2 * R) w[t] = taps[t];
    __syncthreads();
    const int k = t & ((1 << wshift) - 1), jr = t >> wshift, RP = SE_VG_THREADS >> wshift;
    if (k < G) {
        const int lo = max(-R, -k), hi = min(R, G - 1 - k);         // the taps that stay inside the row
        for (int j = jr; j < G; j += RP) {
            const float* a = A + j * G + k;
            float acc = 0.f;
            for (int d = lo; d <= hi; ++d) acc = fmaf(w[d + R], a[d], acc);
            Bk[j * G + k] = acc;
        }
    }
    __syncthreads();
    if (k < G) {
        for (int j = jr; j < G; j += RP) {
            const int lo = max(-R, -j), hi = min(R, G - 1 - j);
            const float* b = Bk + j * G + k;
            float acc = 0.f;
            for (int d = lo; d <= hi; ++d) acc = fmaf(w[d + R], b[d * G], acc);
            q[base + j * G + k] = acc;
        }
    }
}

// grid (G, rows), block 256, dynamic LDS G^2 floats
__global__ __launch_bounds__(SE_VG_THREADS) void vf_update_kernel(const float* __restrict__ prob, const float* __restrict__ coord,
                                                                  const float* __restrict__ taps, const int* __restrict__ have_prior,
                                                                  int prior_all, float* __restrict__ q, float* __restrict__ part,
                                                                  int G, int voxels, int R, int wshift, float keep, float uniform) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float w[2 * SE_VG_MAX_R + 1];
    __shared__ float sm[4][SE_VF_PART];
    const int t = threadIdx.x, j = blockIdx.x, row = blockIdx.y;
    const bool prior = vf_has_prior(have_prior, prior_all, row);    // uniform
    const int k = t & ((1 << wshift) - 1), ir = t >> wshift, RP = SE_VG_THREADS >> wshift;
    const size_t base = (size_t)row * voxels;
    if (prior) vf_stage_slab(q, taps, lds, w, base, j, G, R, t, k, ir, RP);
    __syncthreads();
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};            // Z, sum a c, sum p c
    if (k < G) {
        for (int i = ir; i < G; i += RP) {
            const size_t n = ((size_t)i * G + j) * G + k;
            const float p = prob[base + n];
            const float cx = coord[n * 3 + 0], cy = coord[n * 3 + 1], cz = coord[n * 3 + 2];
            acc[4] += p * cx; acc[5] += p * cy; acc[6] += p * cz;
            if (prior) {
                const float u = vf_blur_i_floor(lds, w, i, k, G, R, keep, uniform);
                const float a = p * u;
                q[base + n] = a;                                    // staged by this workgroup, read by no other
                acc[0] += a;
                acc[1] += a * cx; acc[2] += a * cy; acc[3] += a * cz;
            }
        }
    }
    block_fold_stage<7, SE_VF_PART>(acc, sm);
    if (t < 7) part[((size_t)row * G + j) * SE_VF_PART + t] = block_fold_sum<SE_VF_PART>(sm, t);
}

// grid (chunks, rows), block 256
template <bool VEC>
__global__ __launch_bounds__(SE_VG_THREADS) void vf_finish_kernel(const float* __restrict__ prob, const float* __restrict__ q,
                                                                  const float* __restrict__ part, const int* __restrict__ have_prior,
                                                                  int prior_all, float* __restrict__ state,
                                                                  float* __restrict__ belief_out, float* __restrict__ joints,
                                                                  float* __restrict__ evidence, int* __restrict__ restarted, int G,
                                                                  int voxels) {
    __shared__ float fin[SE_VF_PART];
    const int t = threadIdx.x, row = blockIdx.y;
    vf_fold_records<7>(part, row, G, t, fin);
    const bool prior = vf_has_prior(have_prior, prior_all, row);
    const float Z = fin[0];
    const bool restart = !prior || !(Z > 0.f && Z <= FLT_MAX);      // a NaN fails both comparisons
    if (blockIdx.x == 0 && t == 0) {
        float* o = joints + (size_t)row * 3;
        if (restart) { o[0] = fin[4]; o[1] = fin[5]; o[2] = fin[6]; }
        else { o[0] = fin[1] / Z; o[1] = fin[2] / Z; o[2] = fin[3] / Z; }
        evidence[row] = prior ? Z : __int_as_float(0x7fc00000);
        restarted[row] = restart ? 1 : 0;
    }
    const size_t base = (size_t)row * voxels;
    // b' = a / Z, or the copy of p
    const VfStream st[1] = {{(restart ? prob : q) + base, !restart, Z, state + base, belief_out ? belief_out + base : nullptr}};
    vf_scale_or_copy<VEC>(st, voxels, t);
}

// one workgroup: the taps reversed (blur3T is blur3 with them), for the blur kernel above and the update kernel below
__global__ void vs_prep_kernel(const float* __restrict__ taps, float* __restrict__ rev, int R) {
    const int t = threadIdx.x;
    if (t <= 2 * R) rev[t] = taps[2 * R - t];
}

// grid (G, rows), block 256, dynamic LDS G^2 floats.  `taps`: already reversed.  `link`: the frame's link flags (or NULL: none).
// `g_out`: NULL when gamma is not asked for.
__global__ __launch_bounds__(SE_VG_THREADS) void vs_update_kernel(const float* __restrict__ prob, const float* __restrict__ belief,
                                                                  const float* __restrict__ coord, const float* __restrict__ taps,
                                                                  const int* __restrict__ link, float* __restrict__ q,
                                                                  float* __restrict__ g_out, float* __restrict__ part, int G, int voxels,
                                                                  int R, int wshift, float keep, float uniform) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float w[2 * SE_VG_MAX_R + 1];
    __shared__ float sm[4][SE_VF_PART];
    const int t = threadIdx.x, j = blockIdx.x, row = blockIdx.y;
    const bool linked = vf_has_prior(link, 0, row);                 // uniform
    const int k = t & ((1 << wshift) - 1), ir = t >> wshift, RP = SE_VG_THREADS >> wshift;
    const size_t base = (size_t)row * voxels;
    if (linked) vf_stage_slab(q, taps, lds, w, base, j, G, R, t, k, ir, RP);
    __syncthreads();
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};       // s, S, sum g c, sum b c
    if (k < G) {
        for (int i = ir; i < G; i += RP) {
            const size_t n = ((size_t)i * G + j) * G + k;
            const float b = belief[base + n];
            const float cx = coord[n * 3 + 0], cy = coord[n * 3 + 1], cz = coord[n * 3 + 2];
            acc[5] += b * cx; acc[6] += b * cy; acc[7] += b * cz;
            if (linked) {
                const float p = prob[base + n];
                const float u = vf_blur_i_floor(lds, w, i, k, G, R, keep, uniform);
                const float a = p * u, g = b * u;
                q[base + n] = a;                                    // staged by this workgroup, read by no other
                if (g_out) g_out[base + n] = g;
                acc[0] += a;
                acc[1] += g;
                acc[2] += g * cx; acc[3] += g * cy; acc[4] += g * cz;
            }
        }
    }
    block_fold_stage<8, SE_VF_PART>(acc, sm);
    if (t < 8) part[((size_t)row * G + j) * SE_VF_PART + t] = block_fold_sum<SE_VF_PART>(sm, t);
}

// grid (chunks, rows), block 256.  No __restrict__ on belief / smoothed_out: they may be one array.
template <bool VEC>
__global__ __launch_bounds__(SE_VG_THREADS) void vs_finish_kernel(const float* __restrict__ prob, const float* belief,
                                                                  const float* __restrict__ q, const float* __restrict__ g,
                                                                  const float* __restrict__ part, const int* __restrict__ link,
                                                                  const int* __restrict__ restarted, int* __restrict__ link_next,
                                                                  float* __restrict__ state, float* smoothed_out,
                                                                  float* __restrict__ joints, float* __restrict__ agreement,
                                                                  int* __restrict__ smoothed, int G, int voxels) {
    __shared__ float fin[SE_VF_PART];
    const int t = threadIdx.x, row = blockIdx.y;
    vf_fold_records<8>(part, row, G, t, fin);
    const bool linked = vf_has_prior(link, 0, row);
    const float s = fin[0], S = fin[1];
    const bool back = linked && s > 0.f && s <= FLT_MAX;            // r_t = a / s; a NaN fails both comparisons
    const bool smooth = linked && S > 0.f && S <= FLT_MAX;          // gamma_t = g / S
    if (blockIdx.x == 0 && t == 0) {
        float* o = joints + (size_t)row * 3;
        if (smooth) { o[0] = fin[2] / S; o[1] = fin[3] / S; o[2] = fin[4] / S; }
        else { o[0] = fin[5]; o[1] = fin[6]; o[2] = fin[7]; }
        agreement[row] = linked ? S : __int_as_float(0x7fc00000);
        smoothed[row] = smooth ? 1 : 0;
        link_next[row] = restarted[row] == 0;                       // the frame before this one is linked to it unless it restarted
    }
    const size_t base = (size_t)row * voxels;
    // r_t = a / s, or the copy of p_t; gamma_t = g / S, or the copy of b_t (skipped onto itself)
    const bool write_gamma = smoothed_out != nullptr && (smooth || smoothed_out != belief);
    const VfStream st[2] = {{(back ? q : prob) + base, back, s, state + base, nullptr},
                            {write_gamma ? (smooth ? g : belief) + base : nullptr, smooth, S, write_gamma ? smoothed_out + base : nullptr, nullptr}};
    vf_scale_or_copy<VEC>(st, voxels, t);
}

}  // namespace

extern "C" long long se_volume_filter_scratch_bytes(int rows, int G, int radius) {
    if (!vg_shape_ok(rows, G, radius)) return 0;
    return (vg_elems(rows, G) + (long long)rows * G * SE_VF_PART) * 4;
}

extern "C" int se_volume_filter_f32(const float* prob, const float* coord, const float* taps, float* state, float* belief_out,
                                    float* joints, float* evidence, int* restarted, void* scratch, long long scratch_bytes,
                                    int frames, int rows, int voxels, int G, int radius, float floor, const int* have_prior,
                                    void* stream) {
    if (!prob || !coord || !taps || !state || !joints || !evidence || !restarted || !scratch) return SE_ERR_BAD_ARG;
    if (!vg_args_ok(frames, rows, voxels, G, radius, floor)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, coord, taps, state, belief_out, joints, evidence, restarted, scratch, have_prior}, 4)) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_volume_filter_scratch_bytes(rows, G, radius)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    float* q = reinterpret_cast<float*>(scratch);
    float* part = q + vg_elems(rows, G);
    const auto [wshift, chunks, keep, uniform] = vg_launch(voxels, G, floor);
    const int plane_bytes = G * G * 4;
    SE_ENSURE_LDS(vf_blur_kj_kernel, 2 * SE_VG_MAX_G * SE_VG_MAX_G * 4);
    SE_ENSURE_LDS(vf_update_kernel, SE_VG_MAX_G * SE_VG_MAX_G * 4);
    // 16-byte moves in the finish pass: whole quads per row and every base it touches aligned
    const bool vec = (voxels & 3) == 0 && se_aligned({prob, state, belief_out, scratch}, 16);
    const auto finish = vec ? vf_finish_kernel<true> : vf_finish_kernel<false>;
    const size_t frame_elems = (size_t)rows * voxels;
    for (int f = 0; f < frames; ++f) {
        const float* p = prob + f * frame_elems;
        const int prior_all = f > 0;
        if (prior_all || have_prior) {
            hipLaunchKernelGGL(vf_blur_kj_kernel, dim3(G, rows), dim3(SE_VG_THREADS), 2 * plane_bytes, s, state, taps, have_prior,
                               prior_all, q, G, voxels, radius, wshift);
            SE_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(vf_update_kernel, dim3(G, rows), dim3(SE_VG_THREADS), plane_bytes, s, p, coord, taps, have_prior, prior_all,
                           q, part, G, voxels, radius, wshift, keep, uniform);
        SE_CHECK_LAUNCH();
        float* bo = belief_out ? belief_out + f * frame_elems : nullptr;
        hipLaunchKernelGGL(finish, dim3(chunks, rows), dim3(SE_VG_THREADS), 0, s, p, q, part, have_prior, prior_all, state, bo,
                           joints + (size_t)f * rows * 3, evidence + (size_t)f * rows, restarted + (size_t)f * rows, G, voxels);
        SE_CHECK_LAUNCH();
    }
    return 0;
}

// scratch of the smoother: q and g [rows][voxels], the records [rows][G][8], the reversed taps (40 floats), two arrays of link flags.
// g is reserved whether or not smoothed_out is given (the size is asked for before the call's arguments are known): a call without
// smoothed_out leaves it untouched, 15.7 MB of the workspace at 15 x 64^3 and 126 MB at 15 x 128^3.
inline long long vs_tail_elems(int rows, int G) { return (long long)rows * G * SE_VF_PART + 40 + 2LL * ((rows + 3) & ~3); }

extern "C" long long se_volume_smooth_scratch_bytes(int rows, int G, int radius) {
    if (!vg_shape_ok(rows, G, radius)) return 0;
    return (2 * vg_elems(rows, G) + vs_tail_elems(rows, G)) * 4;
}

extern "C" int se_volume_smooth_f32(const float* prob, const float* belief, const int* restarted, const float* coord, const float* taps,
                                    float* state, float* smoothed_out, float* joints, float* agreement, int* smoothed, void* scratch,
                                    long long scratch_bytes, int frames, int rows, int voxels, int G, int radius, float floor,
                                    const int* have_link, void* stream) {
    if (!prob || !belief || !restarted || !coord || !taps || !state || !joints || !agreement || !smoothed || !scratch)
        return SE_ERR_BAD_ARG;
    if (!vg_args_ok(frames, rows, voxels, G, radius, floor)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, belief, restarted, coord, taps, state, smoothed_out, joints, agreement, smoothed, scratch, have_link}, 4))
        return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_volume_smooth_scratch_bytes(rows, G, radius)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    float* q = reinterpret_cast<float*>(scratch);
    float* g = q + vg_elems(rows, G);
    float* part = g + vg_elems(rows, G);
    float* rev = part + (long long)rows * G * SE_VF_PART;
    int* link2 = reinterpret_cast<int*>(rev + 40);
    const int link_stride = (rows + 3) & ~3;
    const auto [wshift, chunks, keep, uniform] = vg_launch(voxels, G, floor);
    const int plane_bytes = G * G * 4;
    SE_ENSURE_LDS(vf_blur_kj_kernel, 2 * SE_VG_MAX_G * SE_VG_MAX_G * 4);
    SE_ENSURE_LDS(vs_update_kernel, SE_VG_MAX_G * SE_VG_MAX_G * 4);
    const bool vec = (voxels & 3) == 0 && se_aligned({prob, belief, state, smoothed_out, scratch}, 16);
    const auto finish = vec ? vs_finish_kernel<true> : vs_finish_kernel<false>;
    const size_t frame_elems = (size_t)rows * voxels;
    hipLaunchKernelGGL(vs_prep_kernel, dim3(1), dim3(64), 0, s, taps, rev, radius);
    SE_CHECK_LAUNCH();
    for (int f = frames - 1; f >= 0; --f) {
        const float* p = prob + f * frame_elems;
        const float* b = belief + f * frame_elems;
        // the link flags of frame f: the caller's for the last frame, else what the finish pass of frame f + 1 wrote
        const int* link = f == frames - 1 ? have_link : link2 + (size_t)(f & 1) * link_stride;
        int* link_next = link2 + (size_t)((f + 1) & 1) * link_stride;                    // read by frame f - 1
        if (link) {
            hipLaunchKernelGGL(vf_blur_kj_kernel, dim3(G, rows), dim3(SE_VG_THREADS), 2 * plane_bytes, s, state, rev, link, 0, q, G,
                               voxels, radius, wshift);
            SE_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(vs_update_kernel, dim3(G, rows), dim3(SE_VG_THREADS), plane_bytes, s, p, b, coord, rev, link, q,
                           smoothed_out ? g : nullptr, part, G, voxels, radius, wshift, keep, uniform);
        SE_CHECK_LAUNCH();
        float* so = smoothed_out ? smoothed_out + f * frame_elems : nullptr;
        const int* rs = restarted + (size_t)f * rows;
        hipLaunchKernelGGL(finish, dim3(chunks, rows), dim3(SE_VG_THREADS), 0, s, p, b, q, g, part, link, rs, link_next, state, so,
                           joints + (size_t)f * rows * 3, agreement + (size_t)f * rows, smoothed + (size_t)f * rows, G, voxels);
        SE_CHECK_LAUNCH();
    }
    return 0;
}

namespace {

// one workgroup: the taps reversed (w') and m'[d] = (float)(d d) w'[d]
__global__ void ts_prep_kernel(const float* __restrict__ taps, float* __restrict__ rev, float* __restrict__ msq, int R) {
    const int t = threadIdx.x;
    if (t <= 2 * R) {
        const float w = taps[2 * R - t];
        rev[t] = w;
        msq[t] = (float)((t - R) * (t - R)) * w;
    }
}

// grid (G, rows), block 256, dynamic LDS (G + 2 KW) G floats; KW = G, or ceil(G / 2) where three whole planes do not fit.  `rev`, `msq`:
// what ts_prep_kernel wrote.  `link`: the frame's link flags.
__global__ __launch_bounds__(SE_VG_THREADS) void ts_blur_kj_kernel(const float* __restrict__ state, const float* __restrict__ rev,
                                                                   const float* __restrict__ msq, const int* __restrict__ link,
                                                                   float* __restrict__ P0, float* __restrict__ P1,
                                                                   float* __restrict__ part, int G, int voxels, int R, int wshift,
                                                                   int KW) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float w[2 * SE_VG_MAX_R + 1];
    __shared__ float m[2 * SE_VG_MAX_R + 1];
    __shared__ float sm[4][SE_VF_PART];
    const int t = threadIdx.x, i = blockIdx.x, row = blockIdx.y;
    if (!vf_has_prior(link, 0, row)) return;                        // uniform: the row is copied, nothing of it is read
    const int GG = G * G;
    float* A = lds;
    float* B0 = lds + GG;                                           // blur_k(w') A, [G j][KW k]
    float* B1 = B0 + G * KW;                                        // blur_k(m') A
    const size_t base = (size_t)row * voxels + (size_t)i * GG;
    for (int e = t; e < GG; e += SE_VG_THREADS) A[e] = state[base + e];
    if (t <= 2 * R) { w[t] = rev[t]; m[t] = msq[t]; }
    __syncthreads();
    const int k = t & ((1 << wshift) - 1), jr = t >> wshift, RP = SE_VG_THREADS >> wshift;
    float rs[1] = {0.f};                                            // Rsum: this plane's share
    if (k < G)
        for (int j = jr; j < G; j += RP) rs[0] += A[j * G + k];
    for (int k0 = 0; k0 < G; k0 += KW) {                            // one pass, or two over halves of the columns
        const bool mine = k >= k0 && k < min(G, k0 + KW);
        if (mine) {
            const int lo = max(-R, -k), hi = min(R, G - 1 - k);     // the taps that stay inside the row
            for (int j = jr; j < G; j += RP) {
                const float* a = A + j * G + k;
                float acc = 0.f, acm = 0.f;
                for (int d = lo; d <= hi; ++d) {                    // one read of a[d] for both sums; each in ascending d
                    const float x = a[d];
                    acc = fmaf(w[d + R], x, acc);
                    acm = fmaf(m[d + R], x, acm);
                }
                B0[j * KW + k - k0] = acc;
                B1[j * KW + k - k0] = acm;
            }
        }
        __syncthreads();
        if (mine) {
            for (int j = jr; j < G; j += RP) {
                const int lo = max(-R, -j), hi = min(R, G - 1 - j);
                const float* b0 = B0 + j * KW + k - k0;
                const float* b1 = B1 + j * KW + k - k0;
                float acc = 0.f, ac1 = 0.f, acm = 0.f;
                for (int d = lo; d <= hi; ++d) {
                    const float x0 = b0[d * KW], x1 = b1[d * KW], wd = w[d + R];
                    acc = fmaf(wd, x0, acc);
                    ac1 = fmaf(wd, x1, ac1);
                    acm = fmaf(m[d + R], x0, acm);
                }
                P0[base + j * G + k] = acc;
                P1[base + j * G + k] = ac1 + acm;
            }
        }
        __syncthreads();                                            // the next pass writes B0 and B1 again
    }
    block_fold_stage<1, SE_VF_PART>(rs, sm);
    if (t == 0) part[((size_t)row * G + i) * SE_VF_PART + 5] = block_fold_sum<SE_VF_PART>(sm, 0);
}

// A product rounded on its own, never fused into the sum that follows it.  vs_update_kernel's a is stored and its g is used four times,
// and the compiler keeps both as products there; here g has one use and would be contracted into S.
__device__ __forceinline__ float ts_mul(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}

// grid (G, rows), block 256, dynamic LDS 2 G^2 floats.  q0 and u are formed as vs_update_kernel forms them (vf_blur_i_floor, with q0
// kept) and a and g are rounded products: s and S are the smoother's, bit for bit.
__global__ __launch_bounds__(SE_VG_THREADS) void ts_update_kernel(const float* __restrict__ prob, const float* __restrict__ belief,
                                                                  const float* __restrict__ rev, const float* __restrict__ msq,
                                                                  const int* __restrict__ link, float* __restrict__ P0,
                                                                  const float* __restrict__ P1, float* __restrict__ part, int G,
                                                                  int voxels, int R, int wshift, float keep, float uniform) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float w[2 * SE_VG_MAX_R + 1];
    __shared__ float m[2 * SE_VG_MAX_R + 1];
    __shared__ float sm[4][SE_VF_PART];
    const int t = threadIdx.x, j = blockIdx.x, row = blockIdx.y;
    if (!vf_has_prior(link, 0, row)) return;                        // uniform
    const int k = t & ((1 << wshift) - 1), ir = t >> wshift, RP = SE_VG_THREADS >> wshift;
    const size_t base = (size_t)row * voxels;
    float* slab0 = lds;
    float* slab1 = lds + G * G;
    vf_stage_slab(P0, rev, slab0, w, base, j, G, R, t, k, ir, RP);
    vf_stage_slab(P1, msq, slab1, m, base, j, G, R, t, k, ir, RP);
    __syncthreads();
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};                      // s, S, A0, A2, Bsum
    if (k < G) {
        for (int i = ir; i < G; i += RP) {
            const size_t n = ((size_t)i * G + j) * G + k;
            const float b = belief[base + n];
            const float p = prob[base + n];
            const int lo = max(-R, -i), hi = min(R, G - 1 - i);
            const float* s0 = slab0 + i * G + k;
            const float* s1 = slab1 + i * G + k;
            float q0 = 0.f, q2 = 0.f, qm = 0.f;
            for (int d = lo; d <= hi; ++d) {                        // q0 in vf_blur_i_floor's order
                const float x0 = s0[d * G], x1 = s1[d * G], wd = w[d + R];
                q0 = fmaf(wd, x0, q0);
                q2 = fmaf(wd, x1, q2);
                qm = fmaf(m[d + R], x0, qm);
            }
            q2 += qm;
            const float u = fmaf(keep, q0, uniform);
            const float a = ts_mul(p, u), g = ts_mul(b, u);
            P0[base + n] = a;                                       // staged by this workgroup, read by no other
            acc[0] += a;
            acc[1] += g;
            acc[2] += b * q0;
            acc[3] += b * q2;
            acc[4] += b;
        }
    }
    block_fold_stage<5, SE_VF_PART>(acc, sm);
    if (t < 5) part[((size_t)row * G + j) * SE_VF_PART + t] = block_fold_sum<SE_VF_PART>(sm, t);
}

// grid (chunks, rows), block 256
template <bool VEC>
__global__ __launch_bounds__(SE_VG_THREADS) void ts_finish_kernel(const float* __restrict__ prob, const float* __restrict__ q,
                                                                  const float* __restrict__ part, const int* __restrict__ link,
                                                                  const int* __restrict__ restarted, int* __restrict__ link_next,
                                                                  float* __restrict__ state, float* __restrict__ stats,
                                                                  int* __restrict__ linked_out, int G, int voxels) {
    __shared__ float fin[SE_VF_PART];
    const int t = threadIdx.x, row = blockIdx.y;
    const bool linked = vf_has_prior(link, 0, row);
    if (linked) vf_fold_records<SE_TS_STATS>(part, row, G, t, fin);  // uniform; an unlinked row has no records
    const float s = linked ? fin[0] : 0.f;
    const bool back = linked && s > 0.f && s <= FLT_MAX;            // r_t = a / s; a NaN fails both comparisons
    if (blockIdx.x == 0 && t == 0) {
        float* o = stats + (size_t)row * SE_TS_STATS;
        const float nan = __int_as_float(0x7fc00000);
        o[0] = linked ? fin[1] : nan;                               // S
        o[1] = linked ? s : nan;
        o[2] = linked ? fin[2] : nan;                               // A0
        o[3] = linked ? fin[3] : nan;                               // A2
        o[4] = linked ? fin[4] : nan;                               // Bsum
        o[5] = linked ? fin[5] : nan;                               // Rsum
        linked_out[row] = linked ? 1 : 0;
        link_next[row] = restarted[row] == 0;                       // the frame before this one is linked to it unless it restarted
    }
    const size_t base = (size_t)row * voxels;
    const VfStream st[1] = {{(back ? q : prob) + base, back, s, state + base, nullptr}};
    vf_scale_or_copy<VEC>(st, voxels, t);
}

// the dynamic LDS of ts_blur_kj_kernel: whole planes where three fit, else the k-blurred planes by halves of the columns
inline int ts_kw(int G) { return 3 * G * G * 4 <= SE_TS_LDS_MAX ? G : (G + 1) / 2; }

// scratch of the transition statistics: P0 and P1 [rows][voxels], the records [rows][G][8], w' and m' (40 floats each), two arrays of
// link flags
inline long long ts_tail_elems(int rows, int G) { return (long long)rows * G * SE_VF_PART + 80 + 2LL * ((rows + 3) & ~3); }

}  // namespace

extern "C" long long se_volume_transition_stats_scratch_bytes(int rows, int G, int radius) {
    if (!vg_shape_ok(rows, G, radius)) return 0;
    return (2 * vg_elems(rows, G) + ts_tail_elems(rows, G)) * 4;
}

extern "C" int se_volume_transition_stats_f32(const float* prob, const float* belief, const int* restarted, const float* taps,
                                              float* state, float* stats, int* linked, void* scratch, long long scratch_bytes,
                                              int frames, int rows, int voxels, int G, int radius, float floor, const int* have_link,
                                              void* stream) {
    if (!prob || !belief || !restarted || !taps || !state || !stats || !linked || !scratch) return SE_ERR_BAD_ARG;
    if (!vg_args_ok(frames, rows, voxels, G, radius, floor)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, belief, restarted, taps, state, stats, linked, scratch, have_link}, 4)) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_volume_transition_stats_scratch_bytes(rows, G, radius)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    float* P0 = reinterpret_cast<float*>(scratch);
    float* P1 = P0 + vg_elems(rows, G);
    float* part = P1 + vg_elems(rows, G);
    float* rev = part + (long long)rows * G * SE_VF_PART;
    float* msq = rev + 40;
    int* link2 = reinterpret_cast<int*>(msq + 40);
    const int link_stride = (rows + 3) & ~3;
    const auto [wshift, chunks, keep, uniform] = vg_launch(voxels, G, floor);
    const int KW = ts_kw(G);
    const int kj_bytes = (G + 2 * KW) * G * 4;
    SE_ENSURE_LDS(ts_blur_kj_kernel, SE_TS_LDS_MAX);                // three planes at G = 116 are the most: 161,472 B
    SE_ENSURE_LDS(ts_update_kernel, 2 * SE_VG_MAX_G * SE_VG_MAX_G * 4);
    const bool vec = (voxels & 3) == 0 && se_aligned({prob, state, scratch}, 16);
    const auto finish = vec ? ts_finish_kernel<true> : ts_finish_kernel<false>;
    const size_t frame_elems = (size_t)rows * voxels;
    hipLaunchKernelGGL(ts_prep_kernel, dim3(1), dim3(64), 0, s, taps, rev, msq, radius);
    SE_CHECK_LAUNCH();
    for (int f = frames - 1; f >= 0; --f) {
        const float* p = prob + f * frame_elems;
        const float* b = belief + f * frame_elems;
        // the link flags of frame f: the caller's for the last frame, else what the finish pass of frame f + 1 wrote
        const int* link = f == frames - 1 ? have_link : link2 + (size_t)(f & 1) * link_stride;
        int* link_next = link2 + (size_t)((f + 1) & 1) * link_stride;                    // read by frame f - 1
        if (link) {
            hipLaunchKernelGGL(ts_blur_kj_kernel, dim3(G, rows), dim3(SE_VG_THREADS), kj_bytes, s, state, rev, msq, link, P0, P1, part,
                               G, voxels, radius, wshift, KW);
            SE_CHECK_LAUNCH();
            hipLaunchKernelGGL(ts_update_kernel, dim3(G, rows), dim3(SE_VG_THREADS), 2 * G * G * 4, s, p, b, rev, msq, link, P0, P1,
                               part, G, voxels, radius, wshift, keep, uniform);
            SE_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(finish, dim3(chunks, rows), dim3(SE_VG_THREADS), 0, s, p, P0, part, link, restarted + (size_t)f * rows,
                           link_next, state, stats + (size_t)f * rows * SE_TS_STATS, linked + (size_t)f * rows, G, voxels);
        SE_CHECK_LAUNCH();
    }
    return 0;
}
