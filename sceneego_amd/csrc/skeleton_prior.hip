// Skeleton-coupled joints: sum-product belief propagation over the kinematic tree of the joint volumes, with a spherical-shell
// bone-length factor on every edge (sceneego_amd/skeleton_prior.py: SkeletonPrior; VoxelNetwork_depth.skeleton_prior returns one).
// The reference forces bone lengths onto a finished pose (utils/skeleton.py: _skeleton_resize); this runs on the whole distributions.
// include/sceneego_hip.h states the definition; tests/skeleton_prior_model.py restates it in float64.
//
// THE CORRELATION (se_shell_correlate_f32; 2 (J - 1) of them per frame inside se_skeleton_couple_f32)
//     out(x) = scale_mul * (sum over d with w(d) != 0 and x + d inside the grid of w(d) a(x + d)) / s + add
// with w a dense (2R+1)^3 block that is mostly zero: a shell.
//   sk_runs_kernel      (skeleton_shell.h) grid (2R+1, tap rows), block 64: for one di-plane of one block, lane dk finds in the column w(di, ., dk) the first
//                       and the last maximal run of non-zero taps along dj and whether anything non-zero lies between them (for a
//                       shell: two runs, or one, and nothing between); entry 2R+1 of the plane says whether the plane has a tap at all.
//                       (2R+1) x (2R+2) records of 4 ints per block, built once per call.
//   sk_correlate_kernel grid (G x ceil(G/16) x ceil(G/64), rows), block 256: a workgroup owns the outputs (i, 16 rows j, 64 columns k)
//                       of one volume; lane = k, a wave owns SK_JR = 4 consecutive j.  For every di whose plane has a tap and lies inside
//                       the grid, the source plane i + di is staged in LDS with a zero halo of R rows and R columns ((16 + 2R) x (64 + 2R)
//                       floats: 20.8 KB at R = 18), so the loops below carry no bounds test.  Then for dk ascending and dj ascending over
//                       the column's runs the taps - wave-uniform, read through scalar loads - are taken four at a time: 4 LDS reads
//                       (consecutive lanes, consecutive addresses: no bank conflict) feed 16 fused multiply-adds, the window of 7 rows
//                       a lane holds slides down by 4 with 3 values carried in registers.  A run's last 1..3 taps and the taps between
//                       the two runs go one at a time (4 reads, 4 FMAs; between the runs each tap is tested and a zero is skipped).
//                       LDS reads per FMA: 1/4 in the groups of four, 1 in the tails.
// SUMMATION ORDER of one output: inside a plane one chain of fused multiply-adds, dk ascending, then dj ascending, started from 0; the
// planes' sums are added in ascending di.  The longest chain is therefore
//     T(R) = (2R+1)^2 + 2R            (SE_SK_SHELL_CHAIN(R); never more than the non-zero taps: every plane that is added holds one)
// roundings, 1405 at R = 18 against about 15,000 taps.  It depends on the taps alone.
//
// THE TREE (se_skeleton_couple_f32).  Joints are processed by depth level: a call is a chain of launches bounded by the tree, not the batch.
//   upward, depth d = deepest .. 1:   sk_product_kernel  A_j = p_j prod_c U_c for every j of the level, with the chunk sums of A_j
//                                     sk_fold_kernel     s_j
//                                     sk_correlate_kernel U_j = (1 - floor) corr(A_j, w_j) / s_j + floor / N
//   downward, depth d = 0 .. deepest: sk_product_kernel  T_j = p_j D_j prod_c U_c (with the chunk sums Z, sum T c, sum p c) for every j
//                                                        of the level and E_c = p_j D_j prod_{c' != c} U_c' (chunk sum t_c) for every
//                                                        child c of such a j, in one launch
//                                     sk_fold_kernel     Z_j, the joint sums, t_c
//                                     sk_correlate_kernel D_c = (1 - floor) corr(E_c, w_c) / t_c + floor / N
//   sk_finish_kernel    b_j = T_j / Z_j, joints, evidence, coupled - or, when one of the frame's s, t, Z is not a finite number > 0, the
//                       copy of p and sum p c.
// The reference tree (depths 0..5) takes 15 + 17 + 1 = 33 launches and the run table's one.  Products are taken left to right: p, then D, then
// the children's U in ascending order.  Scratch per frame: A / E, U (T_j overwrites U_j, which nobody reads once level depth(j) of the
// downward pass begins) and D: 3 J N floats, the chunk records and the folded sums; frames are walked in groups of SK_GROUP inside
// the call, so the scratch does not grow with the batch.
// SUMS.  No atomics.  A row of N values is cut into CH = min(64, ceil(N / 256)) chunks of ceil(N / CH) values, one workgroup each: thread
// t adds the values t, t + 256, ... of its chunk in sequence (<= 128 terms at 128^3), the workgroup folds them by row_reduce.h
// (butterfly 6, four waves 2), sk_fold_kernel gives lane l record l (CH <= 64: one each) and folds the lanes by a butterfly (6):
// L = 128 + 6 + 2 + 6 = 142 (SE_SK_SUM_CHAIN).  The chunk rule depends on N alone - not on the rows of a launch, as se_sa_splits does - so a
// frame's results are bitwise identical from run to run and do not depend on how frames are batched into calls or groups.
//
// THE EDGE STATISTICS (se_skeleton_edge_stats_f32; sceneego_amd/skeleton_fit.py: SkeletonModelFit) are the same walk (sk_walk) with E_c
// kept beside A_c - a fourth J N buffer per frame in flight - and one sk_moments_kernel launch behind every downward level; they are
// described with that kernel, below.  Both entry points launch the same product, fold and correlation kernels in the same order.
//
// THE UPWARD WALK (se_skeleton_upward_f32 in skeleton_sample.hip, through sk_upward_walk at the end of this file) is the third mode of
// sk_walk: the upward levels above, then one product-and-fold level more for the root, A_0 = p_0 prod U_c and s_0 - the product the
// coupling forms as T_0 in its downward pass, by the same kernel on the same operands, so s_0 equals its evidence[0] bit for bit -
// and sk_upward_finish_kernel.  A_j goes straight into the caller's buffer; the scratch holds U, the chunk records and the sums.
#include <float.h>
#include <stdint.h>

#include "row_reduce.h"
#include "skeleton_shell.h"      // the limits, SkTree / SkRows, the chunk rule, sk_runs_kernel and the launch geometry: shared with skeleton_pose.hip

#define SK_PART 8                // one chunk record: sum, sum v c (x y z), sum p c (x y z), pad
#define SK_MAX_ITEMS (2 * SK_MAX_J)

namespace {

// one product of sk_product_kernel: kind 0 = A_j (into A[j]; sum s_j), 1 = T_j (into U[j]; Z_j and the joint sums), 2 = E_c for child
// c = excl of j (into Eout[c]; sum t_c).  se_skeleton_couple_f32 passes A as Eout (nobody reads A_c any more); se_skeleton_edge_stats_f32
// keeps both and passes no coord: the joint sums stay 0 there.
struct SkItems {
    int n;
    unsigned char j[SK_MAX_ITEMS];
    signed char excl[SK_MAX_ITEMS];
    unsigned char kind[SK_MAX_ITEMS];
};

// the taps lo..hi (dj + R) of one column, all non-zero: four at a time, then one at a time.  wp: the column's taps at dj + R = 0, stride W;
// lp: the lane's LDS value under output row 0 and dj + R = 0, stride LW.
__device__ __forceinline__ void sk_run(const float* __restrict__ wp, int W, const float* lp, int LW, int lo, int hi, float (&acc)[SK_JR]) {
    int d = lo;
    if (d + 3 <= hi) {
        float v0 = lp[(d + 0) * LW], v1 = lp[(d + 1) * LW], v2 = lp[(d + 2) * LW];
        for (; d + 3 <= hi; d += 4) {
            const float w0 = wp[(d + 0) * W], w1 = wp[(d + 1) * W], w2 = wp[(d + 2) * W], w3 = wp[(d + 3) * W];
            const float v3 = lp[(d + 3) * LW], v4 = lp[(d + 4) * LW], v5 = lp[(d + 5) * LW], v6 = lp[(d + 6) * LW];
            acc[0] = fmaf(w0, v0, acc[0]); acc[1] = fmaf(w0, v1, acc[1]); acc[2] = fmaf(w0, v2, acc[2]); acc[3] = fmaf(w0, v3, acc[3]);
            acc[0] = fmaf(w1, v1, acc[0]); acc[1] = fmaf(w1, v2, acc[1]); acc[2] = fmaf(w1, v3, acc[2]); acc[3] = fmaf(w1, v4, acc[3]);
            acc[0] = fmaf(w2, v2, acc[0]); acc[1] = fmaf(w2, v3, acc[1]); acc[2] = fmaf(w2, v4, acc[2]); acc[3] = fmaf(w2, v5, acc[3]);
            acc[0] = fmaf(w3, v3, acc[0]); acc[1] = fmaf(w3, v4, acc[1]); acc[2] = fmaf(w3, v5, acc[2]); acc[3] = fmaf(w3, v6, acc[3]);
            v0 = v4; v1 = v5; v2 = v6;
        }
    }
    for (; d <= hi; ++d) {
        const float w = wp[d * W];
#pragma unroll
        for (int x = 0; x < SK_JR; ++x) acc[x] = fmaf(w, lp[(d + x) * LW], acc[x]);
    }
}
static_assert(SK_JR == 4, "sk_run is written out for four rows per lane");

// grid (G * ceil(G / SK_TJ) * ceil(G / SK_KC), rows), block 256, dynamic LDS (SK_TJ + 2R)(SK_KC + 2R) floats.
// tap_row != NULL (se_shell_correlate_f32): row r reads a + r N, taps[tap_row[r]], s[r] and writes out + r N; a tap_row outside
// 0..tap_rows-1 fills the row with NaN.  tap_row == NULL (inside the tree): row r is joint map.slot[r % map.n] of frame r / map.n in
// [frame][J][N] buffers, its taps are the joint's and its s is s[(frame J + joint) s_stride].
__global__ __launch_bounds__(SK_THREADS) void sk_correlate_kernel(const float* __restrict__ a, const float* __restrict__ taps,
                                                                  const int* __restrict__ tap_row, const float* __restrict__ s,
                                                                  int s_stride, float* __restrict__ out, const int* __restrict__ runs,
                                                                  SkRows map, int J, int tap_rows, int G, int R, float scale_mul,
                                                                  float add) {
    extern __shared__ __align__(16) float lds[];
    const int t = threadIdx.x, kl = t & 63, wv = t >> 6;
    const int W = 2 * R + 1, LW = SK_KC + 2 * R, LH = SK_TJ + 2 * R;
    const int jt_n = (G + SK_TJ - 1) / SK_TJ, kc_n = (G + SK_KC - 1) / SK_KC;
    int bx = blockIdx.x;
    const int kc = bx % kc_n; bx /= kc_n;
    const int jt = bx % jt_n;
    const int i = bx / jt_n;
    const size_t N = (size_t)G * G * G;
    size_t row;
    int tr;
    float sval;
    if (tap_row) {
        row = blockIdx.y;
        tr = tap_row[row];
        sval = s[row];
    } else {
        const int f = blockIdx.y / map.n;
        tr = map.slot[blockIdx.y % map.n];
        row = (size_t)f * J + tr;
        sval = s[row * s_stride];
    }
    const float* in = a + row * N;
    float* o = out + row * N;
    const int k = kc * SK_KC + kl, j0 = jt * SK_TJ + wv * SK_JR;
    if (tr < 0 || tr >= tap_rows) {                                      // uniform
        if (k < G)
            for (int x = 0; x < SK_JR; ++x)
                if (j0 + x < G) o[((size_t)i * G + j0 + x) * G + k] = __int_as_float(0x7fc00000);
        return;
    }
    const float* wt = taps + (size_t)tr * W * W * W;
    const int* rn = runs + (size_t)tr * W * (W + 1) * 4;
    float total[SK_JR] = {0.f, 0.f, 0.f, 0.f};
    const int dlo = max(-R, -i), dhi = min(R, G - 1 - i);
    for (int di = dlo; di <= dhi; ++di) {
        const int* rp = rn + (size_t)(di + R) * (W + 1) * 4;
        if (!rp[W * 4]) continue;                                        // uniform: the plane has no tap
        __syncthreads();                                                 // everyone is done with the plane before
        const float* src = in + (size_t)(i + di) * G * G;
        for (int r = wv; r < LH; r += 4) {
            const int jj = jt * SK_TJ + r - R;
            for (int c = kl; c < LW; c += 64) {
                const int kk = kc * SK_KC + c - R;
                float v = 0.f;
                if (jj >= 0 && jj < G && kk >= 0 && kk < G) v = src[jj * G + kk];
                lds[r * LW + c] = v;
            }
        }
        __syncthreads();
        float acc[SK_JR] = {0.f, 0.f, 0.f, 0.f};
        for (int dk = 0; dk < W; ++dk) {                                 // dk + R
            const int lo1 = rp[dk * 4 + 0], hi1 = rp[dk * 4 + 1], lo2 = rp[dk * 4 + 2], h2 = rp[dk * 4 + 3];
            if (lo1 > hi1) continue;
            const float* wp = wt + (size_t)(di + R) * W * W + dk;
            const float* lp = lds + (wv * SK_JR) * LW + kl + dk;         // row (wv JR + x) + (dj + R), column kl + (dk + R)
            sk_run(wp, W, lp, LW, lo1, hi1, acc);
            const int hi2 = h2 & 0xff;
            if (lo2 <= hi2) {
                if (h2 >> 8) {
                    for (int d = hi1 + 1; d < lo2; ++d) {
                        const float w = wp[d * W];
                        if (w != 0.f) {
#pragma unroll
                            for (int x = 0; x < SK_JR; ++x) acc[x] = fmaf(w, lp[(d + x) * LW], acc[x]);
                        }
                    }
                }
                sk_run(wp, W, lp, LW, lo2, hi2, acc);
            }
        }
#pragma unroll
        for (int x = 0; x < SK_JR; ++x) total[x] += acc[x];
    }
    if (k < G) {
#pragma unroll
        for (int x = 0; x < SK_JR; ++x)
            if (j0 + x < G) o[((size_t)i * G + j0 + x) * G + k] = fmaf(scale_mul, total[x] / sval, add);
    }
}

// grid (CH, items * frames), block 256.  All buffers [frames][J][N]; part [frames][items][CH][SK_PART].
__global__ __launch_bounds__(SK_THREADS) void sk_product_kernel(const float* __restrict__ prob, const float* __restrict__ coord,
                                                                const float* __restrict__ U, const float* __restrict__ D,
                                                                float* __restrict__ A, float* __restrict__ Tout, float* Eout,
                                                                float* __restrict__ part, SkTree tree, SkItems items, int voxels) {
    __shared__ float sm[4][SK_PART];
    const int t = threadIdx.x, it = blockIdx.y % items.n, f = blockIdx.y / items.n;
    const int J = tree.J, j = items.j[it], excl = items.excl[it], kind = items.kind[it];
    const size_t fb = (size_t)f * J * voxels;
    const float* p = prob + fb + (size_t)j * voxels;
    const float* d = (kind != 0 && j > 0) ? D + fb + (size_t)j * voxels : nullptr;
    float* o = kind == 1 ? Tout + fb + (size_t)j * voxels : kind == 2 ? Eout + fb + (size_t)excl * voxels : A + fb + (size_t)j * voxels;
    const int chunk = sk_chunk(voxels), c0 = blockIdx.x * chunk, c1 = min(c0 + chunk, voxels);
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n = c0 + t; n < c1; n += SK_THREADS) {
        const float pv = p[n];
        float v = pv;
        if (d) v *= d[n];
        for (int c = j + 1; c < J; ++c)                                  // the children in ascending order (uniform)
            if (tree.parent[c] == j && c != excl) v *= U[fb + (size_t)c * voxels + n];
        o[n] = v;
        acc[0] += v;
        if (kind == 1 && coord) {
            const float cx = coord[(size_t)n * 3 + 0], cy = coord[(size_t)n * 3 + 1], cz = coord[(size_t)n * 3 + 2];
            acc[1] += v * cx; acc[2] += v * cy; acc[3] += v * cz;
            acc[4] += pv * cx; acc[5] += pv * cy; acc[6] += pv * cz;
        }
    }
    block_fold_stage<7, SK_PART>(acc, sm);
    if (t < 7) part[(((size_t)f * items.n + it) * gridDim.x + blockIdx.x) * SK_PART + t] = block_fold_sum<SK_PART>(sm, t);
}

// grid (items, frames), block 64.  sums [frames][J][3][SK_PART]: plane 0 = s_j, 1 = t_c, 2 = Z_j and the joint sums
__global__ __launch_bounds__(64) void sk_fold_kernel(const float* __restrict__ part, float* __restrict__ sums, SkItems items, int J, int CH) {
    const int it = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    wave_fold_records<7, SK_PART>(part, ((size_t)f * items.n + it) * CH, CH, t, acc);
    const int kind = items.kind[it], slot = kind == 2 ? items.excl[it] : items.j[it];
    const int plane = kind == 0 ? 0 : kind == 2 ? 1 : 2;
    float* o = sums + (((size_t)f * J + slot) * 3 + plane) * SK_PART;
    if (t == 0) {
#pragma unroll
        for (int x = 0; x < 7; ++x) o[x] = acc[x];
    }
}

// grid (chunks, J, frames), block 256.  T [frames][J][N] (the U buffer); outputs at the call's frame f0 + frame.
__global__ __launch_bounds__(SK_THREADS) void sk_finish_kernel(const float* __restrict__ prob, const float* __restrict__ T,
                                                               const float* __restrict__ sums, float* __restrict__ beliefs,
                                                               float* __restrict__ joints, float* __restrict__ evidence,
                                                               int* __restrict__ coupled, int J, int voxels) {
    const int t = threadIdx.x, j = blockIdx.y, f = blockIdx.z;
    const float* sf = sums + (size_t)f * 3 * J * SK_PART;
    int bad = 0;
    for (int e = t; e < 3 * J; e += SK_THREADS) {
        const int plane = e / J, jj = e % J;
        if (plane < 2 && jj == 0) continue;                              // the root sends no message and receives none
        const float v = sf[((size_t)jj * 3 + plane) * SK_PART];
        bad |= !(v > 0.f && v <= FLT_MAX);                               // a NaN fails both comparisons
    }
    const bool fallback = __syncthreads_or(bad) != 0;
    const float* fin = sf + ((size_t)j * 3 + 2) * SK_PART;
    const float Z = fin[0];
    const size_t row = (size_t)f * J + j;
    if (blockIdx.x == 0 && t == 0) {
        float* o = joints + row * 3;
        if (fallback) { o[0] = fin[4]; o[1] = fin[5]; o[2] = fin[6]; }
        else { o[0] = fin[1] / Z; o[1] = fin[2] / Z; o[2] = fin[3] / Z; }
        evidence[row] = Z;
        if (j == 0) coupled[f] = fallback ? 0 : 1;
    }
    if (!beliefs) return;
    const float* src = (fallback ? prob : T) + row * voxels;             // the copy of p is bit for bit
    float* dst = beliefs + row * voxels;
    for (int n = blockIdx.x * SK_THREADS + t; n < voxels; n += gridDim.x * SK_THREADS) {
        float x = src[n];
        if (!fallback) x = x / Z;
        dst[n] = x;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the edge moments
// THE MOMENTS (se_shell_moments_f32; one launch per downward level inside se_skeleton_edge_stats_f32)
//     S_m = sum_x e(x) corr(a, w_m)(x),  m = 0, 1, 2,  w_0 = w,  w_1 = w r,  w_2 = w r^2, a tap with w(d) == 0 skipped in all three
// sk_moments_kernel is sk_correlate_kernel with three accumulators per output and no volume written: the same tiling, the same LDS
// plane with its zero halo, the same run table (built from w alone) and the same sliding window of seven values, so 4 LDS reads feed
// 48 fused multiply-adds in the groups of four.  The three blocks are interleaved first (sk_pack_taps_kernel: one (w, w1, w2, 0)
// record of 16 bytes per tap, dj innermost), so a tap is ONE 16-byte scalar load, not three of four bytes - the scalar loads share
// the lgkmcnt counter with the LDS reads - and the taps of a run are consecutive in memory.
// SUMMATION ORDER.  Each of the three correlation values is the correlation's chain, SE_SK_SHELL_CHAIN(R).  Behind it: a lane folds
// its four outputs into r_m = fma(e_3, c_3, fma(e_2, c_2, fma(e_1, c_1, fma(e_0, c_0, 0)))) (outputs outside the grid are passed
// over; e(x) is read from global memory once per output), the workgroup folds its lanes (butterfly 6, four waves 2) into one record,
// and sk_moments_fold / sk_edge_finish_kernel fold the row's G ceil(G / 16) ceil(G / 64) records: lane l takes records l, l + 64, ...
// in sequence, then a butterfly (6).  Longest chain: 4 + 6 + 2 + ceil(records / 64) + 6 = SE_SK_MOMENT_CHAIN(G), 22 at 64^3 and 50
// at 128^3.  The order is fixed by (G, R) and the taps alone.
#define SK_MPART 4               // one record of the moments: S0, S1, S2, pad

// grid (ceil(W^3 / 256), tap_rows), block 256.  The records are stored with dj innermost, index ((di+R) W + dk+R) W + dj+R: the taps of
// one column's run are consecutive, so their addresses are one base and constant offsets
__global__ __launch_bounds__(SK_THREADS) void sk_pack_taps_kernel(const float* __restrict__ w0, const float* __restrict__ w1,
                                                                  const float* __restrict__ w2, float4* __restrict__ packed, int block, int W) {
    const int n = blockIdx.x * SK_THREADS + threadIdx.x;
    if (n >= block) return;
    const int dk = n % W, dj = n / W % W, di = n / (W * W);
    const size_t base = (size_t)blockIdx.y * block, at = base + n;
    packed[base + ((size_t)di * W + dk) * W + dj] = make_float4(w0[at], w1[at], w2[at], 0.f);
}

__device__ __forceinline__ void sk_fma3(const float4 w, const float v, float (&acc)[3][SK_JR], int x) {
    acc[0][x] = fmaf(w.x, v, acc[0][x]);
    acc[1][x] = fmaf(w.y, v, acc[1][x]);
    acc[2][x] = fmaf(w.z, v, acc[2][x]);
}

// sk_run with the three sums: wp the column's packed taps at dj + R = 0, consecutive
__device__ __forceinline__ void sk_run3(const float4* __restrict__ wp, const float* lp, int LW, int lo, int hi,
                                        float (&acc)[3][SK_JR]) {
    int d = lo;
    if (d + 3 <= hi) {
        float v0 = lp[(d + 0) * LW], v1 = lp[(d + 1) * LW], v2 = lp[(d + 2) * LW];
        for (; d + 3 <= hi; d += 4) {
            const float4 w0 = wp[d + 0], w1 = wp[d + 1], w2 = wp[d + 2], w3 = wp[d + 3];
            const float v3 = lp[(d + 3) * LW], v4 = lp[(d + 4) * LW], v5 = lp[(d + 5) * LW], v6 = lp[(d + 6) * LW];
            sk_fma3(w0, v0, acc, 0); sk_fma3(w0, v1, acc, 1); sk_fma3(w0, v2, acc, 2); sk_fma3(w0, v3, acc, 3);
            sk_fma3(w1, v1, acc, 0); sk_fma3(w1, v2, acc, 1); sk_fma3(w1, v3, acc, 2); sk_fma3(w1, v4, acc, 3);
            sk_fma3(w2, v2, acc, 0); sk_fma3(w2, v3, acc, 1); sk_fma3(w2, v4, acc, 2); sk_fma3(w2, v5, acc, 3);
            sk_fma3(w3, v3, acc, 0); sk_fma3(w3, v4, acc, 1); sk_fma3(w3, v5, acc, 2); sk_fma3(w3, v6, acc, 3);
            v0 = v4; v1 = v5; v2 = v6;
        }
    }
    for (; d <= hi; ++d) {
        const float4 w = wp[d];
#pragma unroll
        for (int x = 0; x < SK_JR; ++x) sk_fma3(w, lp[(d + x) * LW], acc, x);
    }
}

// grid (G * ceil(G / SK_TJ) * ceil(G / SK_KC), rows), block 256, dynamic LDS as sk_correlate_kernel.  Rows as there: tap_row != NULL
// (se_shell_moments_f32): row r reads e + r N, a + r N and the packed taps of block tap_row[r] (outside 0..tap_rows-1: NaN records);
// tap_row == NULL (inside the tree): row r is joint map.slot[r % map.n] of frame r / map.n in [frame][J][N] buffers.  Writes record
// blockIdx.x of the row into part [rows][gridDim.x][SK_MPART] (inside the tree: row = frame J + joint).
__global__ __launch_bounds__(SK_THREADS) void sk_moments_kernel(const float* __restrict__ e, const float* __restrict__ a,
                                                                const float4* __restrict__ packed, const int* __restrict__ tap_row,
                                                                float* __restrict__ part, const int* __restrict__ runs, SkRows map,
                                                                int J, int tap_rows, int G, int R) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float sm[4][SK_MPART];
    const int t = threadIdx.x, kl = t & 63, wv = t >> 6;
    const int W = 2 * R + 1, LW = SK_KC + 2 * R, LH = SK_TJ + 2 * R;
    const int jt_n = (G + SK_TJ - 1) / SK_TJ, kc_n = (G + SK_KC - 1) / SK_KC;
    int bx = blockIdx.x;
    const int kc = bx % kc_n; bx /= kc_n;
    const int jt = bx % jt_n;
    const int i = bx / jt_n;
    const size_t N = (size_t)G * G * G;
    size_t row;
    int tr;
    if (tap_row) {
        row = blockIdx.y;
        tr = tap_row[row];
    } else {
        tr = map.slot[blockIdx.y % map.n];
        row = (size_t)(blockIdx.y / map.n) * J + tr;
    }
    float* rec = part + (row * gridDim.x + blockIdx.x) * SK_MPART;
    if (tr < 0 || tr >= tap_rows) {                                      // uniform
        if (t < 3) rec[t] = __int_as_float(0x7fc00000);
        return;
    }
    const float* in = a + row * N;
    const float4* wt = packed + (size_t)tr * W * W * W;
    const int* rn = runs + (size_t)tr * W * (W + 1) * 4;
    float total[3][SK_JR] = {};
    const int dlo = max(-R, -i), dhi = min(R, G - 1 - i);
    for (int di = dlo; di <= dhi; ++di) {
        const int* rp = rn + (size_t)(di + R) * (W + 1) * 4;
        if (!rp[W * 4]) continue;                                        // uniform: the plane has no tap
        __syncthreads();                                                 // everyone is done with the plane before
        const float* src = in + (size_t)(i + di) * G * G;
        for (int r = wv; r < LH; r += 4) {
            const int jj = jt * SK_TJ + r - R;
            for (int c = kl; c < LW; c += 64) {
                const int kk = kc * SK_KC + c - R;
                float v = 0.f;
                if (jj >= 0 && jj < G && kk >= 0 && kk < G) v = src[jj * G + kk];
                lds[r * LW + c] = v;
            }
        }
        __syncthreads();
        float acc[3][SK_JR] = {};
        for (int dk = 0; dk < W; ++dk) {                                 // dk + R
            const int lo1 = rp[dk * 4 + 0], hi1 = rp[dk * 4 + 1], lo2 = rp[dk * 4 + 2], h2 = rp[dk * 4 + 3];
            if (lo1 > hi1) continue;
            const float4* wp = wt + ((size_t)(di + R) * W + dk) * W;
            const float* lp = lds + (wv * SK_JR) * LW + kl + dk;
            sk_run3(wp, lp, LW, lo1, hi1, acc);
            const int hi2 = h2 & 0xff;
            if (lo2 <= hi2) {
                if (h2 >> 8) {
                    for (int d = hi1 + 1; d < lo2; ++d) {
                        const float4 w = wp[d];
                        if (w.x != 0.f) {
#pragma unroll
                            for (int x = 0; x < SK_JR; ++x) sk_fma3(w, lp[(d + x) * LW], acc, x);
                        }
                    }
                }
                sk_run3(wp, lp, LW, lo2, hi2, acc);
            }
        }
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int x = 0; x < SK_JR; ++x) total[m][x] += acc[m][x];
    }
    const int k = kc * SK_KC + kl, j0 = jt * SK_TJ + wv * SK_JR;
    const float* ev = e + row * N;
    float red[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int x = 0; x < SK_JR; ++x)
        if (k < G && j0 + x < G) {
            const float w = ev[((size_t)i * G + j0 + x) * G + k];
#pragma unroll
            for (int m = 0; m < 3; ++m) red[m] = fmaf(w, total[m][x], red[m]);
        }
    block_fold_stage<3, SK_MPART>(red, sm);
    if (t < 3) rec[t] = block_fold_sum<SK_MPART>(sm, t);
}

// grid (rows), block 64: out [rows][3]
__global__ __launch_bounds__(64) void sk_moments_fold_kernel(const float* __restrict__ part, float* __restrict__ out, int records) {
    float acc[3] = {0.f, 0.f, 0.f};
    wave_fold_records<3, SK_MPART>(part, (size_t)blockIdx.x * records, records, threadIdx.x, acc);
    if (threadIdx.x < 3) out[(size_t)blockIdx.x * 3 + threadIdx.x] = acc[threadIdx.x];
}

// grid (J, frames), block 64: the records of edge j folded, SJ, the normalisers and the frame's flag by sk_finish_kernel's rule.
// stats [frames][J][4], norms [frames][J][3], valid [frames] at the call's frame f0 + frame.
__global__ __launch_bounds__(64) void sk_edge_finish_kernel(const float* __restrict__ part, const float* __restrict__ sums,
                                                            float* __restrict__ stats, float* __restrict__ norms,
                                                            int* __restrict__ valid, int J, int records, float uniform) {
    const int t = threadIdx.x, j = blockIdx.x, f = blockIdx.y;
    const float* sf = sums + (size_t)f * 3 * J * SK_PART;
    const size_t row = (size_t)f * J + j;
    const float nan = __int_as_float(0x7fc00000);
    if (j == 0) {
        int bad = 0;
        for (int e = t; e < 3 * J; e += 64) {
            const int plane = e / J, jj = e % J;
            if (plane < 2 && jj == 0) continue;                          // the root sends no message and receives none
            const float v = sf[((size_t)jj * 3 + plane) * SK_PART];
            bad |= !(v > 0.f && v <= FLT_MAX);
        }
        const bool fallback = __syncthreads_or(bad) != 0;
        if (t == 0) {
            valid[f] = fallback ? 0 : 1;
            float* o = stats + row * 4;
            o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f;
            float* n = norms + row * 3;
            n[0] = nan; n[1] = nan; n[2] = sf[2 * SK_PART];
        }
        return;
    }
    float acc[3] = {0.f, 0.f, 0.f};
    wave_fold_records<3, SK_MPART>(part, row * records, records, t, acc);
    if (t == 0) {
        const float s = sf[((size_t)j * 3 + 0) * SK_PART], tt = sf[((size_t)j * 3 + 1) * SK_PART], Z = sf[((size_t)j * 3 + 2) * SK_PART];
        float* o = stats + row * 4;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = (uniform * tt) * s;
        float* n = norms + row * 3;
        n[0] = s; n[1] = tt; n[2] = Z;
    }
}

// grid (frames), block 64: the upward walk's outputs (se_skeleton_upward_f32).  out_sums [frames][J] = s_j, now also s_0 (the sum of
// the root's product); valid [frames] = 1 iff every one of them is a finite number > 0, at the call's frame f0 + frame.
__global__ __launch_bounds__(64) void sk_upward_finish_kernel(const float* __restrict__ sums, float* __restrict__ out_sums,
                                                              int* __restrict__ valid, int J) {
    const int t = threadIdx.x, f = blockIdx.x;
    int bad = 0;
    if (t < J) {
        const float v = sums[(((size_t)f * J + t) * 3 + 0) * SK_PART];
        out_sums[(size_t)f * J + t] = v;
        bad = !(v > 0.f && v <= FLT_MAX);                                // a NaN fails both comparisons
    }
    const int any = __syncthreads_or(bad);
    if (t == 0) valid[f] = any ? 0 : 1;
}
static_assert(SK_MAX_J <= 64, "sk_upward_finish_kernel gives every joint a lane");

inline int sk_moment_records(int G) { return G * ((G + SK_TJ - 1) / SK_TJ) * ((G + SK_KC - 1) / SK_KC); }
inline long long sk_packed_bytes(int tap_rows, int R) {                  // 16 more: the records are aligned inside the scratch
    const long long W = 2 * R + 1;
    return (long long)tap_rows * W * W * W * 16 + 16;
}
inline float4* sk_align16(void* p) { return reinterpret_cast<float4*>((reinterpret_cast<uintptr_t>(p) + 15) & ~(uintptr_t)15); }

inline long long sk_frame_floats(int J, int G) {
    const long long N = (long long)G * G * G;
    return 3 * J * N + (long long)SK_MAX_ITEMS * sk_chunks((int)N) * SK_PART + 3LL * J * SK_PART;
}

}  // namespace

extern "C" long long se_shell_correlate_scratch_bytes(int tap_rows, int R) {
    if (tap_rows < 1 || tap_rows > 65535 || R < 0 || R > SK_MAX_R) return 0;
    return sk_runs_ints(tap_rows, R) * 4;
}

extern "C" int se_shell_correlate_f32(const float* a, const float* taps, const int* tap_row, const float* s, float* out, void* scratch,
                                      long long scratch_bytes, int rows, int tap_rows, int G, int R, float scale_mul, float add,
                                      void* stream) {
    if (!a || !taps || !tap_row || !s || !out || !scratch) return SE_ERR_BAD_ARG;
    if (rows < 1 || rows > 65535 || tap_rows < 1 || tap_rows > 65535 || !sk_shape_ok(G, R)) return SE_ERR_BAD_ARG;
    if (!se_aligned({a, taps, tap_row, s, out, scratch}, 4) || a == out) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_shell_correlate_scratch_bytes(tap_rows, R)) return SE_ERR_BAD_ARG;
    hipStream_t st = se_stream(stream);
    int* runs = reinterpret_cast<int*>(scratch);
    hipLaunchKernelGGL(sk_runs_kernel, dim3(2 * R + 1, tap_rows), dim3(64), 0, st, taps, runs, R);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sk_correlate_kernel, sk_corr_grid(G, rows), dim3(SK_THREADS), sk_lds_bytes(R), st, a, taps, tap_row, s, 1, out, runs,
                       SkRows{}, 0, tap_rows, G, R, scale_mul, add);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" long long se_shell_moments_scratch_bytes(int rows, int tap_rows, int G, int R) {
    if (rows < 1 || rows > 65535 || tap_rows < 1 || tap_rows > 65535 || !sk_shape_ok(G, R)) return 0;
    return sk_runs_ints(tap_rows, R) * 4 + (long long)rows * sk_moment_records(G) * SK_MPART * 4 + sk_packed_bytes(tap_rows, R);
}

extern "C" int se_shell_moments_f32(const float* e, const float* a, const float* taps, const float* taps_r, const float* taps_r2,
                                    const int* tap_row, float* out, void* scratch, long long scratch_bytes, int rows, int tap_rows, int G,
                                    int R, void* stream) {
    if (!e || !a || !taps || !taps_r || !taps_r2 || !tap_row || !out || !scratch) return SE_ERR_BAD_ARG;
    if (rows < 1 || rows > 65535 || tap_rows < 1 || tap_rows > 65535 || !sk_shape_ok(G, R)) return SE_ERR_BAD_ARG;
    if (!se_aligned({e, a, taps, taps_r, taps_r2, tap_row, out, scratch}, 4)) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_shell_moments_scratch_bytes(rows, tap_rows, G, R)) return SE_ERR_BAD_ARG;
    hipStream_t st = se_stream(stream);
    const int records = sk_moment_records(G), block = (2 * R + 1) * (2 * R + 1) * (2 * R + 1);
    int* runs = reinterpret_cast<int*>(scratch);
    float* part = reinterpret_cast<float*>(runs + sk_runs_ints(tap_rows, R));
    float4* packed = sk_align16(part + (size_t)rows * records * SK_MPART);
    hipLaunchKernelGGL(sk_runs_kernel, dim3(2 * R + 1, tap_rows), dim3(64), 0, st, taps, runs, R);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sk_pack_taps_kernel, dim3((block + SK_THREADS - 1) / SK_THREADS, tap_rows), dim3(SK_THREADS), 0, st, taps, taps_r,
                       taps_r2, packed, block, 2 * R + 1);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sk_moments_kernel, sk_corr_grid(G, rows), dim3(SK_THREADS), sk_lds_bytes(R), st, e, a, packed, tap_row, part, runs,
                       SkRows{}, 0, tap_rows, G, R);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sk_moments_fold_kernel, dim3(rows), dim3(64), 0, st, part, out, records);
    SE_CHECK_LAUNCH();
    return 0;
}

namespace {

// What the three walks over the tree write.  se_skeleton_couple_f32: beliefs (or NULL), joints, evidence, coupled, with coord.
// se_skeleton_edge_stats_f32: stats, norms, valid, with the two further tap blocks; it keeps A_c beside E_c (a fourth J N buffer per
// frame in flight), packs the three blocks and adds one moments launch per downward level.  se_skeleton_upward_f32 (sk_upward_walk;
// the entry point is in skeleton_sample.hip): upward, up_sums, valid; the upward levels alone and one more for the root's product
// A_0, written straight into `upward`, so that only U, the chunk records and the sums live in the scratch.
struct SkOutputs {
    const float* coord;
    float *beliefs, *joints, *evidence;
    int* coupled;
    const float *taps_r, *taps_r2;
    float *stats, *norms;
    int* valid;
    float *upward, *up_sums;
};

// the floats per frame in flight of the upward walk: U, the chunk records, the folded sums
inline long long sk_upward_frame_floats(int J, int G) {
    const long long N = (long long)G * G * G;
    return J * N + (long long)SK_MAX_ITEMS * sk_chunks((int)N) * SK_PART + 3LL * J * SK_PART;
}

inline long long sk_walk_scratch_bytes(int frames, int J, int G, int R, bool moments) {
    long long bytes = ((long long)min(frames, SK_GROUP) * sk_frame_floats(J, G) + sk_runs_ints(J, R)) * 4;
    if (moments)
        bytes += (long long)min(frames, SK_GROUP) * J * ((long long)G * G * G + (long long)sk_moment_records(G) * SK_MPART) * 4 +
                 sk_packed_bytes(J, R);
    return bytes;
}

// The arguments the entry points share are checked by the caller; `out` says which of the three walks this is (out.stats != NULL: the
// edge statistics; out.upward != NULL: the upward walk).
int sk_walk(const float* prob, const float* taps, const int* parent, const SkOutputs& out, void* scratch, int frames, int J, int voxels,
            int G, int R, float floor, const SkTree& tree, const int* depth, int deepest, hipStream_t st) {
    const bool moments = out.stats != nullptr, upward = out.upward != nullptr;
    const size_t N = (size_t)voxels;
    const int group = min(frames, SK_GROUP), CH = sk_chunks(voxels), records = sk_moment_records(G);
    float* A = reinterpret_cast<float*>(scratch);                        // the upward walk: A is the caller's `upward`, no D
    float* U = upward ? A : A + (size_t)group * J * N;
    float* D = upward ? U : U + (size_t)group * J * N;
    float* part = D + (size_t)group * J * N;
    float* sums = part + (size_t)group * SK_MAX_ITEMS * CH * SK_PART;
    int* runs = reinterpret_cast<int*>(sums + (size_t)group * 3 * J * SK_PART);
    float* E = A;                                                        // E_c overwrites A_c unless the moments need both
    float* mpart = nullptr;
    float4* packed = nullptr;
    if (moments) {
        E = reinterpret_cast<float*>(runs + sk_runs_ints(J, R));
        mpart = E + (size_t)group * J * N;
        packed = sk_align16(mpart + (size_t)group * J * records * SK_MPART);
    }
    const float keep = 1.0f - floor, uniform = floor / (float)voxels;
    const int lds = sk_lds_bytes(R);
    const int fin_chunks = min(64, (voxels + SK_THREADS * 4 - 1) / (SK_THREADS * 4));

    if (J > 1) {
        hipLaunchKernelGGL(sk_runs_kernel, dim3(2 * R + 1, J), dim3(64), 0, st, taps, runs, R);
        SE_CHECK_LAUNCH();
        if (moments) {
            const int block = (2 * R + 1) * (2 * R + 1) * (2 * R + 1);
            hipLaunchKernelGGL(sk_pack_taps_kernel, dim3((block + SK_THREADS - 1) / SK_THREADS, J), dim3(SK_THREADS), 0, st, taps,
                               out.taps_r, out.taps_r2, packed, block, 2 * R + 1);
            SE_CHECK_LAUNCH();
        }
    }
    for (int f0 = 0; f0 < frames; f0 += group) {
        const int nf = min(group, frames - f0);
        const float* p = prob + (size_t)f0 * J * N;
        if (upward) E = A = out.upward + (size_t)f0 * J * N;
        // one level: the products, their sums, then the messages of `rows` from `src`
        auto level = [&](const SkItems& items, const SkRows& rows, int plane, const float* src, float* msg) -> int {
            if (items.n) {
                hipLaunchKernelGGL(sk_product_kernel, dim3(CH, items.n * nf), dim3(SK_THREADS), 0, st, p, out.coord, U, D, A, U, E, part,
                                   tree, items, voxels);
                SE_CHECK_LAUNCH();
                hipLaunchKernelGGL(sk_fold_kernel, dim3(items.n, nf), dim3(64), 0, st, part, sums, items, J, CH);
                SE_CHECK_LAUNCH();
            }
            if (rows.n) {
                hipLaunchKernelGGL(sk_correlate_kernel, sk_corr_grid(G, rows.n * nf), dim3(SK_THREADS), lds, st, src, taps, nullptr,
                                   sums + (size_t)plane * SK_PART, 3 * SK_PART, msg, runs, rows, J, J, G, R, keep, uniform);
                SE_CHECK_LAUNCH();
            }
            return 0;
        };
        for (int d = deepest; d >= 1; --d) {
            SkItems items{};
            SkRows rows{};
            for (int j = 1; j < J; ++j)
                if (depth[j] == d) {
                    items.j[items.n] = (unsigned char)j; items.excl[items.n] = -1; items.kind[items.n] = 0; ++items.n;
                    rows.slot[rows.n++] = (unsigned char)j;
                }
            const int rc = level(items, rows, 0, A, U);
            if (rc) return rc;
        }
        if (upward) {                                                    // one level more: A_0 = p_0 prod U_c and its sum; no message
            SkItems items{};
            items.j[0] = 0; items.excl[0] = -1; items.kind[0] = 0; items.n = 1;
            const int rc = level(items, SkRows{}, 0, A, U);
            if (rc) return rc;
            hipLaunchKernelGGL(sk_upward_finish_kernel, dim3(nf), dim3(64), 0, st, sums, out.up_sums + (size_t)f0 * J, out.valid + f0, J);
            SE_CHECK_LAUNCH();
            continue;
        }
        for (int d = 0; d <= deepest; ++d) {
            SkItems items{};
            SkRows rows{};
            for (int j = 0; j < J; ++j)
                if (depth[j] == d) { items.j[items.n] = (unsigned char)j; items.excl[items.n] = -1; items.kind[items.n] = 1; ++items.n; }
            for (int c = 1; c < J; ++c)
                if (depth[c] == d + 1) {
                    items.j[items.n] = (unsigned char)parent[c]; items.excl[items.n] = (signed char)c; items.kind[items.n] = 2; ++items.n;
                    rows.slot[rows.n++] = (unsigned char)c;
                }
            const int rc = level(items, rows, 1, E, D);
            if (rc) return rc;
            if (moments && rows.n) {
                hipLaunchKernelGGL(sk_moments_kernel, sk_corr_grid(G, rows.n * nf), dim3(SK_THREADS), lds, st, E, A, packed, nullptr, mpart,
                                   runs, rows, J, J, G, R);
                SE_CHECK_LAUNCH();
            }
        }
        if (moments) {
            hipLaunchKernelGGL(sk_edge_finish_kernel, dim3(J, nf), dim3(64), 0, st, mpart, sums, out.stats + (size_t)f0 * J * 4,
                               out.norms + (size_t)f0 * J * 3, out.valid + f0, J, records, uniform);
        } else {
            hipLaunchKernelGGL(sk_finish_kernel, dim3(fin_chunks, J, nf), dim3(SK_THREADS), 0, st, p, U, sums,
                               out.beliefs ? out.beliefs + (size_t)f0 * J * N : nullptr, out.joints + (size_t)f0 * J * 3,
                               out.evidence + (size_t)f0 * J, out.coupled + f0, J, voxels);
        }
        SE_CHECK_LAUNCH();
    }
    return 0;
}

// the checks both walks share, the tree they build
inline bool sk_walk_args(const int* parent, int frames, int J, int voxels, int G, int R, float floor, SkTree& tree, int* depth,
                         int& deepest) {
    if (!parent || frames < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R)) return false;
    if ((long long)G * G * G != (long long)voxels) return false;
    if (!(floor >= 0.f && floor <= 1.f)) return false;                                    // a NaN fails
    return sk_build_tree(parent, J, tree, depth, deepest);
}

}  // namespace

extern "C" long long se_skeleton_couple_scratch_bytes(int frames, int J, int G, int R) {
    if (frames < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R)) return 0;
    return sk_walk_scratch_bytes(frames, J, G, R, false);
}

extern "C" int se_skeleton_couple_f32(const float* prob, const float* coord, const float* taps, const int* parent, float* beliefs,
                                      float* joints, float* evidence, int* coupled, void* scratch, long long scratch_bytes, int frames,
                                      int J, int voxels, int G, int R, float floor, void* stream) {
    if (!prob || !coord || !taps || !parent || !joints || !evidence || !coupled || !scratch) return SE_ERR_BAD_ARG;
    SkTree tree{};
    int depth[SK_MAX_J], deepest;
    if (!sk_walk_args(parent, frames, J, voxels, G, R, floor, tree, depth, deepest)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, coord, taps, beliefs, joints, evidence, coupled, scratch}, 4)) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_skeleton_couple_scratch_bytes(frames, J, G, R)) return SE_ERR_BAD_ARG;
    const SkOutputs out{coord, beliefs, joints, evidence, coupled, nullptr, nullptr, nullptr, nullptr, nullptr};
    return sk_walk(prob, taps, parent, out, scratch, frames, J, voxels, G, R, floor, tree, depth, deepest, se_stream(stream));
}

extern "C" long long se_skeleton_edge_stats_scratch_bytes(int frames, int J, int G, int R) {
    if (frames < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R)) return 0;
    return sk_walk_scratch_bytes(frames, J, G, R, true);
}

extern "C" int se_skeleton_edge_stats_f32(const float* prob, const float* taps, const float* taps_r, const float* taps_r2,
                                          const int* parent, float* stats, float* norms, int* valid, void* scratch,
                                          long long scratch_bytes, int frames, int J, int voxels, int G, int R, float floor, void* stream) {
    if (!prob || !taps || !taps_r || !taps_r2 || !parent || !stats || !norms || !valid || !scratch) return SE_ERR_BAD_ARG;
    SkTree tree{};
    int depth[SK_MAX_J], deepest;
    if (!sk_walk_args(parent, frames, J, voxels, G, R, floor, tree, depth, deepest)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, taps, taps_r, taps_r2, stats, norms, valid, scratch}, 4)) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_skeleton_edge_stats_scratch_bytes(frames, J, G, R)) return SE_ERR_BAD_ARG;
    const SkOutputs out{nullptr, nullptr, nullptr, nullptr, nullptr, taps_r, taps_r2, stats, norms, valid};
    return sk_walk(prob, taps, parent, out, scratch, frames, J, voxels, G, R, floor, tree, depth, deepest, se_stream(stream));
}

// The upward walk for se_skeleton_upward_f32 (skeleton_sample.hip; declared in skeleton_shell.h): the pointers and the scratch size are
// that entry point's to check, the shape, the floor and the tree are checked here, before anything is launched.
long long sk_upward_scratch_bytes(int frames, int J, int G, int R) {
    if (frames < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R)) return 0;
    return ((long long)min(frames, SK_GROUP) * sk_upward_frame_floats(J, G) + sk_runs_ints(J, R)) * 4;
}

int sk_upward_walk(const float* prob, const float* taps, const int* parent, float* upward, float* sums, int* valid, void* scratch,
                   int frames, int J, int voxels, int G, int R, float floor, void* stream) {
    SkTree tree{};
    int depth[SK_MAX_J], deepest;
    if (!sk_walk_args(parent, frames, J, voxels, G, R, floor, tree, depth, deepest)) return SE_ERR_BAD_ARG;
    const SkOutputs out{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, valid, upward, sums};
    return sk_walk(prob, taps, parent, out, scratch, frames, J, voxels, G, R, floor, tree, depth, deepest, se_stream(stream));
}
