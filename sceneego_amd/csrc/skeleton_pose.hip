// Most probable pose: the max-product pass over the kinematic tree of the joint volumes of one frame, with the shells, the floor and
// the tree of the skeleton-coupled joints (sceneego_amd/skeleton_pose.py: SkeletonPose; VoxelNetwork_depth.skeleton_pose returns one).
// skeleton_prior.hip gives per joint a marginal; this gives the single most probable configuration of all joints.  The reference
// forces bone lengths onto a finished pose (utils/skeleton.py: _skeleton_resize).
// include/sceneego_hip.h states the definition operation by operation; tests/skeleton_pose_model.py restates it in numpy float32 and
// every value written here is compared with it bit for bit.  This file is built with -ffp-contract=off: one rounding per operation.
//
// Joints by depth level, deepest first (a call is a chain of launches bounded by the tree, not the batch):
//   sp_product_kernel   grid (CH, joints of the level x frames): A_j = p_j prod_c m_c, the children ascending, one rounding per factor;
//                       per chunk one record (max A, lowest index, max p, lowest index).
//   sp_fold_kernel      grid (joints of the level, frames), block 64: the row's records folded: M_j, peak_j and the peak of p_j.
//   sp_maxcorr_kernel   grid (G x ceil(G/16) x ceil(G/64), edges of the level x frames), block 256 - the hot path:
//                           e3(x) = max over d with w(d) != 0 and x + d inside the grid of s_j(x + d) w_j(d),  s_j = ldexp(A_j, -e_j)
//                           m_j(x) = jump > step ? jump : step,  step = keep e3(x),  jump = uniform best_j
//                       The tiling is sk_correlate_kernel's (skeleton_prior.hip): a workgroup owns the outputs (i, 16 rows j, 64 columns
//                       k), lane = k, a wave owns SK_JR = 4 consecutive j; per di whose plane has a tap the source plane i + di is
//                       staged in LDS with a zero halo of R - here scaled by 2^-e_j on the way in, so the rescaling is no pass of its
//                       own; the run table of sk_runs_kernel says which taps of a column are non-zero; taps are wave-uniform (scalar
//                       loads); four taps at a time feed 16 products and 16 maxima from a window of 7 rows, 3 carried in registers;
//                       consecutive lanes read consecutive LDS addresses.  The zero halo is right for a maximum too: 0 w is never > best.
//                       Per tap and row one multiply and one maximum where the sum form has one fused multiply-add.
//                       VALUES ONLY: the maximum is a value and does not depend on the order the taps are walked in, so it is taken
//                       as fmaxf from 0: a NaN candidate is passed over (fmaxf returns the other operand; the accumulator starts at 0
//                       and never becomes NaN), equal candidates give the same value.  No argument is kept here:
//   sp_walk_kernel      grid (frames), block 1024: solved or not (every M_j a finite number > 0); x_0 = peak_0, then for j = 1..J-1
//                       ascending the predecessor of edge j at the parent's voxel, recomputed there by sp_argmax: the same single
//                       multiplications, so the same bits, under the order "greater value, then lower tap index".  One voxel per
//                       edge and frame: no J N back-pointer volume, no compare and selects in the hot loop.
// se_shell_maxcorr_f32 and se_shell_argmax_i32 run sp_maxcorr_kernel and sp_argmax on stand-alone rows.
// se_skeleton_alternatives_f32 adds the downward pass on the same kernels (below, at sa_down_kernel): the max-marginals, per joint the
// best pose that moves it out of a window, with E and d beside A and m in the scratch (tests/skeleton_alternatives_model.py).
// ORDER.  No atomics, no sums: every result is a product, a comparison or a selection under a total order (row_reduce.h: peak_combine),
// so the results are bitwise identical from run to run and do not depend on how frames are batched into calls or groups.
// Scratch per frame in flight: A and m, 2 J N floats, the chunk records and the folded records; frames are walked in groups of SK_GROUP.
#include <float.h>

#include "row_reduce.h"
#include "skeleton_shell.h"

#pragma clang fp contract(off)

#define SP_REC 4                 // one record: max A, its index, max p, its index
#define SP_AT 1024               // threads of a workgroup that takes an argument (sp_argmax): 16 waves over the (2R+1)^3 taps

namespace {

// M -> e = ilogb(M) and best = ldexp(M, -e) in [1, 2); an M that is not a finite number > 0: e = 0, best NaN (the frame is not solved)
struct SpScale {
    int e;
    float best;
    bool alive;
};
__device__ __forceinline__ SpScale sp_scale(float M) {
    SpScale s;
    s.alive = M > 0.f && M <= FLT_MAX;                                   // a NaN never became a maximum; +inf fails here
    s.e = s.alive ? ilogbf(M) : 0;
    s.best = s.alive ? ldexpf(M, -s.e) : __int_as_float(0x7fc00000);
    return s;
}

// The calling workgroup (SP_AT threads, all of them): e3 at voxel x of the row `a` scaled by 2^down under the block of taps w, and the
// lowest tap index that attains it; (0, INT_MAX) when no candidate is > 0.  sm_p / sm_i [SP_AT / 64] may be reused from call to call.
// A thread takes four taps a round: the four weights and the four values (a tap that is past the block or leaves the grid reads
// voxel x itself and is not offered) are loaded before any is used, so eight loads are in flight where a tap-by-tap loop waits for two
// in turn - the back-walk is 14 such passes in sequence.
__device__ __forceinline__ Peak sp_argmax(const float* __restrict__ a, const float* __restrict__ w, int G, int R, int x, int down,
                                          float* sm_p, int* sm_i) {
    const int W = 2 * R + 1, W3 = W * W * W, t = threadIdx.x;
    const int xi = x / (G * G) - R, xj = x / G % G - R, xk = x % G - R;
    Peak pk = {0.f, INT_MAX};
    for (int t0 = t; t0 < W3; t0 += 4 * SP_AT) {
        float wv[4], v[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tap = t0 + u * SP_AT;
            const bool in = tap < W3;
            const int i = xi + tap / (W * W), j = xj + tap / W % W, k = xk + tap % W;
            ok[u] = in && i >= 0 && i < G && j >= 0 && j < G && k >= 0 && k < G;
            wv[u] = in ? w[tap] : 0.f;
            v[u] = a[ok[u] ? (i * G + j) * G + k : x];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float cand = ldexpf(v[u], down) * wv[u];
            if (ok[u] && wv[u] != 0.f && cand > 0.f) pk = peak_combine(pk, Peak{cand, t0 + u * SP_AT});      // a NaN never wins
        }
    }
    pk = wave_reduce_peak(pk);
    __syncthreads();                                                     // everyone is done with sm of the call before
    if ((t & 63) == 0) { sm_p[t >> 6] = pk.p; sm_i[t >> 6] = pk.idx; }
    __syncthreads();
    Peak r = {sm_p[0], sm_i[0]};
#pragma unroll
    for (int v = 1; v < SP_AT / 64; ++v) r = peak_combine(r, Peak{sm_p[v], sm_i[v]});
    return r;
}

// the taps lo..hi (dj + R) of one column, all non-zero: four at a time, then one at a time, as sk_run (skeleton_prior.hip) with a
// product and a maximum in place of the fused multiply-add.
__device__ __forceinline__ void sp_run(const float* __restrict__ wp, int W, const float* lp, int LW, int lo, int hi, float (&acc)[SK_JR]) {
    int d = lo;
    if (d + 3 <= hi) {
        float v0 = lp[(d + 0) * LW], v1 = lp[(d + 1) * LW], v2 = lp[(d + 2) * LW];
        for (; d + 3 <= hi; d += 4) {
            const float w0 = wp[(d + 0) * W], w1 = wp[(d + 1) * W], w2 = wp[(d + 2) * W], w3 = wp[(d + 3) * W];
            const float v3 = lp[(d + 3) * LW], v4 = lp[(d + 4) * LW], v5 = lp[(d + 5) * LW], v6 = lp[(d + 6) * LW];
            acc[0] = fmaxf(acc[0], w0 * v0); acc[1] = fmaxf(acc[1], w0 * v1); acc[2] = fmaxf(acc[2], w0 * v2); acc[3] = fmaxf(acc[3], w0 * v3);
            acc[0] = fmaxf(acc[0], w1 * v1); acc[1] = fmaxf(acc[1], w1 * v2); acc[2] = fmaxf(acc[2], w1 * v3); acc[3] = fmaxf(acc[3], w1 * v4);
            acc[0] = fmaxf(acc[0], w2 * v2); acc[1] = fmaxf(acc[1], w2 * v3); acc[2] = fmaxf(acc[2], w2 * v4); acc[3] = fmaxf(acc[3], w2 * v5);
            acc[0] = fmaxf(acc[0], w3 * v3); acc[1] = fmaxf(acc[1], w3 * v4); acc[2] = fmaxf(acc[2], w3 * v5); acc[3] = fmaxf(acc[3], w3 * v6);
            v0 = v4; v1 = v5; v2 = v6;
        }
    }
    for (; d <= hi; ++d) {
        const float w = wp[d * W];
#pragma unroll
        for (int x = 0; x < SK_JR; ++x) acc[x] = fmaxf(acc[x], w * lp[(d + x) * LW]);
    }
}
static_assert(SK_JR == 4, "sp_run is written out for four rows per lane");

// grid (G * ceil(G / SK_TJ) * ceil(G / SK_KC), rows), block 256, dynamic LDS (SK_TJ + 2R)(SK_KC + 2R) floats.
// tap_row != NULL (se_shell_maxcorr_f32): row r reads a + r N and taps[tap_row[r]] and writes scale_mul e3 to out + r N; a tap_row
// outside 0..tap_rows-1 fills the row with NaN.  tap_row == NULL (inside the tree): row r is joint map.slot[r % map.n] of frame
// r / map.n in [frame][J][N] buffers, its taps are the joint's, it is scaled by the exponent of its record's M on the way into LDS and
// the jump of that M is weighed against the step.
__global__ __launch_bounds__(SK_THREADS) void sp_maxcorr_kernel(const float* __restrict__ a, const float* __restrict__ taps,
                                                                const int* __restrict__ tap_row, const int* __restrict__ rec,
                                                                float* __restrict__ out, const int* __restrict__ runs, SkRows map,
                                                                int J, int tap_rows, int G, int R, float scale_mul, float uniform) {
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
    int tr, down = 0;
    float jump = 0.f;
    if (tap_row) {
        row = blockIdx.y;
        tr = tap_row[row];
    } else {
        const int f = blockIdx.y / map.n;
        tr = map.slot[blockIdx.y % map.n];
        row = (size_t)f * J + tr;
        const SpScale sc = sp_scale(__int_as_float(rec[row * SP_REC]));
        down = -sc.e;
        jump = uniform * sc.best;
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
    float acc[SK_JR] = {0.f, 0.f, 0.f, 0.f};                             // one maximum over all planes: from 0, it only grows
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
                if (jj >= 0 && jj < G && kk >= 0 && kk < G) v = ldexpf(src[jj * G + kk], down);
                lds[r * LW + c] = v;
            }
        }
        __syncthreads();
        for (int dk = 0; dk < W; ++dk) {                                 // dk + R
            const int lo1 = rp[dk * 4 + 0], hi1 = rp[dk * 4 + 1], lo2 = rp[dk * 4 + 2], h2 = rp[dk * 4 + 3];
            if (lo1 > hi1) continue;
            const float* wp = wt + (size_t)(di + R) * W * W + dk;
            const float* lp = lds + (wv * SK_JR) * LW + kl + dk;         // row (wv JR + x) + (dj + R), column kl + (dk + R)
            sp_run(wp, W, lp, LW, lo1, hi1, acc);
            const int hi2 = h2 & 0xff;
            if (lo2 <= hi2) {
                if (h2 >> 8) {
                    for (int d = hi1 + 1; d < lo2; ++d) {
                        const float w = wp[d * W];
                        if (w != 0.f) {
#pragma unroll
                            for (int x = 0; x < SK_JR; ++x) acc[x] = fmaxf(acc[x], w * lp[(d + x) * LW]);
                        }
                    }
                }
                sp_run(wp, W, lp, LW, lo2, hi2, acc);
            }
        }
    }
    if (k < G) {
#pragma unroll
        for (int x = 0; x < SK_JR; ++x)
            if (j0 + x < G) {
                float m = scale_mul * acc[x];                            // step
                if (!tap_row && jump > m) m = jump;                      // a NaN jump (no finite M) never takes it
                o[((size_t)i * G + j0 + x) * G + k] = m;
            }
    }
}

// grid (queries, rows), block SP_AT
__global__ __launch_bounds__(SP_AT) void sp_argmax_kernel(const float* __restrict__ a, const float* __restrict__ taps,
                                                               const int* __restrict__ tap_row, const int* __restrict__ query,
                                                               int* __restrict__ out_tap, float* __restrict__ out_value, int tap_rows,
                                                               int G, int R) {
    __shared__ float sm_p[SP_AT / 64];
    __shared__ int sm_i[SP_AT / 64];
    const int q = blockIdx.x, row = blockIdx.y, W = 2 * R + 1, N = G * G * G;
    const int tr = tap_row[row], x = query[q];
    const size_t o = (size_t)row * gridDim.x + q;
    if (tr < 0 || tr >= tap_rows || x < 0 || x >= N) {                   // uniform
        if (threadIdx.x == 0) { out_tap[o] = -1; out_value[o] = __int_as_float(0x7fc00000); }
        return;
    }
    const Peak pk = sp_argmax(a + (size_t)row * N, taps + (size_t)tr * W * W * W, G, R, x, 0, sm_p, sm_i);
    if (threadIdx.x == 0) { out_tap[o] = pk.idx == INT_MAX ? -1 : pk.idx; out_value[o] = pk.p; }
}

// The calling workgroup (SK_THREADS threads, all of them): the two running maxima of its chunk folded into one record at w.
__device__ __forceinline__ void sp_chunk_record(Peak pa, Peak pp, int* __restrict__ w) {
    __shared__ float sm_p[4][2];
    __shared__ int sm_i[4][2];
    const int t = threadIdx.x;
    pa = wave_reduce_peak(pa);
    pp = wave_reduce_peak(pp);
    if ((t & 63) == 0) {
        sm_p[t >> 6][0] = pa.p; sm_i[t >> 6][0] = pa.idx;
        sm_p[t >> 6][1] = pp.p; sm_i[t >> 6][1] = pp.idx;
    }
    __syncthreads();
    if (t < 2) {
        Peak r = {sm_p[0][t], sm_i[0][t]};
#pragma unroll
        for (int x = 1; x < 4; ++x) r = peak_combine(r, Peak{sm_p[x][t], sm_i[x][t]});
        w[2 * t + 0] = __float_as_int(r.p);
        w[2 * t + 1] = r.idx;
    }
}

// grid (CH, rows.n * frames), block 256.  prob, A, m [frames][J][N]; part [frames][J][CH][SP_REC]
__global__ __launch_bounds__(SK_THREADS) void sp_product_kernel(const float* __restrict__ prob, const float* __restrict__ m,
                                                                float* __restrict__ A, int* __restrict__ part, SkTree tree, SkRows rows,
                                                                int voxels) {
    const int t = threadIdx.x, f = blockIdx.y / rows.n, J = tree.J, j = rows.slot[blockIdx.y % rows.n];
    const size_t fb = (size_t)f * J * voxels;
    const float* p = prob + fb + (size_t)j * voxels;
    float* o = A + fb + (size_t)j * voxels;
    const int chunk = sk_chunk(voxels), c0 = blockIdx.x * chunk, c1 = min(c0 + chunk, voxels);
    Peak pa = {0.f, INT_MAX}, pp = {0.f, INT_MAX};                       // a value must be > 0 to be a maximum
    for (int n = c0 + t; n < c1; n += SK_THREADS) {
        const float pv = p[n];
        float v = pv;
        for (int c = j + 1; c < J; ++c)                                  // the children in ascending order (uniform)
            if (tree.parent[c] == j) v *= m[fb + (size_t)c * voxels + n];
        o[n] = v;
        if (v > 0.f) pa = peak_combine(pa, Peak{v, n});
        if (pv > 0.f) pp = peak_combine(pp, Peak{pv, n});
    }
    sp_chunk_record(pa, pp, part + (((size_t)f * J + j) * gridDim.x + blockIdx.x) * SP_REC);
}

// grid (rows.n, frames), block 64.  rec [frames][J][SP_REC]
__global__ __launch_bounds__(64) void sp_fold_kernel(const int* __restrict__ part, int* __restrict__ rec, SkRows rows, int J, int CH) {
    const int t = threadIdx.x, f = blockIdx.y, j = rows.slot[blockIdx.x];
    const size_t row = (size_t)f * J + j;
    Peak a = {0.f, INT_MAX}, p = {0.f, INT_MAX};
    for (int x = t; x < CH; x += 64) {
        const int* r = part + (row * CH + x) * SP_REC;
        a = peak_combine(a, Peak{__int_as_float(r[0]), r[1]});
        p = peak_combine(p, Peak{__int_as_float(r[2]), r[3]});
    }
    a = wave_reduce_peak(a);
    p = wave_reduce_peak(p);
    if (t == 0) {
        int* o = rec + row * SP_REC;
        o[0] = __float_as_int(a.p); o[1] = a.idx; o[2] = __float_as_int(p.p); o[3] = p.idx;
    }
}

// The voxel behind the message of a row at voxel x: pk = sp_argmax there, sc the scale of the row's maximum, peak its voxel.
__device__ __forceinline__ int sp_behind(Peak pk, SpScale sc, int peak, int x, int G, int R, float keep, float uniform, int& jumped) {
    const int W = 2 * R + 1;
    const float step = keep * pk.p, jump = uniform * sc.best;
    jumped = 1;
    if (jump > step) return peak;
    jumped = 0;
    if (pk.idx == INT_MAX) return peak;                                  // step = jump = 0: not reached from a value > 0
    const int d = pk.idx;                                                // the lowest attaining tap: the lowest voxel
    return ((x / (G * G) + d / (W * W) - R) * G + (x / G % G + d / W % W - R)) * G + (x % G + d % W - R);
}

// grid (frames), block SP_AT.  Outputs at the call's frame f0 + frame.
__global__ __launch_bounds__(SP_AT) void sp_walk_kernel(const float* __restrict__ A, const float* __restrict__ taps,
                                                             const int* __restrict__ rec, int* __restrict__ index,
                                                             int* __restrict__ jumped, int* __restrict__ exponent,
                                                             float* __restrict__ best_root, int* __restrict__ solved, SkTree tree, int G,
                                                             int R, float keep, float uniform) {
    __shared__ float sm_p[SP_AT / 64];
    __shared__ int sm_i[SP_AT / 64];
    __shared__ int pose[SK_MAX_J];
    const int t = threadIdx.x, f = blockIdx.x, J = tree.J, W = 2 * R + 1, N = G * G * G;
    const int* rf = rec + (size_t)f * J * SP_REC;
    int bad = 0;
    for (int j = t; j < J; j += SP_AT) bad |= !sp_scale(__int_as_float(rf[j * SP_REC])).alive;
    const bool fallback = __syncthreads_or(bad) != 0;
    int* oi = index + (size_t)f * J;
    int* oj = jumped + (size_t)f * J;
    int* oe = exponent + (size_t)f * J;
    if (t == 0) {
        solved[f] = fallback ? 0 : 1;
        best_root[f] = fallback ? __int_as_float(0x7fc00000) : sp_scale(__int_as_float(rf[0])).best;
    }
    if (fallback) {                                                      // uniform: every joint takes the peak of its own p
        for (int j = t; j < J; j += SP_AT) {
            const int at = rf[j * SP_REC + 3];
            oi[j] = (at >= 0 && at < N) ? at : -1;
            oj[j] = 0;
            oe[j] = 0;
        }
        return;
    }
    if (t == 0) { pose[0] = rf[1]; oi[0] = rf[1]; oj[0] = 0; oe[0] = sp_scale(__int_as_float(rf[0])).e; }
    for (int j = 1; j < J; ++j) {
        __syncthreads();                                                 // pose[parent] is written
        const int xp = min(max(pose[tree.parent[j]], 0), N - 1);         // always a voxel; the clamp only keeps a corrupted scratch inside the row
        const SpScale sc = sp_scale(__int_as_float(rf[j * SP_REC]));
        const Peak pk = sp_argmax(A + ((size_t)f * J + j) * N, taps + (size_t)j * W * W * W, G, R, xp, -sc.e, sm_p, sm_i);
        if (t == 0) {
            int jmp;
            const int x = sp_behind(pk, sc, rf[j * SP_REC + 1], xp, G, R, keep, uniform, jmp);
            pose[j] = x; oi[j] = x; oj[j] = jmp; oe[j] = sc.e;
        }
    }
}

inline long long sp_frame_words(int J, int G) {
    const long long N = (long long)G * G * G;
    return 2 * J * N + (long long)J * sk_chunks((int)N) * SP_REC + (long long)J * SP_REC;
}

// The upward pass of nf frames, shared by se_skeleton_pose_f32 and se_skeleton_alternatives_f32: A, m and the folded records, then the
// back-walk into the outputs (already at the group's first frame).
inline int sp_upward(hipStream_t st, const float* p, const float* taps, float* A, float* m, int* part, int* rec, const int* runs,
                     const SkTree& tree, const int* depth, int deepest, int nf, int voxels, int G, int R, float keep, float uniform,
                     int* index, int* jumped, int* exponent, float* best_root, int* solved) {
    const int J = tree.J, CH = sk_chunks(voxels), lds = sk_lds_bytes(R);
    for (int d = deepest; d >= 0; --d) {
        SkRows level{};
        for (int j = 0; j < J; ++j)
            if (depth[j] == d) level.slot[level.n++] = (unsigned char)j;
        hipLaunchKernelGGL(sp_product_kernel, dim3(CH, level.n * nf), dim3(SK_THREADS), 0, st, p, m, A, part, tree, level, voxels);
        SE_CHECK_LAUNCH();
        hipLaunchKernelGGL(sp_fold_kernel, dim3(level.n, nf), dim3(64), 0, st, part, rec, level, J, CH);
        SE_CHECK_LAUNCH();
        if (d > 0) {                                                     // every joint of a level below the root sends a message
            hipLaunchKernelGGL(sp_maxcorr_kernel, sk_corr_grid(G, level.n * nf), dim3(SK_THREADS), lds, st, A, taps, nullptr, rec, m,
                               runs, level, J, J, G, R, keep, uniform);
            SE_CHECK_LAUNCH();
        }
    }
    hipLaunchKernelGGL(sp_walk_kernel, dim3(nf), dim3(SP_AT), 0, st, A, taps, rec, index, jumped, exponent, best_root, solved, tree, G, R,
                       keep, uniform);
    SE_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Runner-up poses (se_skeleton_alternatives_f32): the downward max-product pass.  After the upward pass, joints by depth level,
// shallowest first:
//   sa_down_kernel      grid (CH, children of the level x frames): E_c = p_j [d_j] prod m_c', the siblings ascending, one rounding per
//                       factor; per chunk one record (max E, lowest index, -, -).  sp_fold_kernel folds them: G_c at epeak_c.
//   sp_maxcorr_kernel   the upward launch with E for A and the G_c records for the M_j records: d_c.  The same instantiation.
// then, once per group of frames:
//   sa_mu_kernel        grid (CH, J x frames): mu_j = s_j d_j (mu_0 = s_0), written out if asked for; per chunk one record (max mu,
//                       lowest index, max mu outside the window around x*_j, lowest index).  sp_fold_kernel folds them.
//   sa_walk_kernel      grid (anchors, frames), block SP_AT: the outputs of one anchor and its alternative pose, up along the
//                       downward edges and down along the upward ones, every step recomputed by sp_argmax as in sp_walk_kernel.
// A frame is complete when every M_j and every G_c is a finite number > 0 (sa_complete, uniform per workgroup).
__device__ __forceinline__ bool sa_complete(const int* __restrict__ rf, const int* __restrict__ ef, int J) {
    bool ok = sp_scale(__int_as_float(rf[0])).alive;
    for (int c = 1; c < J; ++c) ok = ok && sp_scale(__int_as_float(rf[c * SP_REC])).alive && sp_scale(__int_as_float(ef[c * SP_REC])).alive;
    return ok;
}

// grid (CH, rows.n * frames), block 256; rows: the children c of a level.  prob, m, d, E [frames][J][N]
__global__ __launch_bounds__(SK_THREADS) void sa_down_kernel(const float* __restrict__ prob, const float* __restrict__ m,
                                                             const float* __restrict__ d, float* __restrict__ E, int* __restrict__ part,
                                                             SkTree tree, SkRows rows, int voxels) {
    const int t = threadIdx.x, f = blockIdx.y / rows.n, J = tree.J, c = rows.slot[blockIdx.y % rows.n], j = tree.parent[c];
    const size_t fb = (size_t)f * J * voxels;
    const float* p = prob + fb + (size_t)j * voxels;
    const float* dj = d + fb + (size_t)j * voxels;
    float* o = E + fb + (size_t)c * voxels;
    const int chunk = sk_chunk(voxels), c0 = blockIdx.x * chunk, c1 = min(c0 + chunk, voxels);
    Peak pa = {0.f, INT_MAX};
    for (int n = c0 + t; n < c1; n += SK_THREADS) {
        float v = p[n];
        if (j > 0) v *= dj[n];
        for (int s = j + 1; s < J; ++s)                                  // the other children in ascending order (uniform)
            if (tree.parent[s] == j && s != c) v *= m[fb + (size_t)s * voxels + n];
        o[n] = v;
        if (v > 0.f) pa = peak_combine(pa, Peak{v, n});
    }
    sp_chunk_record(pa, Peak{0.f, INT_MAX}, part + (((size_t)f * J + c) * gridDim.x + blockIdx.x) * SP_REC);
}

// grid (CH, J * frames), block 256.  index and mm (NULL: not asked for) at the group's first frame.
__global__ __launch_bounds__(SK_THREADS) void sa_mu_kernel(const float* __restrict__ prob, const float* __restrict__ A,
                                                           const float* __restrict__ d, const int* __restrict__ rec,
                                                           const int* __restrict__ erec, const int* __restrict__ index,
                                                           float* __restrict__ mm, int* __restrict__ part, int J, int voxels, int G,
                                                           int separation) {
    const int t = threadIdx.x, f = blockIdx.y / J, j = blockIdx.y % J;
    const size_t row = (size_t)f * J + j, rb = row * voxels;
    const int chunk = sk_chunk(voxels), c0 = blockIdx.x * chunk, c1 = min(c0 + chunk, voxels);
    if (!sa_complete(rec + (size_t)f * J * SP_REC, erec + (size_t)f * J * SP_REC, J)) {      // uniform: the row is p, bit for bit
        if (mm)
            for (int n = c0 + t; n < c1; n += SK_THREADS) mm[rb + n] = prob[rb + n];
        return;
    }
    const int down = -sp_scale(__int_as_float(rec[row * SP_REC])).e;
    const int xs = min(max(index[row], 0), voxels - 1);                  // x*_j: a voxel in a solved frame
    const int xi = xs / (G * G), xj = xs / G % G, xk = xs % G;
    Peak pa = {0.f, INT_MAX}, pw = {0.f, INT_MAX};
    for (int n = c0 + t; n < c1; n += SK_THREADS) {
        float v = ldexpf(A[rb + n], down);
        if (j > 0) v *= d[rb + n];
        if (mm) mm[rb + n] = v;
        if (v > 0.f) {
            pa = peak_combine(pa, Peak{v, n});
            const int far = max(max(abs(n / (G * G) - xi), abs(n / G % G - xj)), abs(n % G - xk));
            if (far > separation) pw = peak_combine(pw, Peak{v, n});
        }
    }
    sp_chunk_record(pa, pw, part + (row * gridDim.x + blockIdx.x) * SP_REC);
}

// grid (J, frames), block SP_AT.  index and every output at the group's first frame.
__global__ __launch_bounds__(SP_AT) void sa_walk_kernel(const float* __restrict__ A, const float* __restrict__ E,
                                                        const float* __restrict__ d, const float* __restrict__ taps,
                                                        const int* __restrict__ rec, const int* __restrict__ erec,
                                                        const int* __restrict__ murec, const int* __restrict__ index,
                                                        int* __restrict__ down_exponent, float* __restrict__ mm_best,
                                                        float* __restrict__ pose_value, float* __restrict__ alt_value,
                                                        int* __restrict__ mm_peak, int* __restrict__ alt_index, int* __restrict__ alt_pose,
                                                        int* __restrict__ alt_jumped, int* __restrict__ complete, SkTree tree, int G, int R,
                                                        float keep, float uniform) {
    __shared__ float sm_p[SP_AT / 64];
    __shared__ int sm_i[SP_AT / 64];
    __shared__ int pose[SK_MAX_J], jmp[SK_MAX_J];
    const int t = threadIdx.x, a = blockIdx.x, f = blockIdx.y, J = tree.J, W = 2 * R + 1, N = G * G * G;
    const int* rf = rec + (size_t)f * J * SP_REC;
    const int* ef = erec + (size_t)f * J * SP_REC;
    const size_t row = (size_t)f * J + a;
    const bool ok = sa_complete(rf, ef, J);                              // uniform
    if (a == 0 && t == 0) complete[f] = ok ? 1 : 0;
    const int* mr = murec + row * SP_REC;
    const int at = ok && mr[3] != INT_MAX ? mr[3] : -1;                  // the anchor's voxel outside the window; uniform
    if (t == 0) {
        const float nan = __int_as_float(0x7fc00000);
        down_exponent[row] = ok && a > 0 ? sp_scale(__int_as_float(ef[a * SP_REC])).e : 0;
        mm_best[row] = ok ? __int_as_float(mr[0]) : nan;
        mm_peak[row] = ok && mr[1] != INT_MAX ? mr[1] : -1;
        alt_value[row] = ok ? __int_as_float(mr[2]) : nan;
        alt_index[row] = at;
        float pv = nan;
        if (ok) {                                                        // mu_a at x*_a: the operations of sa_mu_kernel
            const int xs = min(max(index[row], 0), N - 1);
            pv = ldexpf(A[row * N + xs], -sp_scale(__int_as_float(rf[a * SP_REC])).e);
            if (a > 0) pv *= d[row * N + xs];
        }
        pose_value[row] = pv;
    }
    int* op = alt_pose + row * J;
    int* oj = alt_jumped + row * J;
    if (at < 0) {                                                        // uniform: no alternative, or the frame is not complete
        for (int j = t; j < J; j += SP_AT) { op[j] = -1; oj[j] = 0; }
        return;
    }
    for (int j = t; j < J; j += SP_AT) { pose[j] = j == a ? at : -1; jmp[j] = 0; }
    for (int u = a; u > 0; u = tree.parent[u]) {                         // up: the parent voxel behind d_u at x_u
        __syncthreads();                                                 // pose[u] is written
        const int y = min(max(pose[u], 0), N - 1);
        const SpScale sc = sp_scale(__int_as_float(ef[u * SP_REC]));
        const Peak pk = sp_argmax(E + ((size_t)f * J + u) * N, taps + (size_t)u * W * W * W, G, R, y, -sc.e, sm_p, sm_i);
        if (t == 0) pose[tree.parent[u]] = sp_behind(pk, sc, ef[u * SP_REC + 1], y, G, R, keep, uniform, jmp[u]);
    }
    for (int j = 1; j < J; ++j) {                                        // down: the predecessor of upward edge j, as in sp_walk_kernel
        __syncthreads();                                                 // pose[parent] is written
        if (pose[j] >= 0) continue;                                      // uniform: on the way up
        const int xp = min(max(pose[tree.parent[j]], 0), N - 1);
        const SpScale sc = sp_scale(__int_as_float(rf[j * SP_REC]));
        const Peak pk = sp_argmax(A + ((size_t)f * J + j) * N, taps + (size_t)j * W * W * W, G, R, xp, -sc.e, sm_p, sm_i);
        if (t == 0) pose[j] = sp_behind(pk, sc, rf[j * SP_REC + 1], xp, G, R, keep, uniform, jmp[j]);
    }
    __syncthreads();
    for (int j = t; j < J; j += SP_AT) { op[j] = pose[j]; oj[j] = jmp[j]; }
}

inline long long sa_frame_words(int J, int G) {
    const long long N = (long long)G * G * G;
    return 4 * J * N + (long long)J * sk_chunks((int)N) * SP_REC + 3LL * J * SP_REC;
}

}  // namespace

extern "C" int se_shell_maxcorr_f32(const float* a, const float* taps, const int* tap_row, float* out, void* scratch,
                                    long long scratch_bytes, int rows, int tap_rows, int G, int R, float scale_mul, void* stream) {
    if (!a || !taps || !tap_row || !out || !scratch) return SE_ERR_BAD_ARG;
    if (rows < 1 || rows > 65535 || tap_rows < 1 || tap_rows > 65535 || !sk_shape_ok(G, R)) return SE_ERR_BAD_ARG;
    if (!se_aligned({a, taps, tap_row, out, scratch}, 4) || a == out) return SE_ERR_BAD_ARG;
    if (scratch_bytes < sk_runs_ints(tap_rows, R) * 4) return SE_ERR_BAD_ARG;
    hipStream_t st = se_stream(stream);
    int* runs = reinterpret_cast<int*>(scratch);
    hipLaunchKernelGGL(sk_runs_kernel, dim3(2 * R + 1, tap_rows), dim3(64), 0, st, taps, runs, R);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(sp_maxcorr_kernel, sk_corr_grid(G, rows), dim3(SK_THREADS), sk_lds_bytes(R), st, a, taps, tap_row, nullptr, out,
                       runs, SkRows{}, 0, tap_rows, G, R, scale_mul, 0.f);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_shell_argmax_i32(const float* a, const float* taps, const int* tap_row, const int* query, int* out_tap,
                                   float* out_value, int rows, int queries, int tap_rows, int G, int R, void* stream) {
    if (!a || !taps || !tap_row || !query || !out_tap || !out_value) return SE_ERR_BAD_ARG;
    if (rows < 1 || rows > 65535 || queries < 1 || tap_rows < 1 || tap_rows > 65535 || !sk_shape_ok(G, R)) return SE_ERR_BAD_ARG;
    if (!se_aligned({a, taps, tap_row, query, out_tap, out_value}, 4)) return SE_ERR_BAD_ARG;
    hipLaunchKernelGGL(sp_argmax_kernel, dim3(queries, rows), dim3(SP_AT), 0, se_stream(stream), a, taps, tap_row, query, out_tap,
                       out_value, tap_rows, G, R);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" long long se_skeleton_pose_scratch_bytes(int frames, int J, int G, int R) {
    if (frames < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R)) return 0;
    return ((long long)min(frames, SK_GROUP) * sp_frame_words(J, G) + sk_runs_ints(J, R)) * 4;
}

extern "C" int se_skeleton_pose_f32(const float* prob, const float* taps, const int* parent, int* index, int* jumped, int* exponent,
                                    float* best_root, int* solved, void* scratch, long long scratch_bytes, int frames, int J, int voxels,
                                    int G, int R, float floor, void* stream) {
    if (!prob || !taps || !parent || !index || !jumped || !exponent || !best_root || !solved || !scratch) return SE_ERR_BAD_ARG;
    if (frames < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R)) return SE_ERR_BAD_ARG;
    if ((long long)G * G * G != (long long)voxels) return SE_ERR_BAD_ARG;
    if (!(floor >= 0.f && floor <= 1.f)) return SE_ERR_BAD_ARG;                           // a NaN fails
    SkTree tree{};
    int depth[SK_MAX_J], deepest;
    if (!sk_build_tree(parent, J, tree, depth, deepest)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, taps, index, jumped, exponent, best_root, solved, scratch}, 4)) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_skeleton_pose_scratch_bytes(frames, J, G, R)) return SE_ERR_BAD_ARG;
    hipStream_t st = se_stream(stream);

    const size_t N = (size_t)voxels;
    const int group = min(frames, SK_GROUP), CH = sk_chunks(voxels);
    float* A = reinterpret_cast<float*>(scratch);
    float* m = A + (size_t)group * J * N;
    int* part = reinterpret_cast<int*>(m + (size_t)group * J * N);
    int* rec = part + (size_t)group * J * CH * SP_REC;
    int* runs = rec + (size_t)group * J * SP_REC;
    const float keep = 1.0f - floor, uniform = floor / (float)voxels;

    if (J > 1) {
        hipLaunchKernelGGL(sk_runs_kernel, dim3(2 * R + 1, J), dim3(64), 0, st, taps, runs, R);
        SE_CHECK_LAUNCH();
    }
    for (int f0 = 0; f0 < frames; f0 += group) {
        const int nf = min(group, frames - f0);
        const int rc = sp_upward(st, prob + (size_t)f0 * J * N, taps, A, m, part, rec, runs, tree, depth, deepest, nf, voxels, G, R, keep,
                                 uniform, index + (size_t)f0 * J, jumped + (size_t)f0 * J, exponent + (size_t)f0 * J, best_root + f0,
                                 solved + f0);
        if (rc) return rc;
    }
    return 0;
}

extern "C" long long se_skeleton_alternatives_scratch_bytes(int frames, int J, int G, int R) {
    if (frames < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R)) return 0;
    return ((long long)min(frames, SK_GROUP) * sa_frame_words(J, G) + sk_runs_ints(J, R)) * 4;
}

extern "C" int se_skeleton_alternatives_f32(const float* prob, const float* taps, const int* parent, int separation, int* index,
                                            int* jumped, int* exponent, float* best_root, int* solved, int* down_exponent,
                                            float* mm_best, float* pose_value, float* alt_value, int* mm_peak, int* alt_index,
                                            int* alt_pose, int* alt_jumped, int* complete, float* max_marginals, void* scratch,
                                            long long scratch_bytes, int frames, int J, int voxels, int G, int R, float floor,
                                            void* stream) {
    if (!prob || !taps || !parent || !index || !jumped || !exponent || !best_root || !solved || !scratch) return SE_ERR_BAD_ARG;
    if (!down_exponent || !mm_best || !pose_value || !alt_value || !mm_peak || !alt_index || !alt_pose || !alt_jumped || !complete)
        return SE_ERR_BAD_ARG;
    if (frames < 1 || J < 1 || J > SK_MAX_J || !sk_shape_ok(G, R) || separation < 0) return SE_ERR_BAD_ARG;
    if ((long long)G * G * G != (long long)voxels) return SE_ERR_BAD_ARG;
    if (!(floor >= 0.f && floor <= 1.f)) return SE_ERR_BAD_ARG;                           // a NaN fails
    SkTree tree{};
    int depth[SK_MAX_J], deepest;
    if (!sk_build_tree(parent, J, tree, depth, deepest)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, taps, index, jumped, exponent, best_root, solved, down_exponent, mm_best, pose_value, alt_value, mm_peak,
                     alt_index, alt_pose, alt_jumped, complete, max_marginals, scratch}, 4))
        return SE_ERR_BAD_ARG;
    if (max_marginals == prob) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_skeleton_alternatives_scratch_bytes(frames, J, G, R)) return SE_ERR_BAD_ARG;
    hipStream_t st = se_stream(stream);

    const size_t N = (size_t)voxels;
    const int group = min(frames, SK_GROUP), CH = sk_chunks(voxels);
    float* A = reinterpret_cast<float*>(scratch);
    float* m = A + (size_t)group * J * N;
    float* E = m + (size_t)group * J * N;
    float* dn = E + (size_t)group * J * N;
    int* part = reinterpret_cast<int*>(dn + (size_t)group * J * N);
    int* rec = part + (size_t)group * J * CH * SP_REC;
    int* erec = rec + (size_t)group * J * SP_REC;
    int* murec = erec + (size_t)group * J * SP_REC;
    int* runs = murec + (size_t)group * J * SP_REC;
    const float keep = 1.0f - floor, uniform = floor / (float)voxels;
    const int lds = sk_lds_bytes(R);
    SkRows all{};
    for (int j = 0; j < J; ++j) all.slot[all.n++] = (unsigned char)j;

    if (J > 1) {
        hipLaunchKernelGGL(sk_runs_kernel, dim3(2 * R + 1, J), dim3(64), 0, st, taps, runs, R);
        SE_CHECK_LAUNCH();
    }
    for (int f0 = 0; f0 < frames; f0 += group) {
        const int nf = min(group, frames - f0);
        const size_t fj = (size_t)f0 * J;
        const float* p = prob + fj * N;
        const int rc = sp_upward(st, p, taps, A, m, part, rec, runs, tree, depth, deepest, nf, voxels, G, R, keep, uniform, index + fj,
                                 jumped + fj, exponent + fj, best_root + f0, solved + f0);
        if (rc) return rc;
        for (int d = 1; d <= deepest; ++d) {                             // the children of the level above
            SkRows level{};
            for (int j = 0; j < J; ++j)
                if (depth[j] == d) level.slot[level.n++] = (unsigned char)j;
            hipLaunchKernelGGL(sa_down_kernel, dim3(CH, level.n * nf), dim3(SK_THREADS), 0, st, p, m, dn, E, part, tree, level, voxels);
            SE_CHECK_LAUNCH();
            hipLaunchKernelGGL(sp_fold_kernel, dim3(level.n, nf), dim3(64), 0, st, part, erec, level, J, CH);
            SE_CHECK_LAUNCH();
            hipLaunchKernelGGL(sp_maxcorr_kernel, sk_corr_grid(G, level.n * nf), dim3(SK_THREADS), lds, st, E, taps, nullptr, erec, dn,
                               runs, level, J, J, G, R, keep, uniform);
            SE_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(sa_mu_kernel, dim3(CH, J * nf), dim3(SK_THREADS), 0, st, p, A, dn, rec, erec, index + fj,
                           max_marginals ? max_marginals + fj * N : nullptr, part, J, voxels, G, separation);
        SE_CHECK_LAUNCH();
        hipLaunchKernelGGL(sp_fold_kernel, dim3(J, nf), dim3(64), 0, st, part, murec, all, J, CH);
        SE_CHECK_LAUNCH();
        hipLaunchKernelGGL(sa_walk_kernel, dim3(J, nf), dim3(SP_AT), 0, st, A, E, dn, taps, rec, erec, murec, index + fj,
                           down_exponent + fj, mm_best + fj, pose_value + fj, alt_value + fj, mm_peak + fj, alt_index + fj,
                           alt_pose + fj * J, alt_jumped + fj * J, complete + f0, tree, G, R, keep, uniform);
        SE_CHECK_LAUNCH();
    }
    return 0;
}
