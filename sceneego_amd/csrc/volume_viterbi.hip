// Most probable joint trajectory: the max-product (Viterbi) pass over the softmaxed joint volumes of a sequence
// (sceneego_amd/volume_viterbi.py: VolumeViterbi; VoxelNetwork_depth.volume_path returns one).  No counterpart in the reference.
// include/sceneego_hip.h states the definition operation by operation; tests/volume_viterbi_model.py restates it in numpy float32 and
// every value written here is compared with it bit for bit.  This file is built with -ffp-contract=off: one rounding per operation.
//
// Per frame and row (one joint of one track), with the scaled scores s of the frame before in `state`:
//     e1 = stage(s) along k, e2 = stage(e1) along j, e3 = stage(e2) along i         stage: max over d of v[n + d] w[d], with its argmax
//     step = keep e3(x),  jump = uniform best_prev;  m = jump > step ? jump : step;  a = p m
//     M = max a, peak = its lowest index, e = ilogb(M), s' = ldexp(a, -e)            or, without a prior or with an M that is not a
//                                                                                   finite number > 0:  a = p (restart), back = -1
// Three launches per frame, mirroring the filter's (volume_filter.hip), and one more per call:
//   vv_stage_kj_kernel  grid (G, rows), block 256: one i-plane [G j][G k] of s staged in LDS (scaled by the exponent of the frame before
//                       on the way in), the k stage into a second LDS plane, the j stage from there; e2 (float32) and the two winning
//                       offsets (int8 each) go to scratch.  (2 G + 2 R) G floats of LDS: 38 KB at 64^3 and R = 10, 144 KB at 128^3 and R = 16.
//   vv_update_kernel    grid (G, rows), block 256: the slab [G i][G k] of e2 and of the j offsets at one j staged in LDS (26 KB; 96 KB),
//                       the i stage, the composition of the three offsets into the predecessor voxel (the k offset is one gathered
//                       byte), step or jump, the product with p.  The raw a goes to `state`, the back-pointer to `back_out`, the
//                       workgroup's (max a, lowest index) and (max p, lowest index) to one record of 4 words.
//   vv_fold_kernel      grid (chunks, rows), block 256: every workgroup folds the row's G records, decides the restart and, for a row
//                       that restarts WITH a prior (the others were written as copies by the update pass), writes its share of the
//                       copy of p and of the -1 back-pointers; chunk 0 writes peak, best, exponent and restarted of the frame.
//   vv_scale_kernel     once per call: `state` holds the raw a of the last frame and is scaled by that frame's exponent, so the state a
//                       call returns is the scaled one; chunk 0 hands peak and best on in peak_state / best_state.
// Inside a call the scaling is applied when the next frame stages the state: ldexp of the same value by the same exponent, so the bits do
// not depend on how the frames are cut into calls.
// A thread owns column k of the staged plane and every (256 / W)-th row of it, W the power of two >= G: any G in 2..128.  It takes
// SE_VV_ROWS = 4 of its rows through the tap loop together: a tap is a product, a comparison and two selects that wait for the `best`
// of the tap before, and four rows are four independent chains.  For that the planes the j and the i stage read carry R rows of zeros
// on either side, so that every row runs the same 2 R + 1 taps: a tap that leaves the grid reads 0, its candidate 0 w is never > best
// (best starts at 0 and only grows; 0 inf = NaN fails too), which is the definition's "skipping taps that leave the grid" bit for bit.
//
// BYTE MODEL per frame, row and voxel: the k/j stage reads s and writes e2 and two offset bytes (10 B); the update pass reads e2, the
// two offset bytes and p and writes a and the back-pointer (18 B): 28 B, the filter's figure (its third pass is the division; here the
// fold touches voxels only on a restart).  The scale pass adds 8 B per row and voxel per CALL.  The offset gather (one byte at
// (i', j', k)) stays inside the row's plane set that the k/j stage just wrote.
//
// ORDER.  No atomics, no sums: every result is a product, a comparison or a selection under the total order "greater value, then lower
// index" (row_reduce.h: peak_combine, associative and commutative), so any reduction tree gives the same bits.  Back-pointers and scores
// are written with plain vector stores.
//
// THE WALK (vv_path_kernel, one lane per row, sequential over the frames of a stored chunk, last chunk first, the cursor carried in
// device memory) and THE REFINEMENT (vv_refine_kernel, one lane per (frame, row): float64 sums over the window in ascending flat index,
// as joint_modes.hip does its windows) follow the header's definition.
#include <float.h>

#include "row_reduce.h"
#include "volume_grid.h"          // the limits, the shape predicate, the launch parameters and the argument gate: shared with volume_filter.hip

#pragma clang fp contract(off)

#define SE_VV_REC 4               // max a, its index, max p, its index
#define SE_VV_MAX_REFINE 3
#define SE_VV_JUMP (1 << 30)
#define SE_VV_ROWS 4              // rows of its column a thread takes through the tap loop together: independent compare-select chains
#define SE_VB_REC 12              // the backward pass: max r, max p, max mm, max mm outside the window (value, index each), mm(x*), 3 unused
#define SE_VB_TAPS 36             // words of scratch for the reversed taps (2 SE_VG_MAX_R + 1, rounded up to 16 bytes)

namespace {

// The row has a prior at this frame.  Frames behind the call's first: the frame before left a peak (peak_prev = its `peak` output).
// The call's first frame: the caller says so and the state it hands over has a peak.  Nothing read here is written by a launch of the
// same frame, so the three passes agree.
__device__ __forceinline__ bool vv_prior(const int* __restrict__ have_prior, const int* __restrict__ peak_state,
                                         const int* __restrict__ peak_prev, int row) {
    if (peak_prev != nullptr) return peak_prev[row] >= 0;
    return have_prior != nullptr && have_prior[row] != 0 && peak_state[row] >= 0;
}

// grid (G, rows), block 256, dynamic LDS (2 G + 2 R) G floats
__global__ __launch_bounds__(SE_VG_THREADS) void vv_stage_kj_kernel(const float* __restrict__ state, const float* __restrict__ taps,
                                                                    const int* __restrict__ have_prior,
                                                                    const int* __restrict__ peak_state,
                                                                    const int* __restrict__ peak_prev, const int* __restrict__ exp_prev,
                                                                    float* __restrict__ e2, signed char* __restrict__ off_k,
                                                                    signed char* __restrict__ off_j, int G, int voxels, int R,
                                                                    int wshift) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float w[2 * SE_VG_MAX_R + 1];
    const int t = threadIdx.x, i = blockIdx.x, row = blockIdx.y;
    if (!vv_prior(have_prior, peak_state, peak_prev, row)) return;  // uniform: the row restarts, nothing of this pass is read
    const int GG = G * G;
    float* A = lds;                                                 // [G j][G k]
    float* Bk = lds + GG;                                           // [R + G + R j][G k]: R rows of zeros on either side (vv_update_kernel)
    const size_t base = (size_t)row * voxels + (size_t)i * GG;
    const int down = exp_prev != nullptr ? -exp_prev[row] : 0;      // the state of the call's first frame arrives scaled
    for (int e = t; e < GG; e += SE_VG_THREADS) A[e] = ldexpf(state[base + e], down);
    for (int e = t; e < R * G; e += SE_VG_THREADS) { Bk[e] = 0.f; Bk[(R + G) * G + e] = 0.f; }
    if (t <= 2 * R) w[t] = taps[t];
    __syncthreads();
    const int k = t & ((1 << wshift) - 1), jr = t >> wshift, RP = SE_VG_THREADS >> wshift;
    if (k < G) {
        const int lo = max(-R, -k), hi = min(R, G - 1 - k);         // the taps that stay inside the row
        for (int j0 = jr; j0 < G; j0 += SE_VV_ROWS * RP) {
            float best[SE_VV_ROWS];
            int off[SE_VV_ROWS], at[SE_VV_ROWS];
#pragma unroll
            for (int u = 0; u < SE_VV_ROWS; ++u) { at[u] = min(j0 + u * RP, G - 1) * G + k; best[u] = 0.f; off[u] = 0; }
            for (int d = lo; d <= hi; ++d) {
                const float wd = w[d + R];
#pragma unroll
                for (int u = 0; u < SE_VV_ROWS; ++u) {
                    const float cand = A[at[u] + d] * wd;
                    if (cand > best[u]) { best[u] = cand; off[u] = d; }      // a NaN never wins; equal candidates keep the lowest d
                }
            }
#pragma unroll
            for (int u = 0; u < SE_VV_ROWS; ++u) {
                const int j = j0 + u * RP;
                if (j < G) { Bk[(R + j) * G + k] = best[u]; off_k[base + j * G + k] = (signed char)off[u]; }
            }
        }
    }
    __syncthreads();
    if (k < G) {
        for (int j0 = jr; j0 < G; j0 += SE_VV_ROWS * RP) {
            float best[SE_VV_ROWS];
            int off[SE_VV_ROWS], at[SE_VV_ROWS];
#pragma unroll
            for (int u = 0; u < SE_VV_ROWS; ++u) { at[u] = (R + min(j0 + u * RP, G - 1)) * G + k; best[u] = 0.f; off[u] = 0; }
            for (int d = -R; d <= R; ++d) {                         // a tap that leaves the grid reads a zero of the padding: it never wins
                const float wd = w[d + R];
#pragma unroll
                for (int u = 0; u < SE_VV_ROWS; ++u) {
                    const float cand = Bk[at[u] + d * G] * wd;
                    if (cand > best[u]) { best[u] = cand; off[u] = d; }
                }
            }
#pragma unroll
            for (int u = 0; u < SE_VV_ROWS; ++u) {
                const int j = j0 + u * RP;
                if (j < G) { e2[base + j * G + k] = best[u]; off_j[base + j * G + k] = (signed char)off[u]; }
            }
        }
    }
}

// grid (G, rows), block 256, dynamic LDS (G + 2 R) G floats and G^2 bytes.  KEEP (se_volume_viterbi_keep_f32): the raw a also goes to
// `scores`, the frame's own slice of scores_out; the instantiation without it is the kernel se_volume_viterbi_f32 has always launched.
template <bool KEEP>
__global__ __launch_bounds__(SE_VG_THREADS) void vv_update_kernel(const float* __restrict__ prob, const float* __restrict__ taps,
                                                                  const int* __restrict__ have_prior, const int* __restrict__ peak_state,
                                                                  const float* __restrict__ best_state,
                                                                  const int* __restrict__ peak_prev, const float* __restrict__ best_prev,
                                                                  const float* __restrict__ e2, const signed char* __restrict__ off_k,
                                                                  const signed char* __restrict__ off_j, float* __restrict__ state,
                                                                  int* __restrict__ back, int* __restrict__ rec, int G, int voxels,
                                                                  int R, int wshift, float keep, float uniform,
                                                                  float* __restrict__ scores) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float w[2 * SE_VG_MAX_R + 1];
    __shared__ float sm_p[4][2];
    __shared__ int sm_i[4][2];
    const int t = threadIdx.x, j = blockIdx.x, row = blockIdx.y;
    const bool prior = vv_prior(have_prior, peak_state, peak_prev, row);    // uniform
    const int k = t & ((1 << wshift) - 1), ir = t >> wshift, RP = SE_VG_THREADS >> wshift;
    const size_t base = (size_t)row * voxels;
    float* slab = lds;                                              // [R + G + R i][G k]: R rows of zeros on either side
    signed char* dj = reinterpret_cast<signed char*>(lds + (G + 2 * R) * G);        // [G i][G k]
    float jump = 0.f;
    int jump_to = -1;
    if (prior) {
        if (k < G)
            for (int i = ir; i < G; i += RP) {
                const size_t n = base + ((size_t)i * G + j) * G + k;
                slab[(R + i) * G + k] = e2[n];
                dj[i * G + k] = off_j[n];
            }
        for (int e = t; e < R * G; e += SE_VG_THREADS) { slab[e] = 0.f; slab[(R + G) * G + e] = 0.f; }
        if (t <= 2 * R) w[t] = taps[t];
        jump = uniform * (peak_prev != nullptr ? best_prev[row] : best_state[row]);
        jump_to = (peak_prev != nullptr ? peak_prev[row] : peak_state[row]) | SE_VV_JUMP;
    }
    __syncthreads();
    Peak pa = {0.f, INT_MAX}, pp = {0.f, INT_MAX};                  // a value must be > 0 to be a maximum
    if (k < G) {
        for (int i0 = ir; i0 < G; i0 += SE_VV_ROWS * RP) {
            float best[SE_VV_ROWS], p[SE_VV_ROWS];
            int off[SE_VV_ROWS], at[SE_VV_ROWS];
#pragma unroll
            for (int u = 0; u < SE_VV_ROWS; ++u) {
                const int i = min(i0 + u * RP, G - 1);
                p[u] = prob[base + (i * G + j) * G + k];
                at[u] = (R + i) * G + k;
                best[u] = 0.f;
                off[u] = 0;
            }
            if (prior) {
                for (int d = -R; d <= R; ++d) {                     // a tap that leaves the grid reads a zero of the padding: it never wins
                    const float wd = w[d + R];
#pragma unroll
                    for (int u = 0; u < SE_VV_ROWS; ++u) {
                        const float cand = slab[at[u] + d * G] * wd;
                        if (cand > best[u]) { best[u] = cand; off[u] = d; }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < SE_VV_ROWS; ++u) {
                const int i = i0 + u * RP;
                if (i >= G) continue;
                const int n = (i * G + j) * G + k;
                float a = p[u];
                int pred = -1;
                if (prior) {
                    // the predecessor voxel: the three winning offsets composed.  An offset is only ever that of a tap inside the
                    // grid; the clamps only keep a corrupted scratch from steering the gather outside the row.
                    const int ip = min(max(i + off[u], 0), G - 1);
                    const int jp = min(max(j + (int)dj[ip * G + k], 0), G - 1);
                    const int kp = min(max(k + (int)off_k[base + ((size_t)ip * G + jp) * G + k], 0), G - 1);
                    const float step = keep * best[u];
                    float m = step;
                    pred = (ip * G + jp) * G + kp;
                    if (jump > step) { m = jump; pred = jump_to; }
                    a = p[u] * m;
                }
                state[base + n] = a;
                if (KEEP) scores[base + n] = a;
                back[base + n] = pred;
                if (a > 0.f) pa = peak_combine(pa, Peak{a, n});
                if (p[u] > 0.f) pp = peak_combine(pp, Peak{p[u], n});
            }
        }
    }
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
        int* o = rec + ((size_t)row * G + j) * SE_VV_REC + 2 * t;
        o[0] = __float_as_int(r.p);
        o[1] = r.idx;
    }
}

// grid (chunks, rows), block 256.  KEEP: a restart with a prior copies p into `scores` as well
template <bool KEEP>
__global__ __launch_bounds__(SE_VG_THREADS) void vv_fold_kernel(const float* __restrict__ prob, const int* __restrict__ rec,
                                                                const int* __restrict__ have_prior, const int* __restrict__ peak_state,
                                                                const int* __restrict__ peak_prev, float* __restrict__ state,
                                                                int* __restrict__ back, int* __restrict__ peak, float* __restrict__ best,
                                                                int* __restrict__ exponent, int* __restrict__ restarted, int G,
                                                                int voxels, float* __restrict__ scores) {
    __shared__ float fin_p[2];
    __shared__ int fin_i[2];
    const int t = threadIdx.x, row = blockIdx.y;
    if (t < 64) {
        Peak a = {0.f, INT_MAX}, p = {0.f, INT_MAX};
        for (int x = t; x < G; x += 64) {
            const int* r = rec + ((size_t)row * G + x) * SE_VV_REC;
            a = peak_combine(a, Peak{__int_as_float(r[0]), r[1]});
            p = peak_combine(p, Peak{__int_as_float(r[2]), r[3]});
        }
        a = wave_reduce_peak(a);
        p = wave_reduce_peak(p);
        if (t == 0) { fin_p[0] = a.p; fin_i[0] = a.idx; fin_p[1] = p.p; fin_i[1] = p.idx; }
    }
    __syncthreads();
    const bool prior = vv_prior(have_prior, peak_state, peak_prev, row);
    const bool restart = !prior || !(fin_p[0] > 0.f && fin_p[0] <= FLT_MAX);        // a NaN never became a maximum; +inf fails here
    if (blockIdx.x == 0 && t == 0) {
        const float M = restart ? fin_p[1] : fin_p[0];
        const bool alive = M > 0.f && M <= FLT_MAX;                 // no finite positive cell in p either: the next frame restarts
        const int e = alive ? ilogbf(M) : 0;
        peak[row] = alive ? (restart ? fin_i[1] : fin_i[0]) : -1;
        best[row] = alive ? ldexpf(M, -e) : __int_as_float(0x7fc00000);
        exponent[row] = e;
        restarted[row] = restart ? 1 : 0;
    }
    if (!restart || !prior) return;                                 // a row without a prior was written as the copy already
    const size_t base = (size_t)row * voxels;
    for (int n = blockIdx.x * SE_VG_THREADS + t; n < voxels; n += gridDim.x * SE_VG_THREADS) {
        state[base + n] = prob[base + n];                           // bit for bit
        if (KEEP) scores[base + n] = prob[base + n];
        back[base + n] = -1;
    }
}

// grid (chunks, rows), block 256: the state a call returns is the scaled one
__global__ __launch_bounds__(SE_VG_THREADS) void vv_scale_kernel(float* __restrict__ state, const int* __restrict__ exponent,
                                                                 const int* __restrict__ peak, const float* __restrict__ best,
                                                                 int* __restrict__ peak_state, float* __restrict__ best_state,
                                                                 int voxels) {
    const int t = threadIdx.x, row = blockIdx.y;
    const int down = -exponent[row];
    const size_t base = (size_t)row * voxels;
    for (int n = blockIdx.x * SE_VG_THREADS + t; n < voxels; n += gridDim.x * SE_VG_THREADS) state[base + n] = ldexpf(state[base + n], down);
    if (blockIdx.x == 0 && t == 0) { peak_state[row] = peak[row]; best_state[row] = best[row]; }
}

// grid (ceil(rows / 64)), block 64: one lane per row, sequential over the frames from last to first
__global__ __launch_bounds__(64) void vv_path_kernel(const int* __restrict__ back, const int* __restrict__ peak,
                                                     const int* __restrict__ restarted, int* __restrict__ cursor,
                                                     int* __restrict__ index, int* __restrict__ jumped, int frames, int rows, int voxels,
                                                     int have_next) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    // the cursor: the voxel the frame behind this chunk points back to, or < 0: that frame starts a segment (or there is none)
    int x = have_next ? cursor[row] : -1;
    for (int f = frames - 1; f >= 0; --f) {
        const size_t fr = (size_t)f * rows + row;
        if (x < 0 || x >= voxels) x = peak[fr];                     // the frame's own peak (-1: it has none); never an index outside the row
        if (x >= voxels) x = -1;
        const int b = (x >= 0 && restarted[fr] == 0) ? back[fr * voxels + x] : -1;
        index[fr] = x;
        jumped[fr] = (b >= 0 && (b & SE_VV_JUMP)) ? 1 : 0;
        x = b >= 0 ? (b & (SE_VV_JUMP - 1)) : -1;
    }
    cursor[row] = x;
}

// grid (ceil(frames rows / 64)), block 64: one lane per (frame, row)
__global__ __launch_bounds__(64) void vv_refine_kernel(const float* __restrict__ prob, const float* __restrict__ coord,
                                                       const int* __restrict__ index, float* __restrict__ joints, int total, int voxels,
                                                       int G, int refine) {
    const int fr = blockIdx.x * 64 + threadIdx.x;
    if (fr >= total) return;
    float* o = joints + (size_t)fr * 3;
    const int x = index[fr];
    if (x < 0 || x >= voxels) {
        o[0] = o[1] = o[2] = __int_as_float(0x7fc00000);
        return;
    }
    const float* c = coord + (size_t)x * 3;
    float jx = c[0], jy = c[1], jz = c[2];                          // the voxel centre
    if (refine > 0) {
        const int ci = x / (G * G), cj = (x / G) % G, ck = x % G;
        const int ia = max(ci - refine, 0), ib = min(ci + refine, G - 1);
        const int ja = max(cj - refine, 0), jb = min(cj + refine, G - 1);
        const int ka = max(ck - refine, 0), kb = min(ck + refine, G - 1);
        const float* v = prob + (size_t)fr * voxels;
        double m = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
        for (int i = ia; i <= ib; ++i)
            for (int j = ja; j <= jb; ++j)
                for (int k = ka; k <= kb; ++k) {                    // ascending flat index
                    const size_t n = ((size_t)i * G + j) * G + k;
                    const float pf = v[n];
                    if (pf != pf) continue;                         // a NaN cell is passed over
                    const double p = (double)pf;
                    m += p;
                    mx += p * (double)coord[n * 3 + 0];             // exact products: 24 x 24 bits
                    my += p * (double)coord[n * 3 + 1];
                    mz += p * (double)coord[n * 3 + 2];
                }
        if (m > 0.0 && m <= DBL_MAX) {
            jx = (float)(mx / m);
            jy = (float)(my / m);
            jz = (float)(mz / m);
        }
    }
    o[0] = jx; o[1] = jy; o[2] = jz;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// THE BACKWARD PASS (se_volume_viterbi_back_f32): the max-marginals mm_t(x) = s_t(x) m_t(x), the score of the best whole trajectory
// that is at x in frame t.  m_t is the forward recursion's m taken the other way: the same three stages on the scaled r_{t+1} =
// p_{t+1} m_{t+1} with the taps reversed (w_rev[d] = w[-d]: the transition from x to the successor x + d has the score the forward pass
// gives the predecessor offset -d), so vv_stage_kj_kernel runs unchanged on r with the reversed vector, the `link` of the frame (the
// peak of r_{t+1}, or -1: nothing to come from) in the place of its peak_prev.  Per frame, last to first:
//   vv_stage_kj_kernel  as above, skipped by rows that are not linked
//   vb_update_kernel    vv_update_kernel's tap loop, LDS slab and footprint; the epilogue takes the two products r = p m and
//                       mm = s m (s = ldexp(scores, -exponent)), writes r, the successor pointer (optional; it may overwrite the
//                       voxel's score: the thread has read it) and mm (optional), and folds four (max, lowest index) records: r, p,
//                       mm, and mm over the voxels further than `separation` (Chebyshev, in voxels) from the path voxel x*; the
//                       thread that owns x* hands mm(x*) on.  36 B per voxel with the pointers, 28 + 4 (scores) + 4 (pointers).
//   vb_fold_kernel      folds the row's G records; an r without a finite positive maximum under a link is a backward death: every
//                       workgroup then writes its share of r = p, pointers -1, mm NaN; chunk 0 writes the frame's outputs and the
//                       link of the frame before.
// and per call vb_taps_kernel (the reversed taps) and vb_scale_kernel (the carried r scaled; link, best, complete handed on).
__global__ __launch_bounds__(64) void vb_taps_kernel(const float* __restrict__ taps, float* __restrict__ taps_rev, int R) {
    if ((int)threadIdx.x <= 2 * R) taps_rev[threadIdx.x] = taps[2 * R - threadIdx.x];
}

// grid (G, rows), block 256, dynamic LDS (G + 2 R) G floats and G^2 bytes.  `scores` and `succ` may be the same memory: neither is
// __restrict__, and a thread loads the scores of its four voxels before it stores their pointers.
__global__ __launch_bounds__(SE_VG_THREADS) void vb_update_kernel(const float* __restrict__ prob, const float* __restrict__ taps_rev,
                                                                  const int* __restrict__ link_in, const float* __restrict__ best_in,
                                                                  const float* scores, const int* __restrict__ exp_f,
                                                                  const int* __restrict__ index_f, const float* __restrict__ e2,
                                                                  const signed char* __restrict__ off_k,
                                                                  const signed char* __restrict__ off_j, float* __restrict__ r_state,
                                                                  int* succ, float* __restrict__ mm_out, int* __restrict__ rec, int G,
                                                                  int voxels, int R, int wshift, float keep, float uniform,
                                                                  int separation) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float w[2 * SE_VG_MAX_R + 1];
    __shared__ float sm_p[4][4];
    __shared__ int sm_i[4][4];
    __shared__ float sm_pv;
    const int t = threadIdx.x, j = blockIdx.x, row = blockIdx.y;
    const bool linked = link_in != nullptr && link_in[row] >= 0;            // uniform
    const int k = t & ((1 << wshift) - 1), ir = t >> wshift, RP = SE_VG_THREADS >> wshift;
    const size_t base = (size_t)row * voxels;
    float* slab = lds;                                              // [R + G + R i][G k]: R rows of zeros on either side
    signed char* dj = reinterpret_cast<signed char*>(lds + (G + 2 * R) * G);        // [G i][G k]
    int xs = index_f[row];                                          // the path voxel x* of the frame, or none
    if (xs >= voxels) xs = -1;
    const int xi = xs / (G * G), xj = (xs / G) % G, xk = xs % G;    // read only with xs >= 0
    const int down = -exp_f[row];
    float jump = 0.f;
    int jump_to = -1;
    if (t == 0) sm_pv = 0.f;
    if (linked) {
        if (k < G)
            for (int i = ir; i < G; i += RP) {
                const size_t n = base + ((size_t)i * G + j) * G + k;
                slab[(R + i) * G + k] = e2[n];
                dj[i * G + k] = off_j[n];
            }
        for (int e = t; e < R * G; e += SE_VG_THREADS) { slab[e] = 0.f; slab[(R + G) * G + e] = 0.f; }
        if (t <= 2 * R) w[t] = taps_rev[t];
        jump = uniform * best_in[row];
        jump_to = link_in[row] | SE_VV_JUMP;
    }
    __syncthreads();
    Peak pr = {0.f, INT_MAX}, pp = {0.f, INT_MAX}, pm = {0.f, INT_MAX}, pa = {0.f, INT_MAX};   // a value must be > 0 to be a maximum
    if (k < G) {
        const int far_jk = max(abs(j - xj), abs(k - xk));
        for (int i0 = ir; i0 < G; i0 += SE_VV_ROWS * RP) {
            float best[SE_VV_ROWS], p[SE_VV_ROWS], sc[SE_VV_ROWS];
            int off[SE_VV_ROWS], at[SE_VV_ROWS];
#pragma unroll
            for (int u = 0; u < SE_VV_ROWS; ++u) {
                const int i = min(i0 + u * RP, G - 1);
                p[u] = prob[base + (i * G + j) * G + k];
                sc[u] = ldexpf(scores[base + (i * G + j) * G + k], down);
                at[u] = (R + i) * G + k;
                best[u] = 0.f;
                off[u] = 0;
            }
            if (linked) {
                for (int d = -R; d <= R; ++d) {                     // a tap that leaves the grid reads a zero of the padding: it never wins
                    const float wd = w[d + R];
#pragma unroll
                    for (int u = 0; u < SE_VV_ROWS; ++u) {
                        const float cand = slab[at[u] + d * G] * wd;
                        if (cand > best[u]) { best[u] = cand; off[u] = d; }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < SE_VV_ROWS; ++u) {
                const int i = i0 + u * RP;
                if (i >= G) continue;
                const int n = (i * G + j) * G + k;
                float r = p[u], mm = sc[u];
                int next = -1;
                if (linked) {
                    // the successor voxel: the three winning offsets composed, clamped as in vv_update_kernel
                    const int ip = min(max(i + off[u], 0), G - 1);
                    const int jp = min(max(j + (int)dj[ip * G + k], 0), G - 1);
                    const int kp = min(max(k + (int)off_k[base + ((size_t)ip * G + jp) * G + k], 0), G - 1);
                    const float step = keep * best[u];
                    float m = step;
                    next = (ip * G + jp) * G + kp;
                    if (jump > step) { m = jump; next = jump_to; }
                    r = p[u] * m;
                    mm = sc[u] * m;
                }
                r_state[base + n] = r;
                if (succ != nullptr) succ[base + n] = next;
                if (mm_out != nullptr) mm_out[base + n] = mm;
                if (r > 0.f) pr = peak_combine(pr, Peak{r, n});
                if (p[u] > 0.f) pp = peak_combine(pp, Peak{p[u], n});
                if (mm > 0.f) pm = peak_combine(pm, Peak{mm, n});
                if (xs >= 0) {
                    if (mm > 0.f && max(far_jk, abs(i - xi)) > separation) pa = peak_combine(pa, Peak{mm, n});
                    if (n == xs) sm_pv = mm;
                }
            }
        }
    }
    pr = wave_reduce_peak(pr);
    pp = wave_reduce_peak(pp);
    pm = wave_reduce_peak(pm);
    pa = wave_reduce_peak(pa);
    if ((t & 63) == 0) {
        sm_p[t >> 6][0] = pr.p; sm_i[t >> 6][0] = pr.idx;
        sm_p[t >> 6][1] = pp.p; sm_i[t >> 6][1] = pp.idx;
        sm_p[t >> 6][2] = pm.p; sm_i[t >> 6][2] = pm.idx;
        sm_p[t >> 6][3] = pa.p; sm_i[t >> 6][3] = pa.idx;
    }
    __syncthreads();
    if (t < 4) {
        Peak r = {sm_p[0][t], sm_i[0][t]};
#pragma unroll
        for (int x = 1; x < 4; ++x) r = peak_combine(r, Peak{sm_p[x][t], sm_i[x][t]});
        int* o = rec + ((size_t)row * G + j) * SE_VB_REC + 2 * t;
        o[0] = __float_as_int(r.p);
        o[1] = r.idx;
        if (t == 0) o[8] = __float_as_int(sm_pv);                   // mm(x*) in the workgroup that holds x*
    }
}

// grid (chunks, rows), block 256
__global__ __launch_bounds__(SE_VG_THREADS) void vb_fold_kernel(const float* __restrict__ prob, const int* __restrict__ rec,
                                                                const int* __restrict__ link_in, const int* __restrict__ complete_in,
                                                                const int* __restrict__ restarted_f, const int* __restrict__ index_f,
                                                                float* __restrict__ r_state, int* __restrict__ succ,
                                                                float* __restrict__ mm_out, int* __restrict__ link_out,
                                                                float* __restrict__ r_best, int* __restrict__ r_exponent,
                                                                float* __restrict__ mm_best, int* __restrict__ mm_peak,
                                                                float* __restrict__ path_value, float* __restrict__ alt_value,
                                                                int* __restrict__ alt_index, int* __restrict__ complete, int G,
                                                                int voxels) {
    __shared__ float fin_p[4];
    __shared__ int fin_i[4];
    const int t = threadIdx.x, row = blockIdx.y;
    if (t < 64) {
        Peak q[4] = {{0.f, INT_MAX}, {0.f, INT_MAX}, {0.f, INT_MAX}, {0.f, INT_MAX}};
        for (int x = t; x < G; x += 64) {
            const int* r = rec + ((size_t)row * G + x) * SE_VB_REC;
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = peak_combine(q[c], Peak{__int_as_float(r[2 * c]), r[2 * c + 1]});
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            q[c] = wave_reduce_peak(q[c]);
            if (t == 0) { fin_p[c] = q[c].p; fin_i[c] = q[c].idx; }
        }
    }
    __syncthreads();
    const bool linked = link_in != nullptr && link_in[row] >= 0;
    const bool death = linked && !(fin_p[0] > 0.f && fin_p[0] <= FLT_MAX);              // a NaN never became a maximum; +inf fails here
    if (blockIdx.x == 0 && t == 0) {
        const float nanf_ = __int_as_float(0x7fc00000);
        const float M = death ? fin_p[1] : fin_p[0];                // an unlinked row was written as r = p: both records agree
        const bool alive = M > 0.f && M <= FLT_MAX;
        const int e = alive ? ilogbf(M) : 0;
        const int pk = death ? fin_i[1] : fin_i[0];
        r_best[row] = alive ? ldexpf(M, -e) : nanf_;
        r_exponent[row] = e;
        link_out[row] = (alive && restarted_f[row] == 0) ? pk : -1; // a forward restart cuts the chain in both directions
        complete[row] = linked ? (death ? 0 : (complete_in[row] != 0 ? 1 : 0)) : 1;
        const int xs = index_f[row];
        const bool have = xs >= 0 && xs < voxels && !death;         // no path voxel, or no max-marginal to speak of
        const bool any = have && fin_p[2] > 0.f, other = have && fin_p[3] > 0.f;
        mm_best[row] = any ? fin_p[2] : nanf_;
        mm_peak[row] = any ? fin_i[2] : -1;
        path_value[row] = have ? __int_as_float(rec[((size_t)row * G + (xs / G) % G) * SE_VB_REC + 8]) : nanf_;
        alt_value[row] = other ? fin_p[3] : nanf_;
        alt_index[row] = other ? fin_i[3] : -1;
    }
    if (!death) return;
    const size_t base = (size_t)row * voxels;
    for (int n = blockIdx.x * SE_VG_THREADS + t; n < voxels; n += gridDim.x * SE_VG_THREADS) {
        r_state[base + n] = prob[base + n];                         // bit for bit
        if (succ != nullptr) succ[base + n] = -1;
        if (mm_out != nullptr) mm_out[base + n] = __int_as_float(0x7fc00000);
    }
}

// grid (chunks, rows), block 256: the r a call leaves behind is the scaled one, with the link, best and complete of the chunk's first frame
__global__ __launch_bounds__(SE_VG_THREADS) void vb_scale_kernel(float* __restrict__ r_state, const int* __restrict__ r_exponent,
                                                                 const int* __restrict__ link, const float* __restrict__ r_best,
                                                                 const int* __restrict__ complete, int* __restrict__ link_state,
                                                                 float* __restrict__ best_state, int* __restrict__ complete_state,
                                                                 int voxels) {
    const int t = threadIdx.x, row = blockIdx.y;
    const int down = -r_exponent[row];
    const size_t base = (size_t)row * voxels;
    for (int n = blockIdx.x * SE_VG_THREADS + t; n < voxels; n += gridDim.x * SE_VG_THREADS)
        r_state[base + n] = ldexpf(r_state[base + n], down);
    if (blockIdx.x == 0 && t == 0) { link_state[row] = link[row]; best_state[row] = r_best[row]; complete_state[row] = complete[row]; }
}

// grid (ceil(rows / 64)), block 64: one lane per row, sequential over the frames of a chunk.  direction -1 (chunks last first): from
// every anchor back through `back` to the segment's start; the cursor is the voxel the chunk's first frame points back to.  It writes
// every frame (-1 where no branch passes).  direction +1 (afterwards, chunks first to last): from every anchor on through `succ` to
// the segment's end; the cursor is the successor pointer, jump bit included, of the frame before the chunk.  It writes the frames it
// reaches and leaves the anchors' own.
__global__ __launch_bounds__(64) void vb_branch_kernel(const int* __restrict__ back, const int* __restrict__ succ,
                                                       const int* __restrict__ restarted, const int* __restrict__ anchor,
                                                       int* __restrict__ cursor, int* __restrict__ index, int* __restrict__ jumped,
                                                       int frames, int rows, int voxels, int direction, int have_carry) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    if (direction < 0) {
        int x = have_carry ? cursor[row] : -1;
        for (int f = frames - 1; f >= 0; --f) {
            const size_t fr = (size_t)f * rows + row;
            const int a = anchor[fr];
            if (a >= 0) x = a;
            if (x < 0 || x >= voxels) x = -1;                       // never an index outside the row
            const int b = (x >= 0 && restarted[fr] == 0) ? back[fr * voxels + x] : -1;
            index[fr] = x;
            jumped[fr] = (b >= 0 && (b & SE_VV_JUMP)) ? 1 : 0;
            x = b >= 0 ? (b & (SE_VV_JUMP - 1)) : -1;
        }
        cursor[row] = x;
    } else {
        int sp = have_carry ? cursor[row] : -1;
        for (int f = 0; f < frames; ++f) {
            const size_t fr = (size_t)f * rows + row;
            int x = sp >= 0 ? (sp & (SE_VV_JUMP - 1)) : -1;
            const int a = anchor[fr];
            if (a >= 0) x = a;
            if (x >= voxels) x = -1;
            if (a < 0 && x >= 0) { index[fr] = x; jumped[fr] = (sp & SE_VV_JUMP) ? 1 : 0; }
            sp = x >= 0 ? succ[fr * voxels + x] : -1;
        }
        cursor[row] = sp;
    }
}

// e2 [rows][voxels] float32, the records [rows][G][rec] words, then the k and the j offsets [rows][voxels] int8 each
long long vv_scratch_bytes(int rows, int G, int rec, long long more_words) {
    const long long bytes = (vg_elems(rows, G) + (long long)rows * G * rec + more_words) * 4 + 2 * vg_elems(rows, G);
    return (bytes + 15) & ~15LL;
}

// The forward pass of both entry points: the arguments gated, then three launches per frame and the scale pass.  KEEP = false is
// se_volume_viterbi_f32 as it has always been; KEEP = true (se_volume_viterbi_keep_f32) also fills scores_out.
template <bool KEEP>
int vv_forward(const float* prob, const float* taps, float* state, int* peak_state, float* best_state, int* back_out, int* peak,
               float* best, int* exponent, int* restarted, float* scores_out, void* scratch, long long scratch_bytes, int frames,
               int rows, int voxels, int G, int radius, float floor, const int* have_prior, void* stream) {
    if (!prob || !taps || !state || !peak_state || !best_state || !back_out || !peak || !best || !exponent || !restarted || !scratch)
        return SE_ERR_BAD_ARG;
    if (KEEP && !scores_out) return SE_ERR_BAD_ARG;
    if (!vg_args_ok(frames, rows, voxels, G, radius, floor)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, taps, state, peak_state, best_state, back_out, peak, best, exponent, restarted, scratch, have_prior,
                     scores_out}, 4))
        return SE_ERR_BAD_ARG;
    if (scratch_bytes < vv_scratch_bytes(rows, G, SE_VV_REC, 0)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    float* e2 = reinterpret_cast<float*>(scratch);
    int* rec = reinterpret_cast<int*>(e2 + vg_elems(rows, G));
    signed char* off_k = reinterpret_cast<signed char*>(rec + (long long)rows * G * SE_VV_REC);
    signed char* off_j = off_k + vg_elems(rows, G);
    const auto [wshift, chunks, keep, uniform] = vg_launch(voxels, G, floor);
    const int plane = G * G, padded = (G + 2 * radius) * G;                              // floats; the padded plane: R rows of zeros on either side
    const int stage_lds = (plane + padded) * 4, update_lds = (padded * 4 + plane + 15) & ~15;
    const int max_padded = (SE_VG_MAX_G + 2 * SE_VG_MAX_R) * SE_VG_MAX_G;
    SE_ENSURE_LDS(vv_stage_kj_kernel, (SE_VG_MAX_G * SE_VG_MAX_G + max_padded) * 4);        // 144 KB
    SE_ENSURE_LDS(vv_update_kernel<KEEP>, max_padded * 4 + SE_VG_MAX_G * SE_VG_MAX_G);    // 96 KB
    const size_t frame_elems = (size_t)rows * voxels;
    for (int f = 0; f < frames; ++f) {
        const float* p = prob + f * frame_elems;
        float* so = KEEP ? scores_out + f * frame_elems : nullptr;
        const int* peak_prev = f > 0 ? peak + (size_t)(f - 1) * rows : nullptr;
        const float* best_prev = f > 0 ? best + (size_t)(f - 1) * rows : nullptr;
        const int* exp_prev = f > 0 ? exponent + (size_t)(f - 1) * rows : nullptr;
        if (f > 0 || have_prior) {
            hipLaunchKernelGGL(vv_stage_kj_kernel, dim3(G, rows), dim3(SE_VG_THREADS), stage_lds, s, state, taps, have_prior,
                               peak_state, peak_prev, exp_prev, e2, off_k, off_j, G, voxels, radius, wshift);
            SE_CHECK_LAUNCH();
        }
        int* bo = back_out + f * frame_elems;
        hipLaunchKernelGGL(vv_update_kernel<KEEP>, dim3(G, rows), dim3(SE_VG_THREADS), update_lds, s, p, taps, have_prior, peak_state,
                           best_state, peak_prev, best_prev, e2, off_k, off_j, state, bo, rec, G, voxels, radius, wshift, keep, uniform,
                           so);
        SE_CHECK_LAUNCH();
        hipLaunchKernelGGL(vv_fold_kernel<KEEP>, dim3(chunks, rows), dim3(SE_VG_THREADS), 0, s, p, rec, have_prior, peak_state, peak_prev,
                           state, bo, peak + (size_t)f * rows, best + (size_t)f * rows, exponent + (size_t)f * rows,
                           restarted + (size_t)f * rows, G, voxels, so);
        SE_CHECK_LAUNCH();
    }
    const size_t last = (size_t)(frames - 1) * rows;
    hipLaunchKernelGGL(vv_scale_kernel, dim3(chunks, rows), dim3(SE_VG_THREADS), 0, s, state, exponent + last, peak + last, best + last,
                       peak_state, best_state, voxels);
    SE_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" long long se_volume_viterbi_scratch_bytes(int rows, int G, int radius) {
    return vg_shape_ok(rows, G, radius) ? vv_scratch_bytes(rows, G, SE_VV_REC, 0) : 0;
}

extern "C" int se_volume_viterbi_f32(const float* prob, const float* taps, float* state, int* peak_state, float* best_state,
                                     int* back_out, int* peak, float* best, int* exponent, int* restarted, void* scratch,
                                     long long scratch_bytes, int frames, int rows, int voxels, int G, int radius, float floor,
                                     const int* have_prior, void* stream) {
    return vv_forward<false>(prob, taps, state, peak_state, best_state, back_out, peak, best, exponent, restarted, nullptr, scratch,
                             scratch_bytes, frames, rows, voxels, G, radius, floor, have_prior, stream);
}

extern "C" int se_volume_viterbi_keep_f32(const float* prob, const float* taps, float* state, int* peak_state, float* best_state,
                                          int* back_out, int* peak, float* best, int* exponent, int* restarted, float* scores_out,
                                          void* scratch, long long scratch_bytes, int frames, int rows, int voxels, int G, int radius,
                                          float floor, const int* have_prior, void* stream) {
    return vv_forward<true>(prob, taps, state, peak_state, best_state, back_out, peak, best, exponent, restarted, scores_out, scratch,
                            scratch_bytes, frames, rows, voxels, G, radius, floor, have_prior, stream);
}

extern "C" long long se_volume_viterbi_back_scratch_bytes(int rows, int G, int radius) {
    return vg_shape_ok(rows, G, radius) ? vv_scratch_bytes(rows, G, SE_VB_REC, SE_VB_TAPS + 2LL * rows) : 0;
}

extern "C" int se_volume_viterbi_back_f32(const float* prob, const float* scores, const int* exponent,
                                          const int* restarted, const int* index, const float* taps, float* r_state, int* link_state,
                                          float* best_state, int* complete_state, float* mm_best, int* mm_peak, float* path_value,
                                          float* alt_value, int* alt_index, int* complete, float* r_best, int* r_exponent, int* succ,
                                          float* max_marginals, void* scratch, long long scratch_bytes, int frames, int rows,
                                          int voxels, int G, int radius, float floor, int separation, int have_next, void* stream) {
    if (!prob || !scores || !exponent || !restarted || !index || !taps || !r_state || !link_state || !best_state ||
        !complete_state || !mm_best || !mm_peak || !path_value || !alt_value || !alt_index || !complete || !r_best || !r_exponent ||
        !scratch)
        return SE_ERR_BAD_ARG;
    if (!vg_args_ok(frames, rows, voxels, G, radius, floor)) return SE_ERR_BAD_ARG;
    if (separation < 0 || (have_next != 0 && have_next != 1)) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, scores, exponent, restarted, index, taps, r_state, link_state, best_state, complete_state, mm_best,
                     mm_peak, path_value, alt_value, alt_index, complete, r_best, r_exponent, succ, max_marginals, scratch}, 4))
        return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_volume_viterbi_back_scratch_bytes(rows, G, radius)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    float* e2 = reinterpret_cast<float*>(scratch);
    int* rec = reinterpret_cast<int*>(e2 + vg_elems(rows, G));
    float* taps_rev = reinterpret_cast<float*>(rec + (long long)rows * G * SE_VB_REC);
    int* links = reinterpret_cast<int*>(taps_rev + SE_VB_TAPS);                         // two slots of [rows]
    signed char* off_k = reinterpret_cast<signed char*>(links + 2LL * rows);
    signed char* off_j = off_k + vg_elems(rows, G);
    const auto [wshift, chunks, keep, uniform] = vg_launch(voxels, G, floor);
    const int plane = G * G, padded = (G + 2 * radius) * G;
    const int stage_lds = (plane + padded) * 4, update_lds = (padded * 4 + plane + 15) & ~15;
    const int max_padded = (SE_VG_MAX_G + 2 * SE_VG_MAX_R) * SE_VG_MAX_G;
    SE_ENSURE_LDS(vv_stage_kj_kernel, (SE_VG_MAX_G * SE_VG_MAX_G + max_padded) * 4);        // 144 KB
    SE_ENSURE_LDS(vb_update_kernel, max_padded * 4 + SE_VG_MAX_G * SE_VG_MAX_G);          // 96 KB
    hipLaunchKernelGGL(vb_taps_kernel, dim3(1), dim3(64), 0, s, taps, taps_rev, radius);
    SE_CHECK_LAUNCH();
    const size_t frame_elems = (size_t)rows * voxels;
    // the link of frame f to frame f + 1 (the peak of r there, or -1) lies in slot (f + 2) & 1: the fold of frame f + 1 wrote it, the
    // fold of frame f reads it and writes the other slot.  The chunk's last frame reads the carried link_state instead.
    auto slot = [&](int f) { return links + (size_t)((f + 2) & 1) * rows; };
    for (int f = frames - 1; f >= 0; --f) {
        const bool last = f == frames - 1;
        const size_t fr = (size_t)f * rows;
        const int* link_in = last ? (have_next ? link_state : nullptr) : slot(f);
        const float* best_in = last ? best_state : r_best + fr + rows;
        const int* complete_in = last ? complete_state : complete + fr + rows;
        const int* exp_in = last ? nullptr : r_exponent + fr + rows;                    // the carried r arrives scaled
        const float* p = prob + f * frame_elems;
        int* su = succ ? succ + f * frame_elems : nullptr;
        float* mm = max_marginals ? max_marginals + f * frame_elems : nullptr;
        if (link_in) {
            hipLaunchKernelGGL(vv_stage_kj_kernel, dim3(G, rows), dim3(SE_VG_THREADS), stage_lds, s, r_state, taps_rev, nullptr, nullptr,
                               link_in, exp_in, e2, off_k, off_j, G, voxels, radius, wshift);
            SE_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(vb_update_kernel, dim3(G, rows), dim3(SE_VG_THREADS), update_lds, s, p, taps_rev, link_in, best_in,
                           scores + f * frame_elems, exponent + fr, index + fr, e2, off_k, off_j, r_state, su, mm, rec, G, voxels, radius,
                           wshift, keep, uniform, separation);
        SE_CHECK_LAUNCH();
        hipLaunchKernelGGL(vb_fold_kernel, dim3(chunks, rows), dim3(SE_VG_THREADS), 0, s, p, rec, link_in, complete_in, restarted + fr,
                           index + fr, r_state, su, mm, slot(f - 1), r_best + fr, r_exponent + fr, mm_best + fr, mm_peak + fr,
                           path_value + fr, alt_value + fr, alt_index + fr, complete + fr, G, voxels);
        SE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(vb_scale_kernel, dim3(chunks, rows), dim3(SE_VG_THREADS), 0, s, r_state, r_exponent, slot(-1), r_best, complete,
                       link_state, best_state, complete_state, voxels);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_volume_viterbi_branch_i32(const int* back, const int* succ, const int* restarted, const int* anchor, int* cursor,
                                            int* index, int* jumped, int frames, int rows, int voxels, int direction, int have_carry,
                                            void* stream) {
    if (!back || !succ || !restarted || !anchor || !cursor || !index || !jumped) return SE_ERR_BAD_ARG;
    if (frames < 1 || rows < 1 || rows > 65535 || voxels < 1 || voxels > SE_VG_MAX_G * SE_VG_MAX_G * SE_VG_MAX_G) return SE_ERR_BAD_ARG;
    if ((direction != -1 && direction != 1) || (have_carry != 0 && have_carry != 1)) return SE_ERR_BAD_ARG;
    if (!se_aligned({back, succ, restarted, anchor, cursor, index, jumped}, 4)) return SE_ERR_BAD_ARG;
    hipLaunchKernelGGL(vb_branch_kernel, dim3((rows + 63) / 64), dim3(64), 0, se_stream(stream), back, succ, restarted, anchor, cursor,
                       index, jumped, frames, rows, voxels, direction, have_carry);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_volume_viterbi_path_i32(const int* back, const int* peak, const int* restarted, int* cursor, int* index, int* jumped,
                                          int frames, int rows, int voxels, int have_next, void* stream) {
    if (!back || !peak || !restarted || !cursor || !index || !jumped) return SE_ERR_BAD_ARG;
    if (frames < 1 || rows < 1 || rows > 65535 || voxels < 1 || voxels > SE_VG_MAX_G * SE_VG_MAX_G * SE_VG_MAX_G) return SE_ERR_BAD_ARG;
    if (have_next != 0 && have_next != 1) return SE_ERR_BAD_ARG;
    if (!se_aligned({back, peak, restarted, cursor, index, jumped}, 4)) return SE_ERR_BAD_ARG;
    hipLaunchKernelGGL(vv_path_kernel, dim3((rows + 63) / 64), dim3(64), 0, se_stream(stream), back, peak, restarted, cursor, index,
                       jumped, frames, rows, voxels, have_next);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_volume_viterbi_refine_f32(const float* prob, const float* coord, const int* index, float* joints, int frames,
                                            int rows, int voxels, int G, int refine, void* stream) {
    if (!coord || !index || !joints || (!prob && refine > 0)) return SE_ERR_BAD_ARG;
    if (frames < 1 || rows < 1 || rows > 65535 || G < 2 || G > SE_VG_MAX_G) return SE_ERR_BAD_ARG;
    if ((long long)G * G * G != (long long)voxels || (long long)frames * rows > INT_MAX) return SE_ERR_BAD_ARG;
    if (refine < 0 || refine > SE_VV_MAX_REFINE) return SE_ERR_BAD_ARG;
    if (!se_aligned({prob, coord, index, joints}, 4)) return SE_ERR_BAD_ARG;
    const int total = frames * rows;
    hipLaunchKernelGGL(vv_refine_kernel, dim3((total + 63) / 64), dim3(64), 0, se_stream(stream), prob, coord, index, joints, total,
                       voxels, G, refine);
    SE_CHECK_LAUNCH();
    return 0;
}
