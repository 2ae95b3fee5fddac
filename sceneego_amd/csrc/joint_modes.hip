// Multi-hypothesis joints: the K strongest local maxima (modes) of every softmaxed joint volume, each with the mass and the
// first moments of its neighbourhood (sceneego_amd/op.py: joint_modes; VoxelNetwork_depth.joint_modes drives it).  No counterpart in
// the reference.  include/sceneego_hip.h states the definition; tests/joint_modes_model.py restates it and the result is compared
// bit for bit.
//
// A voxel is a mode iff its key (p, -n) is greater than the key of each of its up to 26 neighbours.  With the neighbours split by
// flat index that is two float comparisons and no index arithmetic:
//     p > max(p of the 13 neighbours with a LOWER index)    (an equal neighbour of lower index has the greater key)
//     p >= max(p of the 13 neighbours with a HIGHER index)
// The lower neighbours are plane i-1 (9), row j-1 of plane i (3) and k-1; the higher ones k+1, row j+1 (3) and plane i+1 (9).  The
// 3-wide maximum along k of a row (R3) and the 3x3 maximum of a plane (P9 = max of three R3) are shared between the planes.
//
// Two launches:
//   joint_modes_tile_kernel<S>  grid (tiles, rows), block 256.  A tile is S i-planes x TJ j-rows x all k; it is staged in LDS with a
//                               halo of one plane and one row (from L2: the neighbouring tile reads them from HBM), every row padded
//                               by a quad of -inf on both sides, and everything outside the grid is -inf as well: a neighbour that
//                               does not exist never wins, and nothing wraps from one row of the grid into the next.  Thread
//                               (quad q, row j) owns the 4 k x S i voxels [4q, 4q+4) of row j: per staged plane three 16-byte LDS
//                               reads and six 4-byte ones.  Its mode flags (4 S bits) go to a private LDS word.  The workgroup then
//                               takes its K greatest mode keys by K rounds of a workgroup key-argmax over per-lane running bests
//                               (only the lane that won a round rescans its own voxels for its next best) and writes them, its
//                               mode count and its NaN flag as one record of 2 + 2K words into scratch.
//   joint_modes_merge_kernel    one wave per row: sums the counts, ORs the NaN flags, selects the K greatest keys of the row's records
//                               (round r takes the greatest key below the winner of round r-1: keys are unique), then lane r walks
//                               the window of mode r serially: float64 sums in ascending flat index, one rounding each.
// No atomics; every result is either an exact integer, a selection under a total order or a sum in a fixed order: bitwise identical
// from run to run.  No division of floats anywhere.
#include "row_reduce.h"   // Peak, peak_combine, wave_reduce_peak

#pragma clang fp contract(off)

#define SE_JM_THREADS 256
#define SE_JM_BATCH 8               // staged rows a thread loads before it stores the first
#define SE_JM_MAX_K 16
#define SE_JM_MAX_RADIUS 3
#define SE_JM_MAX_G 1290            // 1290^3 < 2^31 <= 1291^3
#define SE_JM_LDS_BUDGET (65536 - 256)   // dynamic LDS per workgroup, the small static arrays left out

namespace {

// key(a) < key(b) under the order (p, -n)
__device__ __forceinline__ bool key_less(Peak a, Peak b) { return a.p < b.p || (a.p == b.p && a.idx > b.idx); }
__device__ __forceinline__ int wave_reduce_add_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int wave_reduce_or_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}

// How a [G][G][G] volume is cut into tiles; a function of G alone (the scratch size and both kernels follow from it).
struct Tiling {
    int S;        // i-planes per tile (4, or 2 where 6 staged planes do not fit)
    int TJ;       // j-rows per tile: one row per group of QRp threads
    int QR;       // quads per row, ceil(G / 4)
    int qshift;   // QRp = 1 << qshift = min(256, the power of two >= QR) threads work side by side on one row
    int nslab, nband;
    int lds_bytes;
    bool ok;
};
inline Tiling jm_tiling(int G) {
    Tiling t = {};
    if (G < 2 || G > SE_JM_MAX_G) return t;
    t.QR = (G + 3) / 4;
    int p2 = 1;
    while (p2 < t.QR && p2 < SE_JM_THREADS) { p2 <<= 1; ++t.qshift; }
    const int rpb = SE_JM_THREADS / p2;
    t.TJ = G < rpb ? G : rpb;
    const int RS = 4 * t.QR + 8;
    for (t.S = 4; t.S >= 2; t.S -= 2) {
        const long long b = ((long long)(t.S + 2) * (t.TJ + 2) * RS + (long long)t.TJ * t.QR) * 4;
        if (b <= SE_JM_LDS_BUDGET) { t.lds_bytes = (int)b; t.ok = true; break; }
    }
    if (!t.ok) return t;
    t.nslab = (G + t.S - 1) / t.S;
    t.nband = (G + t.TJ - 1) / t.TJ;
    return t;
}

// grid (nslab * nband, rows), block 256, dynamic LDS: (S + 2)(TJ + 2) rows of RS = 4 QR + 8 floats, then TJ * QR flag words
template <int S>
__global__ __launch_bounds__(SE_JM_THREADS) void joint_modes_tile_kernel(const float* __restrict__ prob, int* __restrict__ scratch,
                                                                         int G, int voxels, int K, float min_prob, int TJ, int QR,
                                                                         int qshift, int nband, float inv_tj2) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float sm_p[2][4];
    __shared__ int sm_i[2][4];
    __shared__ int sm_cnt[4];
    __shared__ int sm_nan[4];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int row = blockIdx.y, tile = blockIdx.x;
    const int slab = tile / nband, band = tile - slab * nband;
    const int i0 = slab * S, j0 = band * TJ;
    const int RS = 4 * QR + 8, TJ2 = TJ + 2, nrows = (S + 2) * TJ2;
    const int QRp = 1 << qshift, q0 = t & (QRp - 1), rsub = t >> qshift, RPB = SE_JM_THREADS >> qshift;
    const float* v = prob + (size_t)row * voxels;
    const float NINF = -INFINITY;
    const f32x4 ninf4 = {NINF, NINF, NINF, NINF};
    const bool g4 = (G & 3) == 0;

    // the pad quads left and right of every staged row
    for (int x = t; x < nrows * 2; x += SE_JM_THREADS)
        *reinterpret_cast<f32x4*>(lds + (x >> 1) * RS + ((x & 1) ? 4 + 4 * QR : 0)) = ninf4;
    // the staged rows: row pr = pi * (TJ + 2) + rj holds plane i0 - 1 + pi, row j0 - 1 + rj, or -inf where that is outside the grid
    // SE_JM_BATCH rows per thread at a time: all their loads are issued before the first LDS store waits for one (a load that is
    // stored at once costs a memory round trip per row).  That path is for G a multiple of 4 and is branch-free: a row outside the
    // grid (or past the last staged row) loads the start of the volume instead and is replaced by -inf afterwards.
    for (int q = q0; q < QR; q += QRp) {
        const int k = 4 * q;
        if (g4) {
            for (int prb = rsub; prb < nrows; prb += SE_JM_BATCH * RPB) {
                f32x4 buf[SE_JM_BATCH];
                unsigned inside = 0;
#pragma unroll
                for (int u = 0; u < SE_JM_BATCH; ++u) {
                    const int pr = min(prb + u * RPB, nrows - 1);
                    const int pi = (int)(((float)pr + 0.5f) * inv_tj2);   // exact: pr < 2^12, the quotient >= 1 / (2 TJ2) off an integer
                    const int rj = pr - pi * TJ2;
                    const int i = i0 - 1 + pi, j = j0 - 1 + rj;
                    const bool in = i >= 0 && i < G && j >= 0 && j < G;
                    inside |= (in ? 1u : 0u) << u;
                    buf[u] = *reinterpret_cast<const f32x4*>(v + (in ? ((size_t)i * G + j) * G : 0) + k);   // 16-byte aligned
                }
#pragma unroll
                for (int u = 0; u < SE_JM_BATCH; ++u) {
                    const int pr = prb + u * RPB;
                    if (pr < nrows) *reinterpret_cast<f32x4*>(lds + pr * RS + 4 + k) = ((inside >> u) & 1u) ? buf[u] : ninf4;
                }
            }
        } else {
            for (int pr = rsub; pr < nrows; pr += RPB) {
                const int pi = (int)(((float)pr + 0.5f) * inv_tj2);
                const int rj = pr - pi * TJ2;
                const int i = i0 - 1 + pi, j = j0 - 1 + rj;
                f32x4 x = ninf4;
                if (i >= 0 && i < G && j >= 0 && j < G) {
                    const size_t base = ((size_t)i * G + j) * G;
                    if (k < G) x.x = v[base + k];
                    if (k + 1 < G) x.y = v[base + k + 1];
                    if (k + 2 < G) x.z = v[base + k + 2];
                    if (k + 3 < G) x.w = v[base + k + 3];
                }
                *reinterpret_cast<f32x4*>(lds + pr * RS + 4 + k) = x;
            }
        }
    }
    __syncthreads();

    int* flags = reinterpret_cast<int*>(lds + nrows * RS);
    Peak best = {NINF, INT_MAX};
    int cnt = 0;
    bool nan = false;
    const int jl = rsub;                         // the tile row this thread owns (when jl < TJ)
    const bool owner = jl < TJ && j0 + jl < G;
    if (owner) {
        for (int q = q0; q < QR; q += QRp) {
            float P9[S + 2][4], LO[S + 2][4], HI[S + 2][4], own[S + 2][4];
#pragma unroll
            for (int pi = 0; pi < S + 2; ++pi) {
                float R3[3][4], c[6];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float* r = lds + (pi * TJ2 + jl + d) * RS + 4 + 4 * q;
                    const f32x4 x = *reinterpret_cast<const f32x4*>(r);
                    const float w[6] = {r[-1], x.x, x.y, x.z, x.w, r[4]};
#pragma unroll
                    for (int e = 0; e < 4; ++e) R3[d][e] = fmaxf(fmaxf(w[e], w[e + 1]), w[e + 2]);
                    if (d == 1) {
#pragma unroll
                        for (int e = 0; e < 6; ++e) c[e] = w[e];
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    P9[pi][e] = fmaxf(fmaxf(R3[0][e], R3[1][e]), R3[2][e]);
                    LO[pi][e] = fmaxf(R3[0][e], c[e]);           // row j-1 and k-1
                    HI[pi][e] = fmaxf(c[e + 2], R3[2][e]);       // k+1 and row j+1
                    own[pi][e] = c[e + 1];
                }
            }
            unsigned mask = 0;
#pragma unroll
            for (int s = 0; s < S; ++s) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = own[s + 1][e];               // -inf outside the grid: neither a NaN nor a mode
                    const float lo = fmaxf(P9[s][e], LO[s + 1][e]);
                    const float hi = fmaxf(HI[s + 1][e], P9[s + 2][e]);
                    nan |= p != p;
                    if (p > 0.f && p >= min_prob && p > lo && p >= hi) {
                        mask |= 1u << (s * 4 + e);
                        best = peak_combine(best, Peak{p, ((i0 + s) * G + j0 + jl) * G + 4 * q + e});
                    }
                }
            }
            flags[jl * QR + q] = (int)mask;     // read back by this thread alone
            cnt += __popc(mask);
        }
    }
    cnt = wave_reduce_add_int(cnt);
    const int wnan = wave_reduce_or_int(nan ? 1 : 0);
    if (lane == 0) { sm_cnt[wid] = cnt; sm_nan[wid] = wnan; }

    const int ntiles = gridDim.x;
    int* rec = scratch + ((size_t)row * ntiles + tile) * (2 + 2 * K);
    int r = 0;
    for (; r < K; ++r) {
        const Peak w = wave_reduce_peak(best);
        if (lane == 0) { sm_p[r & 1][wid] = w.p; sm_i[r & 1][wid] = w.idx; }
        __syncthreads();                         // the buffer of round r is rewritten in round r + 2, behind the barrier of r + 1
        Peak g = {sm_p[r & 1][0], sm_i[r & 1][0]};
#pragma unroll
        for (int k = 1; k < 4; ++k) g = peak_combine(g, Peak{sm_p[r & 1][k], sm_i[r & 1][k]});
        if (g.idx == INT_MAX) break;             // uniform: no mode left in the tile
        if (t == 0) { rec[2 + 2 * r] = __float_as_int(g.p); rec[3 + 2 * r] = g.idx; }
        if (best.idx == g.idx) {                 // the winner's lane: its greatest key below the winner
            Peak nb = {NINF, INT_MAX};
            for (int q = q0; q < QR; q += QRp) {
                const unsigned mask = (unsigned)flags[jl * QR + q];
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (!((mask >> (s * 4)) & 15u)) continue;
                    const float* c = lds + ((s + 1) * TJ2 + jl + 1) * RS + 4 + 4 * q;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const Peak cand = {c[e], ((i0 + s) * G + j0 + jl) * G + 4 * q + e};
                        if (((mask >> (s * 4 + e)) & 1u) && key_less(cand, g)) nb = peak_combine(nb, cand);
                    }
                }
            }
            best = nb;
        }
    }
    if (t == 0) {
        for (; r < K; ++r) { rec[2 + 2 * r] = __float_as_int(NINF); rec[3 + 2 * r] = INT_MAX; }
        rec[0] = (sm_cnt[0] + sm_cnt[1]) + (sm_cnt[2] + sm_cnt[3]);   // K >= 1: the barrier of round 0 lies behind the writes
        rec[1] = (sm_nan[0] | sm_nan[1]) | (sm_nan[2] | sm_nan[3]);
    }
}

// grid (rows), block 64: one wave per row
__global__ __launch_bounds__(64) void joint_modes_merge_kernel(const float* __restrict__ prob, const float* __restrict__ coord,
                                                               const int* __restrict__ scratch, float* __restrict__ modes,
                                                               int* __restrict__ index, int* __restrict__ count,
                                                               int* __restrict__ total, int G, int voxels, int K, int radius,
                                                               int ntiles) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int stride = 2 + 2 * K;
    const int* base = scratch + (size_t)row * ntiles * stride;
    int tot = 0, nan = 0;
    for (int tile = lane; tile < ntiles; tile += 64) {
        tot += base[(size_t)tile * stride];
        nan |= base[(size_t)tile * stride + 1];
    }
    tot = wave_reduce_add_int(tot);
    nan = wave_reduce_or_int(nan);

    Peak prev = {INFINITY, -1};                 // above every key
    Peak mine = {-INFINITY, INT_MAX};
    const int nent = ntiles * K;
    for (int r = 0; r < K; ++r) {
        Peak b = {-INFINITY, INT_MAX};
        for (int e = lane; e < nent; e += 64) {
            const int tile = e / K, slot = e - tile * K;
            const int* p = base + (size_t)tile * stride + 2 + 2 * slot;
            const Peak c = {__int_as_float(p[0]), p[1]};
            if (c.idx != INT_MAX && key_less(c, prev)) b = peak_combine(b, c);
        }
        b = wave_reduce_peak(b);
        if (b.idx == INT_MAX) break;            // uniform
        if (lane == r) mine = b;
        prev = b;
    }

    if (lane >= K) return;
    float* o = modes + ((size_t)row * K + lane) * 8;
    const float q = __int_as_float(0x7fc00000);
    if (nan) {                                  // a NaN probability somewhere in the row
#pragma unroll
        for (int a = 0; a < 8; ++a) o[a] = q;
        index[(size_t)row * K + lane] = -1;
        if (lane == 0) { count[row] = -1; total[row] = -1; }
        return;
    }
    if (lane == 0) { count[row] = tot < K ? tot : K; total[row] = tot; }
    if (mine.idx == INT_MAX) {                  // unfilled record
        o[0] = o[1] = o[2] = o[3] = o[4] = 0.f;
        o[5] = o[6] = o[7] = q;
        index[(size_t)row * K + lane] = -1;
        return;
    }
    const int ci = mine.idx / (G * G), cj = (mine.idx / G) % G, ck = mine.idx % G;
    const int ia = max(ci - radius, 0), ib = min(ci + radius, G - 1);
    const int ja = max(cj - radius, 0), jb = min(cj + radius, G - 1);
    const int ka = max(ck - radius, 0), kb = min(ck + radius, G - 1);
    const float* v = prob + (size_t)row * voxels;
    double m = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    for (int i = ia; i <= ib; ++i)
        for (int j = ja; j <= jb; ++j)
            for (int k = ka; k <= kb; ++k) {    // ascending flat index
                const size_t n = ((size_t)i * G + j) * G + k;
                const double p = (double)v[n];
                m += p;
                mx += p * (double)coord[n * 3 + 0];   // exact products: 24 x 24 bits
                my += p * (double)coord[n * 3 + 1];
                mz += p * (double)coord[n * 3 + 2];
            }
    o[0] = mine.p;
    o[1] = (float)m;
    o[2] = (float)mx;
    o[3] = (float)my;
    o[4] = (float)mz;
    o[5] = coord[(size_t)mine.idx * 3 + 0];
    o[6] = coord[(size_t)mine.idx * 3 + 1];
    o[7] = coord[(size_t)mine.idx * 3 + 2];
    index[(size_t)row * K + lane] = mine.idx;
}

}  // namespace

extern "C" long long se_joint_modes_scratch_bytes(int rows, int G, int K) {
    if (rows <= 0 || K < 1 || K > SE_JM_MAX_K) return 0;
    const Tiling t = jm_tiling(G);
    if (!t.ok) return 0;
    return (long long)rows * t.nslab * t.nband * (2 + 2 * K) * 4;
}

extern "C" int se_joint_modes_f32(const float* prob, const float* coord, float* modes, int* index, int* count, int* total,
                                  void* scratch, long long scratch_bytes, int rows, int voxels, int G, int K, int radius,
                                  float min_prob, void* stream) {
    if (!prob || !coord || !modes || !index || !count || !total || !scratch) return SE_ERR_BAD_ARG;
    if (rows <= 0 || rows > 65535 || G < 2 || G > SE_JM_MAX_G) return SE_ERR_BAD_ARG;
    if ((long long)G * G * G != (long long)voxels || (voxels & 3)) return SE_ERR_BAD_ARG;
    if (K < 1 || K > SE_JM_MAX_K || radius < 0 || radius > SE_JM_MAX_RADIUS) return SE_ERR_BAD_ARG;
    if (!(min_prob >= 0.f)) return SE_ERR_BAD_ARG;                                       // a NaN fails
    // the 16-byte loads of the staging pass; the scratch records are 32-bit words
    if ((reinterpret_cast<uintptr_t>(prob) & 15) || (reinterpret_cast<uintptr_t>(coord) & 15)) return SE_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(scratch) & 3) return SE_ERR_BAD_ARG;
    const Tiling t = jm_tiling(G);
    if (!t.ok) return SE_ERR_BAD_ARG;
    if (scratch_bytes < se_joint_modes_scratch_bytes(rows, G, K)) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    const int ntiles = t.nslab * t.nband;
    const float inv_tj2 = 1.0f / (float)(t.TJ + 2);
    int* rec = reinterpret_cast<int*>(scratch);
    if (t.S == 4)
        hipLaunchKernelGGL(joint_modes_tile_kernel<4>, dim3(ntiles, rows), dim3(SE_JM_THREADS), t.lds_bytes, s, prob, rec, G, voxels,
                           K, min_prob, t.TJ, t.QR, t.qshift, t.nband, inv_tj2);
    else
        hipLaunchKernelGGL(joint_modes_tile_kernel<2>, dim3(ntiles, rows), dim3(SE_JM_THREADS), t.lds_bytes, s, prob, rec, G, voxels,
                           K, min_prob, t.TJ, t.QR, t.qshift, t.nband, inv_tj2);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(joint_modes_merge_kernel, dim3(rows), dim3(64), 0, s, prob, coord, rec, modes, index, count, total, G, voxels,
                       K, radius, ntiles);
    SE_CHECK_LAUNCH();
    return 0;
}
