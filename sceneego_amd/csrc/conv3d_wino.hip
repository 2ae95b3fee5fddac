// 3x3x3 convolution with a 1-D Winograd F(4,3) transform along z, on the f32 MFMA, in "ping-pong" form: the kernel of the 3^3 shapes
// with cout % 32 == 0 and cin % 16 == 0 that the 2-D Winograd kernels do not take (dim % 16 == 8).  This file also holds the launcher
// that routes the 7^3 layer to its Winograd kernels (conv3d_wino67.hip, conv3d_wino47.hip).
//
// Structure: one persistent 512-thread workgroup per CU; a work unit is (32-cout block, 4x8x8 output tile); loop order cout block ->
// 16-channel chunk -> unit, so the 108 KB of transformed weights of a (block, chunk) (se_conv3d_pack_f32 section E) are loaded once
// per run of units.  For cin > 16 the per-chunk results are summed through the output tensor (read y-partial, add, write), prefetched
// one item ahead; residual add + ReLU happen on the last chunk.  The arithmetic and the two wave groups are described at the kernel.
#include "conv3d_plan.h"

#include <type_traits>
#include <utility>

namespace {

constexpr int HX = 10;   // halo columns of an 8-wide tile row

template <typename F, int... S>
__device__ __forceinline__ void for_each_index(F&& f, std::integer_sequence<int, S...>) {
    (f(std::integral_constant<int, S>{}), ...);
}

// global -> LDS copy of N4 16-byte pieces by NT threads, 8 loads in flight per thread (a plain loop is compiled to
// load / s_waitcnt vmcnt(0) / ds_write per iteration: one exposed L2 round trip per 16 bytes per thread).
template <int NT>
__device__ __forceinline__ void fill_lds(float* dst, const f32x4* __restrict__ src, int n4, int tid) {
    for (int base = 0; base < n4; base += NT * 8) {
        f32x4 t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + k * NT + tid;
            t[k] = src[i < n4 ? i : 0];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + k * NT + tid;
            if (i < n4) reinterpret_cast<f32x4*>(dst)[i] = t[k];
        }
    }
}

struct WinoIter {   // uniform walk over this workgroup's items: runs of units with equal cout block, chunk-outer
    int u_lo, n, cb, c, k;
    bool valid;
};

// ------------------------------------------------------------------------------------------------
// 3x3x3 convolution with 1-D Winograd F(4,3) along z: 6 multiplies per 4 z-neighbouring outputs instead of 12
// -> HALF the MFMAs of the direct form.  Lavin-Gray matrices, points {0, +-1, +-2, inf}:
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]          (G is folded into the packed weights)
// A 4x8x8 output tile is exactly one z quad; its 6 raw input slabs become 6 transformed slabs V_xi when the halo is
// committed to LDS (B^T applied once per element, as in the 7^3 kernel), so the inner loop is LDS reads + MFMAs only.
// fp32 error of the transform ~4e-7 mean / 5e-6 max per 3-tap dot product (tools/wino43_matrices.py).
//
// "Ping-pong" form (4-7 % faster in one-process A/B runs than a single-phase form in which all 8 waves share one whole V tile):
// the 8 waves form two groups of 4 (one wave per SIMD each) that work on the two y-halves (4 rows) of every 4x8x8 tile
// HALF A PHASE APART: while group A issues the 216 MFMAs of its half tile, group B runs everything else for its own
// half — A^T, partial-sum add, epilogue, output stores and the B^T transform + LDS commit of its next half tile — and in the
// next phase the roles swap.  One workgroup barrier per phase.  With all 8 waves doing these things at the same time the
// matrix pipe idles through every staging step (MFMA busy 62 % of the launch); here a SIMD always has one wave in its MFMA
// block.  In a group, wave wg: cout tile wg>>1, rows 2(wg&1), +1 of the half tile -> 6 accumulators (one per xi).  A lone
// MFMA wave per SIMD must not issue dependent MFMAs back to back (40-cycle latency vs 32-cycle issue), so two (tap, xi)
// sub-steps are interleaved on two different accumulators.
// LDS: 108 KB weights + 2 x 23 KB half V tiles (6 slabs x 6 rows x 10 columns x 16 channels) + unit table.
// ------------------------------------------------------------------------------------------------
constexpr int W43_FLOATS = SE_WINO43_CHUNK_FLOATS;
constexpr int PP_ROWS = 6;                                    // 4 rows + halo
constexpr int PP_COLS = PP_ROWS * HX;                         // 60 halo columns per half tile
constexpr int PP_VH_FLOATS = 6 * PP_COLS * 16;                // 5760 floats = 23040 B

#ifdef SE_STAMPPP
#define PP_T(var) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory"); __builtin_amdgcn_sched_barrier(0); }
#else
#define PP_T(var)
#endif

__global__ __launch_bounds__(512) void conv3d_k3_wino43pp_kernel(ConvArgs a, int tiles_per_dim, int ztiles, int total_tiles,
                                                                 int n_cb, int units_per_wg, int mode, unsigned long long* dbg) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    (void)mode;
    unsigned long long t_a = 0, t_b = 0, t_c = 0, acc_mfma = 0, acc_stage = 0, acc_bar = 0, acc_idle = 0, n_ph = 0;
    (void)t_a; (void)t_b; (void)t_c; (void)acc_mfma; (void)acc_stage; (void)acc_bar; (void)acc_idle; (void)n_ph; (void)dbg;
    float* wl = lds;
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    i32x4* utab = reinterpret_cast<i32x4*>(lds + W43_FLOATS + 2 * PP_VH_FLOATS);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int G = wave >> 2;                      // group: y half of the tile
    const int wg = wave & 3;
    const int vl = lane & 15;
    const int h = lane >> 4;
    const int dim = a.dim;
    const int chunks = a.cin >> 4;
    const int n_units = n_cb * total_tiles;
    const int u_begin = (int)blockIdx.x * units_per_wg;
    const int u_end = min(u_begin + units_per_wg, n_units);
    if (u_begin >= u_end) return;
    float* vt = lds + W43_FLOATS + G * PP_VH_FLOATS;

    for (int i = tid; i < u_end - u_begin; i += 512) {
        int t = (u_begin + i) % total_tiles;
        i32x4 e;
        e.w = t % tiles_per_dim; t /= tiles_per_dim;
        e.z = t % tiles_per_dim; t /= tiles_per_dim;
        e.y = t % ztiles; t /= ztiles;
        e.x = t;
        utab[i] = e;
    }

    // compute role inside the group: cout tile nt, rows 2*(wg&1), +1 of the half tile
    const int nt = wg >> 1;
    const int ry = (wg & 1) * 2 + (vl >> 3);
    const int rx = vl & 7;
    const float* vb = vt + (ry * HX + rx) * 16 + 4 * h;

    // staging role inside the group: thread tg < 240 owns halo column (tg >> 2) and channel quad (tg & 3)
    const int tg = tid & 255;
    const bool s_on = tg < PP_COLS * 4;
    const int s_col = tg >> 2, s_q = tg & 3;
    const int s_cy = s_col / HX, s_cx = s_col % HX;
    f32x4 raw[6];
    auto fetch = [&](int u, int c) {
        const i32x4 e = utab[u - u_begin];
        const int gy = e.z * 8 + G * 4 - 1 + s_cy, gx = e.w * 8 - 1 + s_cx, gz0 = e.y * 4 - 1;
        const bool okc = s_on && (unsigned)gy < (unsigned)dim && (unsigned)gx < (unsigned)dim;
        const long long base = ((((long long)e.x * dim) * dim + gy) * dim + gx) * a.cin_pad + c * 16 + s_q * 4;
        const long long zs = (long long)dim * dim * a.cin_pad;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const bool ok = okc && (unsigned)(gz0 + q) < (unsigned)dim;
            const f32x4 t = *reinterpret_cast<const f32x4*>(a.in + (ok ? base + (gz0 + q) * zs : 0));
            raw[q] = ok ? t : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    auto commit = [&]() {
        if (!s_on) return;
        const f32x4 d0 = raw[0], d1 = raw[1], d2 = raw[2], d3 = raw[3], d4 = raw[4], d5 = raw[5];
        f32x4 v[6];
        v[0] = 4.f * d0 - 5.f * d2 + d4;
        v[5] = 4.f * d1 - 5.f * d3 + d5;
        const f32x4 e1 = d4 - 4.f * d2, o1 = d3 - 4.f * d1;
        v[1] = e1 + o1;
        v[2] = e1 - o1;
        const f32x4 e2 = d4 - d2, o2 = 2.f * (d3 - d1);
        v[3] = e2 + o2;
        v[4] = e2 - o2;
#pragma unroll
        for (int x = 0; x < 6; ++x) *reinterpret_cast<f32x4*>(vt + (x * PP_COLS + s_col) * 16 + s_q * 4) = v[x];
    };
    auto load_weights = [&](int cb, int c) {
        fill_lds<512>(wl, reinterpret_cast<const f32x4*>(a.wpack_e) + ((size_t)c * n_cb + cb) * (W43_FLOATS / 4), W43_FLOATS / 4, tid);
    };
    auto out_offset = [&](int u, int cb) -> long long {
        const i32x4 e = utab[u - u_begin];
        return ((((long long)e.x * dim + e.y * 4) * dim + e.z * 8 + G * 4 + ry) * dim + e.w * 8 + rx) * a.cout + cb * 32 + nt * 16 + 4 * h;
    };
    const long long zstride = (long long)dim * dim * a.cout;
    const bool relu = a.flags & SE_EPI_RELU;
    const bool use_res = (a.flags & SE_EPI_RES_PRE_RELU) && a.res;

    auto first_item = [&]() {
        WinoIter it;
        it.u_lo = u_begin;
        it.cb = u_begin / total_tiles;
        it.n = min(u_end, (it.cb + 1) * total_tiles) - u_begin;
        it.c = 0; it.k = 0; it.valid = true;
        return it;
    };
    auto next_item = [&](WinoIter it) {
        if (++it.k == it.n) {
            it.k = 0;
            if (++it.c == chunks) {
                it.c = 0;
                it.u_lo += it.n;
                if (it.u_lo >= u_end) { it.valid = false; return it; }
                it.cb = it.u_lo / total_tiles;
                it.n = min(u_end, (it.cb + 1) * total_tiles) - it.u_lo;
            }
        }
        return it;
    };

    f32x4 acc[6], part[4], resv[4], bias = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int z = 0; z < 4; ++z) part[z] = resv[z] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int x = 0; x < 6; ++x) acc[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
    long long o0 = 0;
    const f32x4* wrow = reinterpret_cast<const f32x4*>(wl) + nt * 64 + lane;

    // epilogue operands of an item (running partial sums of earlier chunks, skip tensor, bias): issued early in its own MFMA
    // block, consumed one phase later (the previous chunk's stores of this half tile are at least two barriers old)
    auto load_operands = [&](const WinoIter& it) {
        o0 = out_offset(it.u_lo + it.k, it.cb);
        if (it.c > 0) {
#pragma unroll
            for (int z = 0; z < 4; ++z) part[z] = *reinterpret_cast<const f32x4*>(a.out + o0 + z * zstride);
        }
        if (it.c == chunks - 1) {
            bias = *reinterpret_cast<const f32x4*>(a.bpack + it.cb * 32 + nt * 16 + 4 * h);
            if (use_res) {
#pragma unroll
                for (int z = 0; z < 4; ++z) resv[z] = *reinterpret_cast<const f32x4*>(a.res + o0 + z * zstride);
            }
        }
    };

    __syncthreads();   // utab
    {
        const WinoIter it0 = first_item();
        fetch(it0.u_lo, 0);
        commit();
        load_weights(it0.cb, 0);
    }
    __syncthreads();

    int u_lo = u_begin;
    while (u_lo < u_end) {
        const int cb = u_lo / total_tiles;
        const int n = min(u_end, (cb + 1) * total_tiles) - u_lo;
        for (int c = 0; c < chunks; ++c) {
            const bool last_chunk = c == chunks - 1;
            const bool seg_next = c + 1 < chunks || u_lo + n < u_end;
            const int nc = c + 1 < chunks ? c + 1 : 0;
            // phases: group G issues the MFMAs of item j in phase 2j + G and finishes it (and stages what follows) in 2j + G + 1
            for (int t = 0; t <= 2 * n; ++t) {
                const int r = t - G;
                int kind = 0;
                PP_T(t_a)
                if (r >= 0 && !(r & 1) && (r >> 1) < n) {
                    kind = 1;
                    // ------------------------------ MFMA phase of item j: LDS reads and MFMAs only ------------------------------
                    __builtin_amdgcn_s_setprio(3);      // the partner wave on this SIMD is staging: its VALU must not delay MFMA issue
                    WinoIter mcur;
                    mcur.u_lo = u_lo; mcur.n = n; mcur.cb = cb; mcur.c = c; mcur.k = r >> 1; mcur.valid = true;
                    const WinoIter mnxt = next_item(mcur);
#pragma unroll
                    for (int x = 0; x < 6; ++x) acc[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    f32x4 w0 = wrow[0], v0 = *reinterpret_cast<const f32x4*>(vb);
                    f32x4 w1 = wrow[128], v1 = *reinterpret_cast<const f32x4*>(vb + PP_COLS * 16);
                    f32x4 w2 = w0, v2 = v0, w3 = w1, v3 = v1;
                    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                    auto pairstep = [&](auto p_tag) {
                        constexpr int P = decltype(p_tag)::value;
                        constexpr int S0 = 2 * P, S1 = 2 * P + 1;
                        constexpr int x0 = S0 % 6, x1 = S1 % 6;
                        // global loads ride inside the MFMA block (the MFMA wave has issue priority; in the staging phase, at
                        // low priority and behind the output stores, they measured 3 % slower overall)
                        if constexpr (P == 1) { if (mnxt.valid) fetch(mnxt.u_lo + mnxt.k, mnxt.c); }   // next half tile's columns
                        if constexpr (P == 4) load_operands(mcur);                                     // this item's epilogue operands
                        if constexpr (P + 1 < 27) {
                            constexpr int T2 = (S0 + 2) / 6, X2 = (S0 + 2) % 6, T3 = (S1 + 2) / 6, X3 = (S1 + 2) % 6;
                            w2 = wrow[(S0 + 2) * 128];
                            v2 = *reinterpret_cast<const f32x4*>(vb + (X2 * PP_COLS + (T2 / 3) * HX + (T2 % 3)) * 16);
                            w3 = wrow[(S1 + 2) * 128];
                            v3 = *reinterpret_cast<const f32x4*>(vb + (X3 * PP_COLS + (T3 / 3) * HX + (T3 % 3)) * 16);
                        }
                        acc[x0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, v0.x, acc[x0], 0, 0, 0);
                        acc[x1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, v1.x, acc[x1], 0, 0, 0);
                        acc[x0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, v0.y, acc[x0], 0, 0, 0);
                        acc[x1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, v1.y, acc[x1], 0, 0, 0);
                        acc[x0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, v0.z, acc[x0], 0, 0, 0);
                        acc[x1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, v1.z, acc[x1], 0, 0, 0);
                        acc[x0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, v0.w, acc[x0], 0, 0, 0);
                        acc[x1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, v1.w, acc[x1], 0, 0, 0);
                        if constexpr (P + 1 < 27) {
                            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                        } else {
                            __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                        }
                        w0 = w2; v0 = v2; w1 = w3; v1 = v3;
                    };
                    for_each_index(pairstep, std::make_integer_sequence<int, 27>{});
                    __builtin_amdgcn_s_setprio(0);
                } else if (r >= 1 && (r & 1) && ((r - 1) >> 1) < n) {
                    kind = 2;
                    // ------------------------------ finish item j, stage what follows ------------------------------
                    WinoIter cur;
                    cur.u_lo = u_lo; cur.n = n; cur.cb = cb; cur.c = c; cur.k = (r - 1) >> 1; cur.valid = true;
                    const WinoIter nxt = next_item(cur);
                    f32x4 y[4];
                    {
                        const f32x4 s12 = acc[1] + acc[2], d12 = acc[1] - acc[2], s34 = acc[3] + acc[4], d34 = acc[3] - acc[4];
                        y[0] = acc[0] + s12 + s34;
                        y[1] = d12 + 2.f * d34;
                        y[2] = s12 + 4.f * s34;
                        y[3] = d12 + 8.f * d34 + acc[5];
                    }
                    if (c > 0) {
#pragma unroll
                        for (int z = 0; z < 4; ++z) y[z] += part[z];
                    }
                    if (nxt.valid) commit();         // this group's V half tile is free: its MFMA block ended before the barrier
                    if (last_chunk) {
#pragma unroll
                        for (int z = 0; z < 4; ++z) {
                            y[z] += bias;
                            if (use_res) y[z] += resv[z];
                            if (relu) {
                                y[z].x = fmaxf(y[z].x, 0.f); y[z].y = fmaxf(y[z].y, 0.f);
                                y[z].z = fmaxf(y[z].z, 0.f); y[z].w = fmaxf(y[z].w, 0.f);
                            }
                        }
                    }
#pragma unroll
                    for (int z = 0; z < 4; ++z) *reinterpret_cast<f32x4*>(a.out + o0 + z * zstride) = y[z];
                }
                PP_T(t_b)
                __syncthreads();
                PP_T(t_c)
#ifdef SE_STAMPPP
                if (kind == 1) acc_mfma += t_b - t_a; else if (kind == 2) acc_stage += t_b - t_a; else acc_idle += t_b - t_a;
                acc_bar += t_c - t_b;
                ++n_ph;
#endif
                (void)kind;
            }
            if (seg_next) {
                load_weights(c + 1 < chunks ? cb : (u_lo + n) / total_tiles, nc);
                __syncthreads();
            }
        }
        u_lo += n;
    }
#ifdef SE_STAMPPP
    if (lane == 0 && dbg) {
        unsigned long long* o = dbg + ((size_t)blockIdx.x * 8 + wave) * 6;
        o[0] = acc_mfma; o[1] = acc_stage; o[2] = acc_bar; o[3] = acc_idle; o[4] = n_ph; o[5] = 0;
    }
#endif
}

unsigned long long* g_wino_dbg43 = nullptr;   // se_debug_set_stamp_buffer: read by the stamp builds (SE_STAMPPP / SE_STAMP47 / SE_STAMP67)

constexpr int LDS43 = 160 * 1024;

// work units of one launch per persistent workgroup (min(units, CUs) workgroups)
int per_wg(int n_units, int num_cus) {
    const int grid = n_units < num_cus ? n_units : num_cus;
    return (n_units + grid - 1) / grid;
}

}  // namespace

// The unit table (16 B per unit in the LDS left beside weights and tiles) of `kernel` holds a launch of `batch` samples.
bool se_conv3d_wino1d_fits(int kernel, int batch, int dim, int cout, int num_cus) {
    if (kernel != SE_CONV_WINO43PP_1D) return false;
    const int total_tiles = batch * (dim / 4) * (dim / 8) * (dim / 8);   // 4 x 8 x 8 output tiles
    const int n_units = (cout / 32) * total_tiles;                       // a unit is (tile, 32-cout block)
    const int fixed_floats = W43_FLOATS + 2 * PP_VH_FLOATS;              // LDS floats beside the table
    return n_units > 0 && per_wg(n_units, num_cus) <= (LDS43 - fixed_floats * 4) / 16;
}

// The 1-D Winograd 3^3 kernel: ping-pong F(4,3) (shapes the 2-D kernels do not take, e.g. dim % 16 != 0).
// Preconditions (se_conv3d_plan): se_wino1d_shape_ok, cin_pad == cin, channels-last tensors, no SE_EPI_RES_POST_RELU /
// SE_EPI_OUT_PLANAR, section E present, se_conv3d_wino1d_fits.
int se_conv3d_wino1d_launch(const ConvArgs& a, int batch, int kernel, hipStream_t s) {
    if (kernel != SE_CONV_WINO43PP_1D) return SE_ERR_BAD_ARG;
    const int tiles = a.dim / 8, ztiles = a.dim / 4;
    const int total_tiles = batch * ztiles * tiles * tiles;
    const int n_cb = a.cout / 32;
    const int n_units = n_cb * total_tiles;
    const int per = per_wg(n_units, se_num_cus());
    const dim3 grid((n_units + per - 1) / per);
    SE_ENSURE_LDS(conv3d_k3_wino43pp_kernel, LDS43);
    hipLaunchKernelGGL(conv3d_k3_wino43pp_kernel, grid, dim3(512), LDS43, s, a, tiles, ztiles, total_tiles, n_cb, per, 0, g_wino_dbg43);
    SE_CHECK_LAUNCH();
    return 0;
}

#ifdef SE_DEVTOOLS
// Debug only: device buffer (u64 [workgroups][8 waves][6]; F(6,7): [8]) that the stamp builds of the kernels launched from this file
// fill with their cycle sums.  A build without one of those flags never reads it.
extern "C" void se_debug_set_stamp_buffer(void* p) { g_wino_dbg43 = reinterpret_cast<unsigned long long*>(p); }
#endif

// The Winograd 7^3 kernels: F(6,7) (conv3d_wino67.hip), F(4,7) per input layout (conv3d_wino47.hip).
// Preconditions (se_conv3d_plan): se_k7_wino_shape_ok, no residual, channels-last output, section F (F(6,7): H) present, the
// kernel's _fits.
int se_conv3d_k7_wino_launch(const ConvArgs& a, int batch, int kernel, hipStream_t s) {
    const int num_cus = se_num_cus();
    switch (kernel) {
        case SE_CONV_K7_WINO67: return se_conv3d_k7_wino67_launch(a, batch, num_cus, s, g_wino_dbg43);
        case SE_CONV_K7_WINO47_P3: return se_conv3d_k7_wino47_launch_p3(a, batch, num_cus, s, g_wino_dbg43);
        case SE_CONV_K7_WINO47_CL: return se_conv3d_k7_wino47_launch_cl(a, batch, num_cus, s, g_wino_dbg43);
        default: return SE_ERR_BAD_ARG;
    }
}
