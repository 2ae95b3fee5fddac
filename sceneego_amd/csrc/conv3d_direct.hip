// The float32 kernels that read their activations straight from global memory / L2 (channels-last [B][Z][Y][X][C], operand maps:
// conv3d.hip): the generic "direct" kernel (any k in {1,3,7}, any volume size, batch flattened into the voxel axis - the
// always-available path of the plan), ConvTranspose3d k2s2, and the two max-pools.
#include "common.h"

#include "conv3d_plan.h"

namespace {

// ------------------------------------------------------------------------------------------------
// direct implicit-GEMM kernel
// ------------------------------------------------------------------------------------------------
template <int KS, int M_T, int N_T, bool DECONV>
__global__ __launch_bounds__(256) void conv3d_direct_kernel(ConvArgs a) {
    constexpr int P = (KS - 1) / 2;
    constexpr int TAPS = KS * KS * KS;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vl = lane & 15;   // voxel within the 16-voxel tile / cout within the weight tile
    const int h = lane >> 4;    // k group
    const int dim = a.dim;
    const int cgs = (a.cin + 15) >> 4;   // channel groups that hold real channels
    const int nt0 = blockIdx.y * N_T;
    const int sub = DECONV ? blockIdx.z : 0;  // (a,b,c) sub-position of the 2x2x2 transposed kernel

    // voxel coordinates of this lane's column in each of the wave's M_T tiles
    const long long v_base = ((long long)blockIdx.x * 4 + wave) * (M_T * 16);
    int vb[M_T], vz[M_T], vy[M_T], vx[M_T];
    bool vok[M_T];
#pragma unroll
    for (int m = 0; m < M_T; ++m) {
        const long long vid = v_base + m * 16 + vl;
        vok[m] = vid < a.total_vox;
        long long t = vok[m] ? vid : 0;
        vx[m] = (int)(t % dim); t /= dim;
        vy[m] = (int)(t % dim); t /= dim;
        vz[m] = (int)(t % dim); t /= dim;
        vb[m] = (int)t;
    }

    f32x4 acc[M_T][N_T];
#pragma unroll
    for (int m = 0; m < M_T; ++m)
#pragma unroll
        for (int n = 0; n < N_T; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const f32x4* wp = reinterpret_cast<const f32x4*>(a.wpack);
    for (int tap = 0; tap < (DECONV ? 1 : TAPS); ++tap) {
        const int dz = tap / (KS * KS) - P;
        const int dy = (tap / KS) % KS - P;
        const int dx = tap % KS - P;
        const float* src[M_T];
        bool ok[M_T];
#pragma unroll
        for (int m = 0; m < M_T; ++m) {
            const int zz = vz[m] + dz, yy = vy[m] + dy, xx = vx[m] + dx;
            ok[m] = vok[m] && (unsigned)zz < (unsigned)dim && (unsigned)yy < (unsigned)dim && (unsigned)xx < (unsigned)dim;
            const long long off = ((((long long)vb[m] * dim + zz) * dim + yy) * dim + xx) * a.cin_pad + 4 * h;
            src[m] = a.in + (ok[m] ? off : 0);
        }
        const int wtap = DECONV ? sub : tap;
        for (int cg = 0; cg < cgs; ++cg) {
            f32x4 xf[M_T];
#pragma unroll
            for (int m = 0; m < M_T; ++m) {
                xf[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (ok[m]) xf[m] = *reinterpret_cast<const f32x4*>(src[m] + cg * 16);
            }
            const f32x4* wrow = wp + ((size_t)(cg * (DECONV ? 8 : TAPS) + wtap) * a.nts + nt0) * 64 + lane;
#pragma unroll
            for (int n = 0; n < N_T; ++n) {
                const f32x4 wf = wrow[n * 64];
#pragma unroll
                for (int m = 0; m < M_T; ++m) {
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.x, xf[m].x, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.y, xf[m].y, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.z, xf[m].z, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.w, xf[m].w, acc[m][n], 0, 0, 0);
                }
            }
        }
    }

    // epilogue: lane owns couts co0..co0+3 of voxel (m, vl)
    const int odim = DECONV ? dim * 2 : dim;
    const long long ovox_per_b = (long long)odim * odim * odim;
#pragma unroll
    for (int m = 0; m < M_T; ++m) {
        if (!vok[m]) continue;
        int oz = vz[m], oy = vy[m], ox = vx[m];
        if (DECONV) {
            oz = 2 * oz + (sub >> 2);
            oy = 2 * oy + ((sub >> 1) & 1);
            ox = 2 * ox + (sub & 1);
        }
        const long long on = ((long long)oz * odim + oy) * odim + ox;  // voxel index inside the sample
#pragma unroll
        for (int n = 0; n < N_T; ++n) conv_epilogue(a, acc[m][n], vb[m], on, ovox_per_b, (nt0 + n) * 16 + 4 * h);
    }
}

// ------------------------------------------------------------------------------------------------
// ConvTranspose3d(k=2, s=2) + folded BN (+skip add) + ReLU (Upsample3DBlock, reference network/v2v.py:55-67), all eight
// sub-positions of a voxel tile in ONE workgroup.  HBM-bound (2 B of input, 16 B of output + 16 B of skip tensor per
// input-voxel-channel pair at 64->32): the direct kernel's grid.z form re-reads the input eight times, leaves the two x
// neighbours of an output line pair to different workgroups and waits for the skip tensor behind its MFMAs; here the input
// fragments of a tile stay in registers over the eight sub-positions, the (2x, 2x+1) records of all cout tiles are written back to
// back by the same wave, and the skip records of a sub-position are requested in front of its MFMAs.
// A wave owns M_T tiles of 16 consecutive voxels; CGS = cin / 16, N_T = cout / 16 (all couts in one workgroup).
// ------------------------------------------------------------------------------------------------
// OUTQ (round 5, SE_OUT_QUAD; dim % 16 == 0): the output is QUAD-planar [B][cout/4][2D][2D][2D][4] - what the 3x3x3 kernel of the
// block behind it (back_layers.0, reference network/v2v.py:155) reads whole 16-byte records of.  A lane's D fragment is one record,
// but the records of ONE x parity are 32 bytes apart (round 2 measured such half-line stores at 0.147 -> 0.229 ms for the octet-planar
// form); here both parities of a (z, y) sub-position are computed first and exchanged across lanes (ds_bpermute: lane l takes voxel
// l >> 1, parity l & 1) so that a store instruction writes 16 consecutive records = 256 contiguous bytes per cout quad.
// RESQ (with OUTQ, SE_RES_QUAD; SE_EPI_RES_POST_RELU only): the skip tensor is quad-planar as well and is added BEHIND the exchange, where
// a lane holds the record it stores - the skip read is then the same 256 contiguous bytes per 16 lanes as the store (the channels-last
// skip read of a sub-position is 64-byte pieces at a 256-byte stride), and the block that produced the skip tensor writes whole records.
template <int CGS, int N_T, int M_T, bool OUTQ, bool RESQ = false>
__global__ __launch_bounds__(256) void deconv3d_k2s2_kernel(ConvArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vl = lane & 15;
    const int h = lane >> 4;
    const int dim = a.dim;
    const long long v_base = ((long long)blockIdx.x * 4 + wave) * (M_T * 16);
    int vb[M_T], vz[M_T], vy[M_T], vx[M_T];
    bool vok[M_T];
    f32x4 xf[M_T][CGS];
#pragma unroll
    for (int m = 0; m < M_T; ++m) {
        const long long vid = v_base + m * 16 + vl;
        vok[m] = vid < a.total_vox;
        long long t = vok[m] ? vid : 0;
        const float* src = a.in + t * a.cin_pad + 4 * h;
        vx[m] = (int)(t % dim); t /= dim;
        vy[m] = (int)(t % dim); t /= dim;
        vz[m] = (int)(t % dim); t /= dim;
        vb[m] = (int)t;
#pragma unroll
        for (int cg = 0; cg < CGS; ++cg) {
            xf[m][cg] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (vok[m]) xf[m][cg] = *reinterpret_cast<const f32x4*>(src + cg * 16);
        }
    }
    const int odim = dim * 2;
    const long long ovox_per_b = (long long)odim * odim * odim;
    const f32x4* wp = reinterpret_cast<const f32x4*>(a.wpack) + lane;
    const bool relu = a.flags & SE_EPI_RELU;
    const bool res_pre = !RESQ && (a.flags & SE_EPI_RES_PRE_RELU) && a.res, res_post = !RESQ && (a.flags & SE_EPI_RES_POST_RELU) && a.res;
    f32x4 bias[N_T];
#pragma unroll
    for (int n = 0; n < N_T; ++n) bias[n] = *reinterpret_cast<const f32x4*>(a.bpack + n * 16 + 4 * h);
    f32x4 val[OUTQ ? 2 : 1][M_T][N_T];      // OUTQ: finished records of the two x parities of a (z, y) sub-position
#pragma unroll 1
    for (int sub = 0; sub < 8; ++sub) {
        // output records of this sub-position; the skip tensor is requested first so that its latency lies under the MFMAs
        long long ooff[M_T];
        f32x4 rv[M_T][N_T];
#pragma unroll
        for (int m = 0; m < M_T; ++m) {
            const int oz = 2 * vz[m] + (sub >> 2), oy = 2 * vy[m] + ((sub >> 1) & 1), ox = 2 * vx[m] + (sub & 1);
            ooff[m] = ((long long)vb[m] * ovox_per_b + ((long long)oz * odim + oy) * odim + ox) * a.cout + 4 * h;
#pragma unroll
            for (int n = 0; n < N_T; ++n) {
                rv[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if ((res_pre || res_post) && vok[m]) rv[m][n] = *reinterpret_cast<const f32x4*>(a.res + ooff[m] + n * 16);
            }
        }
        f32x4 acc[M_T][N_T];
#pragma unroll
        for (int m = 0; m < M_T; ++m)
#pragma unroll
            for (int n = 0; n < N_T; ++n) acc[m][n] = bias[n];
#pragma unroll
        for (int cg = 0; cg < CGS; ++cg) {
            f32x4 wf[N_T];
#pragma unroll
            for (int n = 0; n < N_T; ++n) wf[n] = wp[((size_t)(cg * 8 + sub) * N_T + n) * 64];
            // k step outer, accumulators inner: consecutive MFMAs never share an accumulator
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int m = 0; m < M_T; ++m)
#pragma unroll
                    for (int n = 0; n < N_T; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[n][k], xf[m][cg][k], acc[m][n], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < M_T; ++m) {
            if (!OUTQ && !vok[m]) continue;
#pragma unroll
            for (int n = 0; n < N_T; ++n) {
                f32x4 v = acc[m][n];
                if (res_pre) v += rv[m][n];
                if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                if (res_post) v += rv[m][n];
                if constexpr (OUTQ) {
                    if (sub & 1) val[1][m][n] = v; else val[0][m][n] = v;
                } else {
                    *reinterpret_cast<f32x4*>(a.out + ooff[m] + n * 16) = v;
                }
            }
        }
        if constexpr (OUTQ) {
            if (!(sub & 1)) continue;
            // both x parities of (oz, oy) are finished: lane l of a 16-lane row takes (voxel l >> 1, parity l & 1) for the records
            // x0 .. x0 + 15 and (voxel 8 + (l >> 1), parity l & 1) for x0 + 16 .. x0 + 31; the tile's 16 voxels are one x run
            const int src_a = ((lane & 48) | (vl >> 1)) * 4, src_b = src_a + 32;
            const bool odd = vl & 1;
#pragma unroll
            for (int m = 0; m < M_T; ++m) {
                if (!vok[m]) continue;                 // uniform over the wave: the tile is 16 aligned voxels
                const int oz = 2 * vz[m] + (sub >> 2), oy = 2 * vy[m] + ((sub >> 1) & 1), ox0 = 2 * (vx[m] - vl) + vl;
#pragma unroll
                for (int n = 0; n < N_T; ++n) {
                    // (component by component, written out: with a `for (c)` loop over the vector elements hipcc 7.2 permuted only
                    // element 0 and splatted it over the record - disassembly, round 5)
                    auto pull = [&](int src, float e) {
                        return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, e)));
                    };
                    const f32x4 v0 = val[0][m][n], v1 = val[1][m][n];
                    const f32x4 a0 = {pull(src_a, v0.x), pull(src_a, v0.y), pull(src_a, v0.z), pull(src_a, v0.w)};
                    const f32x4 a1 = {pull(src_a, v1.x), pull(src_a, v1.y), pull(src_a, v1.z), pull(src_a, v1.w)};
                    const f32x4 b0 = {pull(src_b, v0.x), pull(src_b, v0.y), pull(src_b, v0.z), pull(src_b, v0.w)};
                    const f32x4 b1 = {pull(src_b, v1.x), pull(src_b, v1.y), pull(src_b, v1.z), pull(src_b, v1.w)};
                    f32x4 ra = odd ? a1 : a0, rb = odd ? b1 : b0;
                    const long long qo = (((((long long)vb[m] * (a.cout >> 2) + n * 4 + h) * odim + oz) * odim + oy) * odim + ox0) * 4;
                    if constexpr (RESQ) {       // quad-planar skip tensor: the records this lane stores
                        ra += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.res + qo));          // the skip tensor: read once
                        rb += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a.res + qo + 64));
                    }
                    float* o = a.out + qo;
                    *reinterpret_cast<f32x4*>(o) = ra;
                    *reinterpret_cast<f32x4*>(o + 64) = rb;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// max-pool 2x2x2 stride 2, channels-last, 16 B per lane
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool2_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                       long long total /* B*od^3*cq */, int od, int cq) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % cq);
    long long r = t / cq;
    const int x = (int)(r % od); r /= od;
    const int y = (int)(r % od); r /= od;
    const int z = (int)(r % od); r /= od;
    const long long b = r;
    const int id = od * 2;
    const int C = cq * 4;
    const float* p = in + ((((b * id + 2 * z) * id + 2 * y) * id + 2 * x) * (long long)C) + q * 4;
    f32x4 m = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const long long off = (((long long)(k >> 2) * id + ((k >> 1) & 1)) * id + (k & 1)) * C;
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + off);
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
    *reinterpret_cast<f32x4*>(out + t * 4) = m;
}

// same, octet-planar input [B][C/8][id^3][8]: thread = (voxel, channel quad); the two quads of an octet are adjacent threads, so a
// wave reads 32 contiguous bytes per input voxel and octet and still writes 16-byte channels-last pieces
__global__ __launch_bounds__(256) void maxpool2_octin_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             long long total /* B*od^3*cq */, int od, int cq) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % cq);
    long long r = t / cq;
    const int x = (int)(r % od); r /= od;
    const int y = (int)(r % od); r /= od;
    const int z = (int)(r % od); r /= od;
    const long long b = r;
    const int id = od * 2;
    const long long vox = (long long)id * id * id;
    const float* p = in + ((b * (cq >> 1) + (q >> 1)) * vox + ((long long)(2 * z) * id + 2 * y) * id + 2 * x) * 8 + (q & 1) * 4;
    f32x4 m = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const long long off = (((long long)(k >> 2) * id + ((k >> 1) & 1)) * id + (k & 1)) * 8;
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + off);
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
    *reinterpret_cast<f32x4*>(out + t * 4) = m;
}

template <int KS>
int launch_direct(const ConvArgs& a, hipStream_t s) {
    // cout tiles per workgroup: 2 when the layer has an even number of 16-wide cout tiles
    const long long vox_per_wg = 4 * 4 * 16;  // 4 waves x M_T=4 x 16
    const unsigned gx = (unsigned)((a.total_vox + vox_per_wg - 1) / vox_per_wg);
    if (a.nts % 2 == 0) {
        hipLaunchKernelGGL((conv3d_direct_kernel<KS, 4, 2, false>), dim3(gx, a.nts / 2), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL((conv3d_direct_kernel<KS, 4, 1, false>), dim3(gx, a.nts), dim3(256), 0, s, a);
    }
    SE_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// Any channels-last call with ksize 1, 3 or 7: nothing for the plan to check.
int se_conv3d_direct_launch(const ConvArgs& a, int ksize, hipStream_t s) {
    return ksize == 1 ? launch_direct<1>(a, s) : ksize == 3 ? launch_direct<3>(a, s) : launch_direct<7>(a, s);
}

extern "C" int se_deconv3d_k2s2_f32(const float* in, const float* wpack, const float* bpack, const float* residual,
                                    float* out, int batch, int dim, int cin, int cout, int flags, void* stream) {
    if (batch <= 0 || dim <= 0 || cin <= 0 || (cin & 15) || cout <= 0 || (cout & 15)) return SE_ERR_BAD_ARG;
    if (flags & SE_EPI_OUT_PLANAR) return SE_ERR_BAD_ARG;
    if ((flags & SE_EPI_RES_PRE_RELU) && (flags & SE_EPI_RES_POST_RELU)) return SE_ERR_BAD_ARG;
    if (flags & (SE_LAYOUT_OCTET_BITS | SE_IN_QUAD)) return SE_ERR_BAD_ARG;
    const bool outq = flags & SE_OUT_QUAD, resq = flags & SE_RES_QUAD;
    // a quad-planar skip tensor: only with the quad-planar output, added behind the ReLU (what the decoder does)
    if (resq && (!outq || !residual || !(flags & SE_EPI_RES_POST_RELU))) return SE_ERR_BAD_ARG;
    ConvArgs a;
    a.in = in; a.wpack = wpack; a.bpack = bpack; a.res = residual; a.out = out;
    a.total_vox = (long long)batch * dim * dim * dim;
    a.dim = dim; a.cin = cin; a.cin_pad = cin; a.cout = cout; a.nts = cout / 16; a.flags = flags & ~(SE_OUT_QUAD | SE_RES_QUAD);
    // all eight sub-positions per workgroup where that still fills the chip (measured at B=8: 64->32 from 32^3, 2048 workgroups,
    // 0.241 -> 0.149 ms = 4.05 TB/s; the 128->128 levels, 1..64 workgroups, 0.02 -> 0.14 ms: those keep the grid.z form, whose 8x
    // more workgroups matter more than the input re-reads there)
    const unsigned g2 = (unsigned)((a.total_vox + 127) / 128), g1 = (unsigned)((a.total_vox + 63) / 64);
#define SE_DECONV_CASE(CI, CO, MT, G)                                                                                          \
    if (cin == CI && cout == CO) {                                                                                             \
        hipLaunchKernelGGL((deconv3d_k2s2_kernel<CI / 16, CO / 16, MT, false>), dim3(G), dim3(256), 0, se_stream(stream), a); \
        SE_CHECK_LAUNCH();                                                                                                     \
        return 0;                                                                                                              \
    }
    if (outq) {
        // quad-planar output (SE_OUT_QUAD): the 64 -> 32 layer in front of back_layers.0, volumes whose x rows hold whole 16-voxel tiles
        if ((dim & 15) || !((cin == 64 && cout == 32) || (cin == 128 && cout == 64))) return SE_ERR_BAD_ARG;
        const bool two = g2 >= 4u * (unsigned)se_num_cus();
#define SE_DECONVQ(CG, NT, MT, G)                                                                                                      \
        do {                                                                                                                           \
            if (resq) hipLaunchKernelGGL((deconv3d_k2s2_kernel<CG, NT, MT, true, true>), dim3(G), dim3(256), 0, se_stream(stream), a); \
            else hipLaunchKernelGGL((deconv3d_k2s2_kernel<CG, NT, MT, true, false>), dim3(G), dim3(256), 0, se_stream(stream), a);     \
        } while (0)
        if (cin == 64 && two) SE_DECONVQ(4, 2, 2, g2);
        else if (cin == 64) SE_DECONVQ(4, 2, 1, g1);
        else if (two) SE_DECONVQ(8, 4, 2, g2);
        else SE_DECONVQ(8, 4, 1, g1);
#undef SE_DECONVQ
        SE_CHECK_LAUNCH();
        return 0;
    }
    if (g2 >= 4u * (unsigned)se_num_cus()) {
        SE_DECONV_CASE(64, 32, 2, g2)
        SE_DECONV_CASE(128, 64, 2, g2)
        SE_DECONV_CASE(128, 128, 2, g2)
    } else if (g1 >= 2u * (unsigned)se_num_cus()) {
        SE_DECONV_CASE(64, 32, 1, g1)
        SE_DECONV_CASE(128, 64, 1, g1)
    }
#undef SE_DECONV_CASE
    const long long vox_per_wg = 4 * 4 * 16;
    const unsigned gx = (unsigned)((a.total_vox + vox_per_wg - 1) / vox_per_wg);
    if (a.nts % 2 == 0) {
        hipLaunchKernelGGL((conv3d_direct_kernel<1, 4, 2, true>), dim3(gx, a.nts / 2, 8), dim3(256), 0, se_stream(stream), a);
    } else {
        hipLaunchKernelGGL((conv3d_direct_kernel<1, 4, 1, true>), dim3(gx, a.nts, 8), dim3(256), 0, se_stream(stream), a);
    }
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_maxpool3d_2_octin_f32(const float* in, float* out, int batch, int dim, int channels, void* stream) {
    if (batch <= 0 || dim <= 0 || (dim & 1) || channels <= 0 || (channels & 7)) return SE_ERR_BAD_ARG;
    const int od = dim / 2, cq = channels / 4;
    const long long total = (long long)batch * od * od * od * cq;
    hipLaunchKernelGGL(maxpool2_octin_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, se_stream(stream), in, out,
                       total, od, cq);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_maxpool3d_2_f32(const float* in, float* out, int batch, int dim, int channels, void* stream) {
    if (batch <= 0 || dim <= 0 || (dim & 1) || channels <= 0 || (channels & 3)) return SE_ERR_BAD_ARG;
    const int od = dim / 2, cq = channels / 4;
    const long long total = (long long)batch * od * od * od * cq;
    hipLaunchKernelGGL(maxpool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, se_stream(stream), in, out,
                       total, od, cq);
    SE_CHECK_LAUNCH();
    return 0;
}
