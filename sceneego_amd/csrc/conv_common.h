// Shared between the float32 3D convolution files: conv3d.hip (plan, C ABI) and one file per kernel family (conv3d_plan.h lists them).
#pragma once
#include "common.h"
#include "conv3d_pack.h"   // the packed-weight format: chunk sizes, SePackLayout, round_up16

// XCD-aware walk of the persistent kernels (round 5).  Workgroups are dealt to the 8 XCDs round-robin (workgroup b runs on XCD b % 8,
// each XCD has its own L2), so with unit ranges in blockIdx order the NEIGHBOURING ranges - which share their halo rows - sit in eight
// different L2s and every shared row is fetched from the fabric once per L2.  Virtual index: the workgroups of one XCD walk
// consecutive ranges, the halo between them is an L2 hit.  (Round 4 measured the same map at -2 ... +1 % of time - the kernels are not
// bound by where their rows come from; what it buys is fabric traffic: SE_XCD_WALK=0 in an A/B build restores blockIdx order.)
#ifndef SE_XCD_WALK
#define SE_XCD_WALK 1
#endif
__device__ __forceinline__ int se_xcd_walk_index(int wg, int n_wg) {
    return (SE_XCD_WALK && (n_wg & 7) == 0) ? (wg & 7) * (n_wg >> 3) + (wg >> 3) : wg;
}
// The interleaved form of the same idea (workgroup w of an XCD's S takes units w, w + S, ...: the S tiles in flight on an XCD are S
// consecutive units) lives in the kernels that have it: SE_K44P_XCD_WALK (on), SE_K67_XCD_WALK (off).

// Shapes the 2-D Winograd 3x3x3 kernel (conv3d_wino2d.hip) covers - ONE predicate for se_conv3d_f32_algo() (what callers use to
// choose the octet-planar / pooled / fused-skip forms) and for the launcher.  `cin` is the channel stride of the input tensor (the
// kernel needs cin_pad == cin).  The last term: 32-bit byte offsets inside one sample (bit 31 marks out-of-volume lanes).
inline bool se_wino2d_shape_ok(int dim, int cin, int cout) {
    if (dim < 16 || (dim & 15) || cout <= 0 || (cout & 31) || cin <= 0 || (cin & 7)) return false;
    return (long long)dim * dim * dim * (cin > cout ? cin : cout) * 4 < (1LL << 31);
}

// A 2-D Winograd shape with so few voxels that its 4 x 8 x 16 tiles leave most of the chip idle (16^3 at batch 1: 8 tiles x 4 cout
// blocks on 256 CUs, 92 us per 128 -> 128 launch): a call WITHOUT octet-planar / pooled / fused-skip forms then runs on the
// in-workgroup split-K kernel of the 8^3 level (32-voxel tiles, 512 workgroups, 47 us).  se_conv3d_f32_variant() reports it, the
// V2V program asks per (batch, level).
inline bool se_conv3d_small_volume(int batch, int dim) { return (long long)batch * dim * dim * dim <= 4096; }
// Shapes of the 1-D Winograd F(4,3) 3^3 kernel (conv3d_wino.hip; 4 x 8 x 8 tiles, 16-channel chunks, 32-cout blocks) and of the
// Winograd 7^3 kernels (conv3d_wino67.hip, conv3d_wino47.hip; 16 output channels) - as se_wino2d_shape_ok, for the plan and the queries.
inline bool se_wino1d_shape_ok(int dim, int cin, int cout) { return dim >= 16 && (dim & 7) == 0 && (cout & 31) == 0 && (cin & 15) == 0; }
inline bool se_k7_wino_shape_ok(int dim, int cout) { return dim >= 16 && (dim & 7) == 0 && cout == 16; }

struct ConvArgs {
    const float* in;
    const float* wpack;    // section A
    const float* wpack_b = nullptr;  // section B (NULL when absent, as every section pointer below)
    const float* wpack_e = nullptr;  // section E
    const float* wpack_f = nullptr;  // section F
    const float* wpack_h = nullptr;  // section H
    const float* wpack_i = nullptr;  // section I
    const float* wpack_g = nullptr;  // section G
    const unsigned short* wsplit6 = nullptr;  // the layer's split planes (se_conv3d_split6_pack; a buffer of its own), NULL: float32 forms only
    const float* skip_w = nullptr;   // SE_EPI_SKIPCONV16: folded 1x1x1 skip weights [cout][16]; `res` then is the skip convolution's 16-channel input
    float* pool_out = nullptr;       // 2-D Winograd kernel only: also write max_pool3d(out, 2, 2), channels-last [B][D/2][D/2][D/2][cout] (else NULL)
    const float* bpack;
    const float* res;
    float* out;
    long long total_vox;  // B * dim^3 (input voxels)
    int dim;
    int cin;       // real input channels (chunks beyond it are skipped: their weights are zero)
    int cin_pad;   // channel stride of the input tensor
    int cout;      // real output channels
    int nts;       // cout tiles of 16 in the packed weights
    int flags;
    float* ws = nullptr;          // the caller's workspace (se_conv3d_f32): split-K partial sums of the small levels, second-half sums of a split 7^3 launch
    long long ws_elems = 0;
};

// Points a call's section pointers at the sections its packed buffer has (NULL where the layout has none).
inline void se_conv_args_set_sections(ConvArgs& a, const float* wpack, const SePackLayout& l) {
    a.wpack = wpack;
    a.wpack_b = l.section(wpack, SE_PACK_B);
    a.wpack_e = l.section(wpack, SE_PACK_E);
    a.wpack_f = l.section(wpack, SE_PACK_F);
    a.wpack_g = l.section(wpack, SE_PACK_G);
    a.wpack_h = l.section(wpack, SE_PACK_H);
    a.wpack_i = l.section(wpack, SE_PACK_I);
}

// Epilogue for one accumulator fragment: this lane owns output channels co0..co0+3 of one voxel
// (`on` = voxel index inside sample `b`, `ovox_per_b` voxels per sample).  bias (+BN shift) -> [+res] -> [ReLU]
// -> [+res] -> 16-byte channels-last store, or 4 planar stores for SE_EPI_OUT_PLANAR.
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x4 v, int b, long long on, long long ovox_per_b,
                                              int co0) {
    if (co0 >= a.cout) return;
    v += *reinterpret_cast<const f32x4*>(a.bpack + co0);
    const bool relu = a.flags & SE_EPI_RELU;
    if (a.flags & SE_EPI_OUT_PLANAR) {
        float* o = a.out + ((long long)b * a.cout + co0) * ovox_per_b + on;
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (co0 + r < a.cout) o[(long long)r * ovox_per_b] = relu ? fmaxf(vv[r], 0.f) : vv[r];
        }
        return;
    }
    const long long ooff = ((long long)b * ovox_per_b + on) * a.cout + co0;
    if ((a.flags & SE_EPI_RES_PRE_RELU) && a.res) v += *reinterpret_cast<const f32x4*>(a.res + ooff);
    if (relu) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    if ((a.flags & SE_EPI_RES_POST_RELU) && a.res) v += *reinterpret_cast<const f32x4*>(a.res + ooff);
    *reinterpret_cast<f32x4*>(a.out + ooff) = v;
}
