// V2V 3D convolutions on the gfx950 matrix cores, exact float32 (v_mfma_f32_16x16x4_f32).
//
// Layout: activations are channels-last [B][Z][Y][X][C]; a convolution is the implicit GEMM
//     out[cout][voxel] = sum_{tap, cin} W[cout][cin][tap] * in[voxel + tap][cin]
// One MFMA computes a 16(cout) x 16(voxel) tile over 4 values of k.  Operand maps (guide §3):
//     A: lane l holds A[i = l&15][k = l>>4]   -> weights,     i = cout
//     B: lane l holds B[k = l>>4][j = l&15]   -> activations, j = voxel
//     D: lane l holds D[i = 4*(l>>4) + r][j = l&15], r = 0..3 -> 4 consecutive couts of ONE voxel,
//        i.e. a 16-byte channels-last store per lane.
// A lane reads its activations as ONE 16-byte load: 4 consecutive channels c0..c0+3 with
// c0 = 16*cg + 4*(l>>4).  The four MFMAs j = 0..3 that consume it contract the channel set
// {16*cg + 4*h + j : h = 0..3}; the weight blocks are packed to match (se_conv3d_pack_f32), so a
// 16-channel group of one tap costs one 16-B load per operand and 4 MFMAs per (cout tile, voxel tile).
// The f32 MFMA is bit-for-bit an fmaf chain: no precision is traded for the matrix pipe.
//
// This file: the plan of a call (se_conv3d_plan: which kernel, in which slices of the batch) and the C entry points of the float32
// convolutions.  The kernels live one family per file, each behind a `_launch` function (conv3d_plan.h); the packed-weight format
// they read is conv3d_pack.h.
#include "common.h"

#include "conv3d_plan.h"

extern "C" int se_abi_version(void) { return 43; }

// Which family of kernels a default channels-last call (no SE_EPI_OUT_PLANAR / SE_EPI_RES_POST_RELU, cin_pad == cin) of this shape
// belongs to: 2 = 2-D Winograd, 1 = 1-D Winograd F(4,3), 7 = Winograd 7^3, 0 = none of them.  The shape predicates are the plan's.
extern "C" int se_conv3d_f32_algo(int dim, int cin, int cout, int ksize) {
    if (ksize == 3 && se_wino2d_shape_ok(dim, cin, cout)) return 2;
    if (ksize == 3 && se_wino1d_shape_ok(dim, cin, cout)) return 1;
    if (ksize == 7 && se_k7_wino_shape_ok(dim, cout)) return 7;
    return 0;
}

// flags that ask for one of the forms only the 2-D Winograd kernels have: octet- / quad-planar tensors, the fused skip convolution
constexpr int SE_FORM_FLAGS = SE_LAYOUT_OCTET_BITS | SE_LAYOUT_QUAD_BITS | SE_EPI_SKIPCONV16;
// a 2-D Winograd shape that is left to the in-workgroup split-K kernel of the small levels (conv_common.h: se_conv3d_small_volume)
static bool small_plain_call(int batch, int dim, int flags) { return !(flags & SE_FORM_FLAGS) && se_conv3d_small_volume(batch, dim); }

// Which kernel a launch of `batch` samples with these layout flags (SE_IN_OCTET ...) runs on: se_conv3d_f32_algo's value, except
//   3 = the F(4,3) x F(4,3) ping-pong kernel (conv3d_wino44pp.hip; a member of the 2-D Winograd family: same layouts, flags and fused
//       forms as algo 2) - it declines a channels-last input with >= 32 channels, which stays on algo 2 (se_conv3d_wino44pp_layout_ok);
//   0 for a 2-D Winograd shape with <= 4096 voxels in the batch when the call asks for no octet-planar / pooled / fused form.
// Computed from the predicates of se_conv3d_plan, for the call this signature can describe: cin_pad == cin, no second output, and
// of the flags only the SE_FORM_FLAGS are looked at.  The plan sees more, and where it does this answer is the LESS strict one: with
// cin_pad != cin, SE_EPI_RES_POST_RELU or SE_EPI_OUT_PLANAR no 2-D Winograd kernel runs (the call goes to the 1-D / tiled / direct
// kernels, or is SE_ERR_BAD_ARG if it asks for a planar form), yet 2 or 3 is returned here; and a pooled output keeps a small volume
// on the 2-D kernel where 0 is returned here.  V2VProgram asks with cin_pad == cin and none of those flags, where both agree.
extern "C" int se_conv3d_f32_variant(int batch, int dim, int cin, int cout, int ksize, int flags) {
    const int algo = se_conv3d_f32_algo(dim, cin, cout, ksize);
    if (algo == 2 && small_plain_call(batch, dim, flags)) return 0;
    if (algo == 2 && g_variant != 64 && se_conv3d_wino44pp_shape(batch, dim, cout) && se_conv3d_wino44pp_layout_ok(cin, flags)) return 3;
    return algo;
}

#ifndef SE_HALO64
#define SE_HALO64 1
#endif

// The plan of one call.  Order of preference: the 2-D Winograd kernels, the 1-D Winograd kernel, the LDS-tiled direct kernels (these
// run in slices of the batch), then the kernels of the small levels and the direct kernel (whole batch).  A call that asks for a
// tensor layout or fused output which the kernel its shape and flags lead to does not have is an error: no other kernel would read
// or write those tensors the way the caller laid them out.
SeConvPlan se_conv3d_plan(const ConvArgs& a, int batch, int ksize) {
    const int dim = a.dim, flags = a.flags, cus = se_num_cus();
    SeConvPlan p = {SE_CONV_DIRECT, ksize, batch, 1, 0, 0};
    // samples per launch of the sliced kernels.  Unit-table budget: the smallest table among the persistent kernels holds ~430 entries
    // per workgroup; at most 32 samples (weak-scaling config 4 runs 32 samples per GPU, i.e. exactly one slice)
    const long long t8 = dim / 8;
    const long long units_per_sample = ksize == 7 ? t8 * t8 * t8 : (long long)(a.cout >= 32 ? a.cout / 32 : 1) * (dim / 4) * t8 * t8;
    const long long budget = units_per_sample > 0 ? 400LL * cus / units_per_sample : 32;
    const int slice = (int)(budget < 1 ? 1 : budget > 32 ? 32 : budget);
    const int n = batch < slice ? batch : slice, tail = batch % n;   // every launch has n samples, the last one `tail` if that is not 0
    const auto sliced = [&p, n](int kernel, int form) {
        p.kernel = kernel, p.form = form, p.slice = n;
        if (form < 0) p.error = SE_ERR_BAD_ARG;
        return p;
    };
    const auto bad_arg = [&p] { p.error = SE_ERR_BAD_ARG; return p; };
    const auto fits = [n, tail](auto&& pred) { return pred(n) && (!tail || pred(tail)); };

    const bool forms = (flags & SE_FORM_FLAGS) || a.pool_out || a.skip_w;
    const bool plain_epilogue = !(flags & (SE_EPI_RES_POST_RELU | SE_EPI_OUT_PLANAR));
    const bool in_2d = ksize == 3 && a.wpack_g && a.cin_pad == a.cin && se_wino2d_shape_ok(dim, a.cin, a.cout) && plain_epilogue;
    const bool in_1d = ksize == 3 && a.wpack_e && a.cin_pad == a.cin && se_wino1d_shape_ok(dim, a.cin, a.cout) && plain_epilogue &&
                       !(flags & (SE_LAYOUT_OCTET_BITS | SE_LAYOUT_QUAD_BITS));
    const bool in_tiled = dim >= 16 && (dim & 7) == 0 && (a.cout & 15) == 0 && (ksize == 3 || (ksize == 7 && a.nts == 1));
    const bool in_k7w = ksize == 7 && a.wpack_f && se_k7_wino_shape_ok(dim, a.cout) && !a.res && !(flags & SE_EPI_OUT_PLANAR);
    const bool fits_2d = fits([&](int nb) { return se_conv3d_wino2d_fits(nb, dim, a.cout); });
    const bool fits_1d = in_1d && fits([&](int nb) { return se_conv3d_wino1d_fits(SE_CONV_WINO43PP_1D, nb, dim, a.cout, cus); });

    // what is tried at all: everything, unless a development build's A/B selection says otherwise
    bool small_to_splitk = true, try_2d = true, try_44pp = true, try_1d = true, try_k7w = true, try_67 = true, try_wavesplit = true;
    long long wavesplit_min_vox = 2048;
#ifdef SE_DEVTOOLS
    // se_debug_set_variant(g): which kernel families g switches off, and which instance of a production kernel template it names
    // (reached where the production order would reach that kernel).  The only place of the plan that knows about variants; g = 0
    // is the production plan, every other g also keeps tiny 2-D Winograd shapes off the small-level kernels.
    //   1 - 9     no Winograd kernel: the LDS-tiled direct, small-level and direct kernels
    //   10 - 19   no 2-D Winograd kernel: 1-D F(4,3) and the Winograd 7^3 kernels;
    //             18: grid split-K for every small level, 19: in-workgroup split-K for every small level
    //   21 - 23   3^3 on the LDS-tiled direct kernel with 8 x 8 x {4, 8, 16} output tiles (the tile-size sweep of BASELINE config 5)
    //   30        1-D F(4,3) where production runs a 2-D Winograd kernel
    //   40        the production families
    //   41 - 60   3^3: experiment and attribution instances of the F(4,3) x F(2,3) kernel (conv3d_wino2d.hip lists them);
    //             47 on a 7^3 layer: F(4,7) where production runs F(6,7)
    //   64        the 2-D family stays on F(4,3) x F(2,3)
    //   70 - 79   read by conv2d_1x1.hip and conv2d_3x3.hip
    if (const int g = g_variant) {
        small_to_splitk = false;
        try_2d = g >= 40 && g < 70, try_44pp = g == 40;
        try_1d = g == 30 || (g >= 10 && g < 20);
        try_k7w = g >= 10, try_67 = g != 47;
        try_wavesplit = g != 18, wavesplit_min_vox = g == 19 ? 0 : 2048;
        if (try_2d && in_2d && fits_2d && g >= 41) {
            const int octets = ((flags & SE_IN_OCTET) ? 1 : 0) | ((flags & SE_OUT_OCTET) ? 2 : 0) | ((flags & SE_RES_OCTET) && a.res ? 4 : 0);
            const bool quad_ok = !(flags & SE_LAYOUT_QUAD_BITS) || se_conv3d_wino2d_form(a) >= 0;   // for forms 0 and 3 (and run AS those)
            if (quad_ok && (octets == 0 || octets == 3)) {
                p.exp = g;
                return sliced(SE_CONV_WINO2D, octets);
            }
        }
        if (g >= 21 && g <= 23 && !forms && in_tiled && ksize == 3 && a.nts % 2 == 0 && dim % 16 == 0)   // no Winograd kernel is tried
            return sliced(SE_CONV_DEV_TILED_K3_TZ, 4 << (g - 21));
    }
#endif

    // tiny volumes of 2-D Winograd shapes (16^3 at batch 1: 32 work units for 256 CUs): a plain channels-last call is left to the
    // in-workgroup split-K kernel of the 8^3 level (47 against 92 us per 128 -> 128 launch); a caller that asks for an octet-planar /
    // pooled / fused-skip form gets the 2-D kernel
    const bool to_small_levels = small_to_splitk && in_2d && !forms && small_plain_call(batch, dim, flags);
    if (!to_small_levels) {
        if (try_2d && in_2d) {
            // the 64^3 / 32^3 levels run on the F(4,3) x F(4,3) ping-pong kernel (1/4 of the direct MFMAs; the F(4,3) x F(2,3) kernel: 1/3)
            if (try_44pp && a.wpack_i && se_conv3d_wino44pp_layout_ok(a.cin, flags) && se_conv3d_wino44pp_shape(batch, dim, a.cout) &&
                fits([&](int nb) { return se_conv3d_wino44pp_fits(nb, dim, a.cout); }))
                return sliced(SE_CONV_WINO44PP, se_conv3d_wino44pp_form(a));
            if (fits_2d) return sliced(SE_CONV_WINO2D, se_conv3d_wino2d_form(a));
        }
        if (forms) return bad_arg();
        if (try_1d && fits_1d) return sliced(SE_CONV_WINO43PP_1D, 0);
        if (in_tiled && ksize == 3) return sliced(SE_CONV_TILED_K3, a.nts % 4 == 0 ? 4 : a.nts % 2 == 0 ? 2 : 1);
        if (in_tiled) {   // 7^3 with 16 output channels
            const bool p3 = flags & SE_IN_PLANAR3;
            if (try_k7w && in_k7w) {
                if (try_67 && a.wpack_h && (dim & 15) == 0 && fits([&](int nb) { return se_conv3d_k7_wino67_fits(a, nb, cus); }))
                    return sliced(SE_CONV_K7_WINO67, 0);
                if (fits([&](int nb) { return se_conv3d_k7_wino47_fits(nb, dim, cus); }))
                    return sliced(p3 ? SE_CONV_K7_WINO47_P3 : SE_CONV_K7_WINO47_CL, 0);
            }
            if (p3) return bad_arg();
            return sliced(SE_CONV_TILED_K7, 0);
        }
    }

    // the small levels, odd volumes and the planar 15-channel output layer: channels-last input, whole batch in one launch
    if (flags & (SE_LAYOUT_OCTET_BITS | SE_LAYOUT_QUAD_BITS | SE_IN_PLANAR3)) return bad_arg();
    const bool cout_pairs = ksize == 3 && !(flags & SE_EPI_OUT_PLANAR) && a.nts % 2 == 0;   // these kernels own two cout tiles per workgroup
    if (cout_pairs && try_wavesplit && a.total_vox <= 8192 && a.total_vox * a.cin_pad * 4LL < (1LL << 31) && a.total_vox >= wavesplit_min_vox) {
        // 8^3-sized levels: in-workgroup split-K, single launch (0.063 vs 0.077 ms for grid split-K + reduce at B = 8)
        // ... on the bf16 matrix pipe (six-product split form) when the caller brought the layer's split planes
        if (SE_HALO64 && a.total_vox >= 2048 && (dim == 8 || dim == 16) && (a.cin & 31) == 0)
            p.kernel = a.wsplit6 && se_conv3d_halo64_s6_domain(a) ? SE_CONV_HALO64_S6 : SE_CONV_HALO64, p.form = dim;
        else p.kernel = SE_CONV_WAVESPLIT, p.form = a.total_vox >= 2048 ? 4 : a.total_vox >= 256 ? 8 : 16;
        return p;
    }
    if (cout_pairs && a.ws) {
        // small volumes with wide channels: split the taps over grid.z when the plain launch would not fill the chip
        const long long wgs = (a.total_vox + 63) / 64 * (a.nts / 2);
        int splits = 27;                                  // taps per split: 1, 3, 9 (or no split)
        while (splits > 1 && (wgs * (splits / 3) >= 2048 || (long long)splits * a.total_vox * a.cout > a.ws_elems)) splits /= 3;
        if (wgs < 1024 && splits > 1) p.kernel = SE_CONV_SPLITK_GRID, p.splits = splits;
    }
    return p;
}

// One launch of the planned kernel on `batch` samples (a slice of the call, or all of it).
static int launch_planned(const SeConvPlan& p, const ConvArgs& a, int batch, hipStream_t s) {
    switch (p.kernel) {
        case SE_CONV_WINO44PP: return se_conv3d_wino44pp_launch(a, batch, p.form, s);
        case SE_CONV_WINO2D: return se_conv3d_wino2d_launch(a, batch, p.form, p.exp, s);
        case SE_CONV_K7_WINO67:
        case SE_CONV_K7_WINO47_P3:
        case SE_CONV_K7_WINO47_CL: return se_conv3d_k7_wino_launch(a, batch, p.kernel, s);
        case SE_CONV_WINO43PP_1D: return se_conv3d_wino1d_launch(a, batch, p.kernel, s);
        case SE_CONV_TILED_K3:
        case SE_CONV_TILED_K7: return se_conv3d_tiled_launch(a, batch, p.kernel, p.form, s);
        case SE_CONV_HALO64:
        case SE_CONV_HALO64_S6:
        case SE_CONV_WAVESPLIT:
        case SE_CONV_SPLITK_GRID: return se_conv3d_small_launch(a, p, s);
        case SE_CONV_DIRECT: return se_conv3d_direct_launch(a, p.form, s);
#ifdef SE_DEVTOOLS
        case SE_CONV_DEV_TILED_K3_TZ: return se_conv3d_tiled_launch(a, batch, p.kernel, p.form, s);
#endif
        default: return SE_ERR_BAD_ARG;
    }
}

static int conv3d_f32_impl(const float* in, const float* wpack, const unsigned short* wsplit6, const float* bpack, const float* residual, float* out,
                           float* pool_out, const float* skip_w, int batch, int dim, int cin, int cin_pad, int cout, int ksize, int flags,
                           float* workspace, long long workspace_elems, void* stream) {
    if (batch <= 0 || dim <= 0 || cin <= 0 || cin_pad < cin || (cin_pad & 15) || cout <= 0) return SE_ERR_BAD_ARG;
    if (ksize != 1 && ksize != 3 && ksize != 7) return SE_ERR_BAD_ARG;
    const bool planar = flags & SE_EPI_OUT_PLANAR;
    if (!planar && (cout & 15)) return SE_ERR_BAD_ARG;
    if (planar && (flags & (SE_EPI_RES_PRE_RELU | SE_EPI_RES_POST_RELU))) return SE_ERR_BAD_ARG;
    if ((flags & SE_EPI_RES_PRE_RELU) && (flags & SE_EPI_RES_POST_RELU)) return SE_ERR_BAD_ARG;
    const int algo = se_conv3d_f32_algo(dim, cin, cout, ksize);
    if (!skip_w && (flags & SE_EPI_SKIPCONV16)) return SE_ERR_BAD_ARG;
    if (skip_w && (!residual || algo != 2 || cin_pad != cin)) return SE_ERR_BAD_ARG;
    if (pool_out && ((dim & 1) || algo != 2 || cin_pad != cin)) return SE_ERR_BAD_ARG;   // only the 2-D Winograd kernels pool
    if ((flags & SE_IN_PLANAR3) && ksize != 7) return SE_ERR_BAD_ARG;
    if ((flags & (SE_LAYOUT_OCTET_BITS | SE_LAYOUT_QUAD_BITS)) && algo != 2) return SE_ERR_BAD_ARG;
    if ((flags & SE_LAYOUT_OCTET_BITS) && (flags & SE_LAYOUT_QUAD_BITS)) return SE_ERR_BAD_ARG;
    // quad-planar tensors exist in the F(4,3) x F(4,3) kernel only - and as the OUTPUT of a channels-last launch of the F(4,3) x F(2,3) one
    if ((flags & SE_LAYOUT_QUAD_BITS) && se_conv3d_f32_variant(batch, dim, cin, cout, ksize, flags) != 3 &&
        (flags & SE_LAYOUT_QUAD_BITS) != SE_OUT_QUAD)
        return SE_ERR_BAD_ARG;
    const long long vox = (long long)dim * dim * dim;
    ConvArgs a;
    a.in = in; a.bpack = bpack; a.res = residual; a.out = out;
    se_conv_args_set_sections(a, wpack, se_conv3d_pack_layout(cout, cin_pad, ksize, 0));
    a.wsplit6 = wsplit6;
    a.total_vox = batch * vox;
    a.dim = dim; a.cin = cin; a.cin_pad = cin_pad; a.cout = cout; a.nts = round_up16(cout) / 16; a.flags = flags;
    a.pool_out = pool_out;
    a.skip_w = skip_w;
    a.ws = workspace;
    a.ws_elems = workspace ? workspace_elems : 0;
    const SeConvPlan p = se_conv3d_plan(a, batch, ksize);
    if (p.error) return p.error;
    hipStream_t s = se_stream(stream);
    for (int b0 = 0; b0 < batch; b0 += p.slice) {
        const int nb = batch - b0 < p.slice ? batch - b0 : p.slice;
        ConvArgs sl = a;
        // floats per voxel of the input: channels-last record, or 3 x ceil(cin/3) planes for the triplet-planar 7^3 input
        sl.in = a.in + b0 * vox * ((flags & SE_IN_PLANAR3) ? (cin + 2) / 3 * 3 : cin_pad);
        sl.out = a.out + b0 * vox * cout;
        if (a.res) sl.res = a.res + b0 * vox * ((flags & SE_EPI_SKIPCONV16) ? 16 : cout);
        if (a.pool_out) sl.pool_out = a.pool_out + b0 * (vox / 8) * cout;
        sl.total_vox = nb * vox;
        const int rc = launch_planned(p, sl, nb, s);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int se_conv3d_f32(const float* in, const float* wpack, const float* bpack, const float* residual,
                             float* out, int batch, int dim, int cin, int cin_pad, int cout, int ksize, int flags,
                             float* workspace, long long workspace_elems, void* stream) {
    return conv3d_f32_impl(in, wpack, nullptr, bpack, residual, out, nullptr, nullptr, batch, dim, cin, cin_pad, cout, ksize, flags, workspace,
                           workspace_elems, stream);
}

// se_conv3d_f32 for a layer that also has split planes (se_conv3d_split6_pack): the plan may then choose a six-product bf16 form
// (split6.h) where one exists and is the faster kernel; with wsplit6 == NULL this IS se_conv3d_f32.
extern "C" int se_conv3d_w6_f32(const float* in, const float* wpack, const se_bf16* wsplit6, const float* bpack, const float* residual,
                                float* out, int batch, int dim, int cin, int cin_pad, int cout, int ksize, int flags,
                                float* workspace, long long workspace_elems, void* stream) {
    return conv3d_f32_impl(in, wpack, wsplit6, bpack, residual, out, nullptr, nullptr, batch, dim, cin, cin_pad, cout, ksize, flags, workspace,
                           workspace_elems, stream);
}

// 1 when se_conv3d_w6_f32 runs this call (cin_pad == cin, a workspace, split planes given) on a six-product bf16 form, else 0:
// the plan's own answer, for the route record of the V2V program.
extern "C" int se_conv3d_f32_split6(int batch, int dim, int cin, int cout, int ksize, int flags) {
    if (batch <= 0 || dim <= 0 || cin <= 0 || (cin & 15) || cout <= 0 || (cout & 15) || (ksize != 1 && ksize != 3 && ksize != 7)) return 0;
    static const float dummy[4] = {0.f, 0.f, 0.f, 0.f};      // section pointers are compared with NULL by the plan, never read
    ConvArgs a;
    a.in = nullptr; a.bpack = nullptr; a.res = nullptr; a.out = nullptr;
    se_conv_args_set_sections(a, dummy, se_conv3d_pack_layout(cout, cin, ksize, 0));
    a.wsplit6 = se_split6_packed_elems(cout, cin, ksize, 0) > 0 ? reinterpret_cast<const unsigned short*>(dummy) : nullptr;
    a.total_vox = (long long)batch * dim * dim * dim;
    a.dim = dim; a.cin = cin; a.cin_pad = cin; a.cout = cout; a.nts = round_up16(cout) / 16; a.flags = flags;
    const SeConvPlan p = se_conv3d_plan(a, batch, ksize);
    return !p.error && p.kernel == SE_CONV_HALO64_S6;
}

// The split form of the 64-voxel-tile kernel on its whole domain (se_conv3d_halo64_s6_domain: dim 8 or 16, cin and cin_pad % 32 == 0,
// cout % 32 == 0, at most 8192 voxels in the batch), whatever the plan would run the call on: what the tests of the form launch.
// flags: SE_EPI_RELU, SE_EPI_RES_PRE_RELU / _POST_RELU.  SE_ERR_BAD_ARG otherwise (nothing launched).
extern "C" int se_conv3d_k3_split6_f32(const float* in, const se_bf16* wsplit6, const float* bpack, const float* residual, float* out,
                                       int batch, int dim, int cin, int cin_pad, int cout, int flags, void* stream) {
    if (!in || !wsplit6 || !bpack || !out || batch <= 0 || cin <= 0 || cin_pad < cin || cout <= 0 || (cout & 15)) return SE_ERR_BAD_ARG;
    if (flags & ~(SE_EPI_RELU | SE_EPI_RES_PRE_RELU | SE_EPI_RES_POST_RELU)) return SE_ERR_BAD_ARG;
    if ((flags & SE_EPI_RES_PRE_RELU) && (flags & SE_EPI_RES_POST_RELU)) return SE_ERR_BAD_ARG;
    ConvArgs a;
    a.in = in; a.wpack = nullptr; a.wsplit6 = wsplit6; a.bpack = bpack; a.res = residual; a.out = out;
    a.total_vox = (long long)batch * dim * dim * dim;
    a.dim = dim; a.cin = cin; a.cin_pad = cin_pad; a.cout = cout; a.nts = cout / 16; a.flags = flags;
    if (!se_conv3d_halo64_s6_domain(a)) return SE_ERR_BAD_ARG;
    const SeConvPlan p = {SE_CONV_HALO64_S6, dim, batch, 1, 0, 0};
    return se_conv3d_small_launch(a, p, se_stream(stream));
}

// Same convolution; the kernel also writes max_pool3d(out, kernel 2, stride 2) (channels-last) from its epilogue, so the 2x pool
// of a Res3DBlock output (reference network/v2v.py:104-119: encoder_pool after the front / encoder blocks) does not re-read it.
extern "C" int se_conv3d_pool_f32(const float* in, const float* wpack, const float* bpack, const float* residual,
                                  float* out, float* pool_out, int batch, int dim, int cin, int cin_pad, int cout, int ksize,
                                  int flags, float* workspace, long long workspace_elems, void* stream) {
    if (!pool_out) return SE_ERR_BAD_ARG;
    return conv3d_f32_impl(in, wpack, nullptr, bpack, residual, out, pool_out, nullptr, batch, dim, cin, cin_pad, cout, ksize, flags, workspace,
                           workspace_elems, stream);
}

extern "C" int se_conv3d_skip16_f32(const float* in, const float* wpack, const float* bpack, const float* skip_in,
                                    const float* skip_w, float* out, int batch, int dim, int cin, int cout, int flags,
                                    void* stream) {
    if (!skip_in || !skip_w) return SE_ERR_BAD_ARG;
    const int lay = flags & ~SE_EPI_RELU;
    if (lay != (SE_IN_OCTET | SE_OUT_OCTET) && lay != (SE_IN_QUAD | SE_OUT_QUAD) && lay != (SE_IN_QUAD | SE_OUT_QUAD | SE_RES_QUAD)) return SE_ERR_BAD_ARG;
    return conv3d_f32_impl(in, wpack, nullptr, bpack, skip_in, out, nullptr, skip_w, batch, dim, cin, cin, cout, 3,
                           flags | SE_EPI_SKIPCONV16, nullptr, 0, stream);
}
