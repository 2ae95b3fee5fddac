// Which kernel a float32 3D convolution call (se_conv3d_f32 / _pool_f32 / _skip16_f32) runs on: decided ONCE per call, on the whole
// batch, before anything is launched (se_conv3d_plan, conv3d.hip).  Every kernel file exports what the plan needs to know about its
// kernel - a `_fits` predicate next to the constants that bound its unit table, a `_form` function next to the list of template
// instances - and a `_launch` function whose preconditions the plan has checked.
#pragma once
#include "conv_common.h"

enum SeConvKernel {
    SE_CONV_WINO44PP,        // 2-D Winograd F(4,3) x F(4,3), ping-pong (conv3d_wino44pp.hip); form: L of conv3d_k3_wino44pp_kernel<L>
    SE_CONV_WINO2D,          // 2-D Winograd F(4,3) x F(2,3) (conv3d_wino2d.hip); form: L of conv3d_k3_wino2d_kernel<E, L>
    SE_CONV_WINO43PP_1D,     // 1-D Winograd F(4,3), ping-pong (conv3d_wino.hip)
    SE_CONV_K7_WINO67,       // 7^3: 1-D Winograd F(6,7) (conv3d_wino67.hip), either input layout
    SE_CONV_K7_WINO47_P3,    // 7^3: 1-D Winograd F(4,7), triplet-planar input (conv3d_wino47.hip)
    SE_CONV_K7_WINO47_CL,    // 7^3: 1-D Winograd F(4,7), channels-last input
    SE_CONV_TILED_K3,        // LDS-tiled direct 3^3 (conv3d_tiled.hip); form: cout tiles per workgroup (4, 2, 1)
    SE_CONV_TILED_K7,        // LDS-tiled direct 7^3
    SE_CONV_HALO64,          // small levels (conv3d_small.hip): 64-voxel tiles through LDS; form: dim (8, 16)
    SE_CONV_HALO64_S6,       // small levels: the six-product bf16 form of SE_CONV_HALO64 (split6.h; needs ConvArgs::wsplit6); form: dim (8, 16)
    SE_CONV_WAVESPLIT,       // small levels: in-workgroup split-K; form: waves per workgroup (4: two cout tile pairs of 2 x 4 waves, 8, 16)
    SE_CONV_SPLITK_GRID,     // small levels: taps split over grid.z into the caller's workspace + reduce; `splits`
    SE_CONV_DIRECT,          // any shape (conv3d_direct.hip): activations straight from global memory; form: ksize
#ifdef SE_DEVTOOLS           // reachable only through se_debug_set_variant
    SE_CONV_DEV_TILED_K3_TZ, // (21-23) LDS-tiled direct 3^3 with 8 x 8 x form output tiles (4, 8, 16), 2 cout tiles
#endif
};

struct SeConvPlan {
    int kernel;   // SeConvKernel
    int form;     // the template / layout selector of that kernel's launcher (see SeConvKernel)
    int slice;    // samples per launch: the persistent kernels keep a table of their work units in LDS, a larger batch is cut up
    int splits;   // SE_CONV_SPLITK_GRID: parts the 27 taps are split into
    int exp;      // development builds: the se_debug_set_variant experiment of conv3d_k3_wino2d_kernel<E, L> (0: none)
    int error;    // SE_ERR_BAD_ARG: no kernel serves the call as its tensors are laid out; else 0
};

// Pure: launches nothing, allocates nothing, reads a (wpack_* say which weight sections exist) and se_num_cus().
SeConvPlan se_conv3d_plan(const ConvArgs& a, int batch, int ksize);

// ---- what the kernel files export; `batch` is the number of samples of ONE launch, preconditions are the plan's to check ----
// conv3d_wino44pp.hip.  _shape: on the batch of the whole call; _form: L, or -1 for a combination that is not instantiated
bool se_conv3d_wino44pp_shape(int batch, int dim, int cout);
bool se_conv3d_wino44pp_layout_ok(int cin, int flags);
bool se_conv3d_wino44pp_fits(int batch, int dim, int cout);
int se_conv3d_wino44pp_form(const ConvArgs& a);
int se_conv3d_wino44pp_launch(const ConvArgs& a, int batch, int form, hipStream_t s);
// conv3d_wino2d.hip
bool se_conv3d_wino2d_fits(int batch, int dim, int cout);
int se_conv3d_wino2d_form(const ConvArgs& a);
int se_conv3d_wino2d_launch(const ConvArgs& a, int batch, int form, int exp, hipStream_t s);
// conv3d_wino.hip: the 1-D Winograd kernels; `kernel` is the plan's (SE_CONV_WINO43PP_1D, SE_CONV_K7_*).  _fits: the unit table of
// `kernel` holds a launch of `batch` samples
bool se_conv3d_wino1d_fits(int kernel, int batch, int dim, int cout, int num_cus);
int se_conv3d_wino1d_launch(const ConvArgs& a, int batch, int kernel, hipStream_t s);
int se_conv3d_k7_wino_launch(const ConvArgs& a, int batch, int kernel, hipStream_t s);
// conv3d_wino67.hip, conv3d_wino47.hip (one translation unit per input layout, the same unit table)
bool se_conv3d_k7_wino67_fits(const ConvArgs& a, int batch, int num_cus);
int se_conv3d_k7_wino67_launch(const ConvArgs& a, int batch, int num_cus, hipStream_t s, unsigned long long* dbg);
bool se_conv3d_k7_wino47_fits(int batch, int dim, int num_cus);
int se_conv3d_k7_wino47_launch_cl(const ConvArgs& a, int batch, int num_cus, hipStream_t s, unsigned long long* dbg);
int se_conv3d_k7_wino47_launch_p3(const ConvArgs& a, int batch, int num_cus, hipStream_t s, unsigned long long* dbg);
// conv3d_tiled.hip: SE_CONV_TILED_K3 / _K7 (development builds: SE_CONV_DEV_TILED_K3_TZ too)
int se_conv3d_tiled_launch(const ConvArgs& a, int batch, int kernel, int form, hipStream_t s);
// conv3d_small.hip: SE_CONV_HALO64 / _HALO64_S6 / _WAVESPLIT / _SPLITK_GRID, on the whole batch; reads p.kernel, p.form and p.splits
// _s6_domain: what conv3d_k3_halo64_s6_kernel can run at all (whole 64-voxel tiles of rows, 32-channel stages of input and split
// planes, cout tile pairs, 32-bit byte offsets into the input); when it is the faster kernel is the plan's to say
inline bool se_conv3d_halo64_s6_domain(const ConvArgs& a) {
    return (a.dim == 8 || a.dim == 16) && a.cin > 0 && (a.cin & 31) == 0 && (a.cin_pad & 31) == 0 && a.nts > 0 && a.nts % 2 == 0 && a.cout == a.nts * 16 &&
           a.total_vox > 0 && a.total_vox <= 8192 && a.total_vox * a.cin_pad * 4LL < (1LL << 31);
}
int se_conv3d_small_launch(const ConvArgs& a, const SeConvPlan& p, hipStream_t s);
// conv3d_direct.hip: SE_CONV_DIRECT, on the whole batch
int se_conv3d_direct_launch(const ConvArgs& a, int ksize, hipStream_t s);
