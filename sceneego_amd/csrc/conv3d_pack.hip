// Weight packer of the float32 3D convolutions (+ BatchNorm fold): writes the buffer conv3d_pack.h describes, one launch per
// section that the layer has plus one for the bias.  Runs once per layer when a model is compiled, never on the hot path.
#include "common.h"

#include "conv_common.h"
#include "split6.h"

namespace {

template <int S>
__global__ void pack_section_kernel(SePackSource src, float* __restrict__ out, long long at, long long n) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) out[at + t] = se_pack_value(S, src, t);
}

__global__ void pack_bias_kernel(SePackSource src, const float* __restrict__ b, const float* __restrict__ beta,
                                 const float* __restrict__ mean, float* __restrict__ bpack) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < round_up16(src.cout)) bpack[t] = se_pack_bias(src, b, beta, mean, t);
}

using PackKernel = void (*)(SePackSource, float*, long long, long long);
constexpr PackKernel PACK_KERNELS[SE_PACK_SECTIONS] = {
    pack_section_kernel<SE_PACK_A>, pack_section_kernel<SE_PACK_B>, pack_section_kernel<SE_PACK_E>, pack_section_kernel<SE_PACK_F>,
    pack_section_kernel<SE_PACK_G>, pack_section_kernel<SE_PACK_H>, pack_section_kernel<SE_PACK_I>};

// the split planes of a layer (conv3d_pack.h: se_split6_value), from section A of its packed float32 buffer
__global__ void pack_split6_kernel(const float* __restrict__ section_a, unsigned short* __restrict__ out, int cout, int ksize, int transposed,
                                   long long n) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) out[t] = se_split6_value(section_a, cout, ksize, transposed, t);
}

// test entry point: the device split of n float32 values (split6.h: se_split3_pair) -> planes [3][n] of bf16; n even
__global__ void split6_planes_kernel(const float* __restrict__ x, unsigned short* __restrict__ planes, long long n) {
    const long long t = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (t >= n) return;
    unsigned part[3];
    se_split3_pair(x[t], x[t + 1], part);
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<unsigned*>(planes + k * n + t) = part[k];
}

}  // namespace

extern "C" long long se_conv3d_split6_packed_elems(int cout, int cin_pad, int ksize, int transposed) {
    return se_split6_packed_elems(cout, cin_pad, ksize, transposed);
}

extern "C" int se_conv3d_split6_pack(const float* wpack, se_bf16* wsplit, int cout, int cin_pad, int ksize, int transposed, void* stream) {
    const long long n = se_split6_packed_elems(cout, cin_pad, ksize, transposed);
    if (!wpack || !wsplit || n <= 0) return SE_ERR_BAD_ARG;
    hipLaunchKernelGGL(pack_split6_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, se_stream(stream), wpack,
                       reinterpret_cast<unsigned short*>(wsplit), cout, ksize, transposed, n);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_split6_planes_f32(const float* x, se_bf16* planes, long long n, void* stream) {
    if (!x || !planes || n <= 0 || (n & 1)) return SE_ERR_BAD_ARG;
    hipLaunchKernelGGL(split6_planes_kernel, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, se_stream(stream), x,
                       reinterpret_cast<unsigned short*>(planes), n);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" long long se_conv3d_packed_elems(int cout, int cin_pad, int ksize, int transposed) {
    return se_conv3d_pack_layout(cout, cin_pad, ksize, transposed).total;
}

extern "C" int se_conv3d_pack_f32(const float* w, const float* b, const float* gamma, const float* beta,
                                  const float* mean, const float* var, float eps, float* wpack, float* bpack,
                                  int cout, int cin, int cin_pad, int ksize, int transposed, void* stream) {
    if (cout <= 0 || cin <= 0 || cin_pad < cin || (cin_pad & 15)) return SE_ERR_BAD_ARG;
    if (transposed ? (ksize != 2) : (ksize != 1 && ksize != 3 && ksize != 7)) return SE_ERR_BAD_ARG;
    if ((gamma != nullptr) != (beta != nullptr) || (gamma != nullptr) != (mean != nullptr) ||
        (gamma != nullptr) != (var != nullptr))
        return SE_ERR_BAD_ARG;
    const SePackLayout l = se_conv3d_pack_layout(cout, cin_pad, ksize, transposed);
    const SePackSource src = {w, gamma, var, eps, cout, cin, cin_pad, ksize, transposed};
    hipStream_t s = se_stream(stream);
    hipLaunchKernelGGL(pack_bias_kernel, dim3((unsigned)((round_up16(cout) + 255) / 256)), dim3(256), 0, s, src, b, beta, mean, bpack);
    SE_CHECK_LAUNCH();
    for (int sec = 0; sec < SE_PACK_SECTIONS; ++sec) {
        if (l.elems[sec] <= 0) continue;
        hipLaunchKernelGGL(PACK_KERNELS[sec], dim3((unsigned)((l.elems[sec] + 255) / 256)), dim3(256), 0, s, src, wpack, l.at[sec],
                           l.elems[sec]);
        SE_CHECK_LAUNCH();
    }
    return 0;
}
