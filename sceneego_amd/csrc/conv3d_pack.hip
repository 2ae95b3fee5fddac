// Weight packer of the float32 3D convolutions (+ BatchNorm fold): writes the buffer conv3d_pack.h describes, one launch per
// section that the layer has plus one for the bias.  Runs once per layer when a model is compiled, never on the hot path.
#include "common.h"

#include "conv_common.h"

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
    pack_section_kernel<SE_PACK_A>, pack_section_kernel<SE_PACK_B>, pack_section_kernel<SE_PACK_C>,
    pack_section_kernel<SE_PACK_D>, pack_section_kernel<SE_PACK_E>, pack_section_kernel<SE_PACK_F>,
    pack_section_kernel<SE_PACK_G>, pack_section_kernel<SE_PACK_H>, pack_section_kernel<SE_PACK_I>};

}  // namespace

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
