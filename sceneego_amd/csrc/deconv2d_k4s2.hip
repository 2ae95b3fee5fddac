// ConvTranspose2d(k = 4, stride 2, padding 1) + bias (+ ReLU) of the 2-D pose head (network/pose_resnet.py:205-224, run at :238) as
// ONE launch: float32 NCHW in, float32 NCHW out, every float32 product taken as six bf16 products on v_mfma_f32_16x16x32_bf16
// (split6.h: x = a + b + c, w = p + q + r, products ap aq bp ar cp bq; float32 accuracy at the bf16 pipe's rate).
//
// Four-phase implicit GEMM.  Output pixel (2j + a, 2i + b) sums 2 x 2 taps over the input rows j - 1 + a, j + a and columns
// i - 1 + b, i + b:  with the input at shift (sy, sx) in {-1, 0, 1}^2 from (j, i), phase a takes sy in {a - 1, a} with kernel row
// ky = 1 + a - 2 sy, phase b takes sx in {b - 1, b} with kx = 1 + b - 2 sx.
//
// A workgroup (8 waves) owns a tile of 8 rows x 16 columns of input positions of one sample (one-pixel halo: 10 x 18), all four
// phases and 64 output channels; it walks the input channels in chunks of 32 (the K of one MFMA).
//   Activations: a thread loads 8 consecutive channels of a halo pixel (8 planes of the NCHW tensor: 8 dword loads, lanes along the
//   row; outside the map the buffer offset is out of range and the load returns zero), splits them once (se_split3_x8) and writes the
//   three bf16 planes as [plane 3][octet 4][16 B] = 192 of a 224-byte record per pixel (the pitch of conv3d_k3_halo64_s6_kernel: the
//   16 lanes of a ds_read_b128 group land on 16 different 16-byte slots).  Two chunk buffers: 2 x 180 x 224 = 80,640 B of LDS; one
//   barrier per chunk.
//   Wave w: phase row a = w & 1, cout tile (w >> 1) of the block's four, BOTH column phases b, all 8 position tiles (tile = one row of
//   16 pixels): 2 x 8 accumulators (64 registers).  Per chunk it walks its 6 shifts (sy in {a - 1, a} x sx); a shift's activation
//   fragments feed the phase b = 0 (sx = -1, 0) and b = 1 (sx = 0, 1) products: 8 (phase, tap) products per 6 shifts.
//   Weights arrive pre-split in A-fragment order (se_deconv2d_k4s2_s6_pack), in the order the wave walks them; each wave loads only
//   its own (a, cout tile) fragments, so no fragment is loaded twice by a workgroup: 8 fragments x 3 KB per chunk and wave, two shifts
//   in flight in a register ring.
//   Products in the order of SE_S6_W / SE_S6_X, product loop outermost over the accumulators.
//   Epilogue: a lane holds both b phases of (cout, position): one 8-byte store; 16 lanes = 128 contiguous bytes of an output row.
// Budget per wave and chunk: 8 x 8 x 6 = 384 MFMAs against 6 shifts x 8 tiles x 3 = 144 ds_read_b128 (0.375 reads per MFMA; the LDS
// serves one 1 KB wave-read per MFMA slot and SIMD) and 24 x 1 KB of weights.  L2 bytes per launch: every workgroup streams the split
// weights of its 64 couts once, cin / 32 x 192 KB; at 256 -> 256 channels and 8 x 32 x 32 positions that is 256 workgroups x 1.5 MB =
// 393 MB of weights (+ 4 x 8.4 MB x 180 / 128 of activations).
// No atomics and a fixed summation order (chunks, then shifts, then products): launches are bit-identical, and a sample's result does
// not depend on the batch it is in (a tile never crosses a sample).
#include "common.h"

#include "conv3d_pack.h"
#include "split6.h"

namespace {

constexpr int DC_TR = 8, DC_TC = 16;                  // tile: rows x columns of input positions
constexpr int DC_HR = DC_TR + 2, DC_HC = DC_TC + 2;   // with the halo
constexpr int DC_HV = DC_HR * DC_HC;                  // 180 halo pixels
constexpr int DC_PITCH = 224;
constexpr int DC_HB = DC_HV * DC_PITCH;               // one chunk buffer
constexpr int DC_PIECES = DC_HV * 4;                  // (pixel, channel octet) pieces of a chunk: 720
constexpr int DC_HP = (DC_PIECES + 511) / 512;
constexpr int DC_LDS_BYTES = 2 * DC_HB;
constexpr int DC_COUT_BLOCK = 64;
constexpr int DC_WAVE_CHUNK_BYTES = 8 * 3 * 1024;     // the 8 fragments of one (chunk, cout tile, phase row)
static_assert(DC_LDS_BYTES <= 160 * 1024, "two chunk buffers in LDS");

// Element t of the split planes:  [chunk = cin / 32][cout tile][a 2][fragment 8][plane 3][lane 64][j 8]
//   fragment = 4 dy + f: input row shift sy = a - 1 + dy (ky = 3 - a - 2 dy); f = 0: (sx -1, b 0), 1: (sx 0, b 0), 2: (sx 0, b 1),
//   3: (sx +1, b 1) (kx = 1 + b - 2 sx);  value = plane of w[cin = 32 chunk + 8 (lane >> 4) + j][cout = 16 tile + (lane & 15)][ky][kx]
__host__ __device__ inline void se_deconv_s6_decode(long long t, int nts, int& ci, int& co, int& ky, int& kx, int& plane) {
    const int j = (int)(t & 7);
    const int lane = (int)((t >> 3) & 63);
    long long r = t >> 9;
    plane = (int)(r % 3); r /= 3;
    const int frag = (int)(r & 7); r >>= 3;
    const int a = (int)(r & 1); r >>= 1;
    const int ct = (int)(r % nts);
    const int sg = (int)(r / nts);
    const int dy = frag >> 2, f = frag & 3;
    const int sx = (f + 1) / 2 - 1, b = f >> 1;
    ky = 3 - a - 2 * dy;
    kx = 1 + b - 2 * sx;
    ci = sg * 32 + 8 * (lane >> 4) + j;
    co = ct * 16 + (lane & 15);
}

__global__ void deconv_s6_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int cout, long long n) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    int ci, co, ky, kx, plane;
    se_deconv_s6_decode(t, cout / 16, ci, co, ky, kx, plane);
    float v = w[(((long long)ci * cout + co) * 4 + ky) * 4 + kx];
    unsigned short h = se_bf16_rne_bits(v);
    for (int p = 0; p < plane; ++p) {
        v -= se_bf16_bits_value(h);
        h = se_bf16_rne_bits(v);
    }
    out[t] = h;
}

struct DeconvArgs {
    const float* x;
    const unsigned short* wsplit;
    const float* bias;
    float* out;
    int batch, cin, cout, h, w, relu;
};

__global__ __launch_bounds__(512) void deconv2d_k4s2_s6_kernel(DeconvArgs a) {
    constexpr int HC = DC_HC, PITCH = DC_PITCH, HP = DC_HP;
    typedef float f32x2s __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int vl = lane & 15, h = lane >> 4;
    const int pa = wave & 1;                              // phase row a
    const int ct = blockIdx.y * 4 + (wave >> 1);          // cout tile
    const int nts = a.cout >> 4;
    const int stages = a.cin >> 5;
    constexpr unsigned OOB = 0x80000000u;
    int t = blockIdx.x;
    const int tx = t % (a.w / DC_TC); t /= (a.w / DC_TC);
    const int ty = t % (a.h / DC_TR);
    const int b = t / (a.h / DC_TR);
    const int y0 = ty * DC_TR, x0 = tx * DC_TC;
    const unsigned plane_bytes = (unsigned)(a.h * a.w * 4);

    // this thread's halo pieces (pixel hv, channel octet q): byte offset of channel 8 q of the chunk, out of range outside the map
    unsigned goff[HP];
    int lpiece[HP];
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        const int p = tid + 512 * j;
        const int q = p / DC_HV, hv = p - q * DC_HV;
        const int hy = hv / HC, hx = hv - hy * HC;
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        const bool ok = p < DC_PIECES && (unsigned)gy < (unsigned)a.h && (unsigned)gx < (unsigned)a.w;
        goff[j] = ok ? (unsigned)(((b * a.cin + q * 8) * a.h + gy) * a.w + gx) * 4u : OOB;      // launcher: the tensor fits 31 bits
        lpiece[j] = hv * PITCH + q * 16;                                                         // plane k: + 64 k
    }
    const unsigned in_bytes = (unsigned)a.batch * (unsigned)a.cin * plane_bytes;
    const unsigned w_bytes = (unsigned)(stages * nts * 2 * DC_WAVE_CHUNK_BYTES);
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)in_bytes, 0x00020000);
    const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.wsplit), 0, (int)w_bytes, 0x00020000);
    const int woff = lane * 16;
    // operand reads: lane (vl, h) = pixel vl of a tile row, channels 8 h .. 8 h + 7 of the chunk, at shift (sy, sx) = (pa - 1, -1)
    const int lbase = (pa * HC + vl) * PITCH + h * 16;

    float st[HP][8];
    auto load_stage = [&](int sg) {
#pragma unroll
        for (int j = 0; j < HP; ++j)
#pragma unroll
            for (int c = 0; c < 8; ++c)
                st[j][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, (int)goff[j], (int)((sg * 32 + c) * plane_bytes), 0));
    };
    auto commit_stage = [&](unsigned char* buf) {
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            const Split6Frag f = se_split3_x8((f32x4){st[j][0], st[j][1], st[j][2], st[j][3]}, (f32x4){st[j][4], st[j][5], st[j][6], st[j][7]});
            if (tid + 512 * j < DC_PIECES) {
#pragma unroll
                for (int k = 0; k < 3; ++k) *reinterpret_cast<u16x8*>(buf + lpiece[j] + k * 64) = f.p[k];
            }
        }
    };
    // step s = 3 dy + sxi of a chunk (sx = sxi - 1): fragments 4 dy + {0}, {1, 2}, {3}
    Split6Frag wr[2][2];
    auto load_w = [&](Split6Frag (&w)[2], int s, int sg) {
        const int dy = s / 3, sxi = s % 3;
        const int f0 = 4 * dy + (sxi == 0 ? 0 : sxi == 1 ? 1 : 3);
        const int wso = ((sg * nts + ct) * 2 + pa) * DC_WAVE_CHUNK_BYTES + f0 * 3072;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            if (m == 0 || sxi == 1) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    w[m].p[k] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, woff, wso + (m * 3 + k) * 1024, 0));
            }
        }
    };
    f32x4 acc[2][DC_TR];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < DC_TR; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    load_stage(0);
    load_w(wr[0], 0, 0);
    load_w(wr[1], 1, 0);
    for (int sg = 0; sg < stages; ++sg) {
        unsigned char* buf = lds + (sg & 1) * DC_HB;
        commit_stage(buf);
        __syncthreads();          // the chunk is in LDS; every wave has left the chunk before the previous one (the buffer written next)
        const bool more = sg + 1 < stages;
        if (more) load_stage(sg + 1);
        // half step hs = 2 s + nh: step s = 3 dy + sxi on the position tiles 4 nh .. 4 nh + 3; its 12 fragment reads are issued one half
        // step ahead, into the other register set
        Split6Frag x[2][4];
        auto load_x = [&](Split6Frag (&xf)[4], int hs) {
            const int s = hs >> 1, nh = hs & 1;
            const unsigned char* p = buf + lbase + ((s / 3 + nh * 4) * HC + s % 3) * PITCH;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int k = 0; k < 3; ++k) xf[n].p[k] = *reinterpret_cast<const u16x8*>(p + n * HC * PITCH + k * 64);
        };
        load_x(x[0], 0);
#pragma unroll
        for (int hs = 0; hs < 12; ++hs) {
            const int s = hs >> 1, nh = hs & 1, sxi = s % 3;
            const Split6Frag(&w)[2] = wr[s & 1];
            const Split6Frag(&xf)[4] = x[hs & 1];
            if (hs + 1 < 12) load_x(x[(hs + 1) & 1], hs + 1);
            __builtin_amdgcn_sched_barrier(0);         // ... and are issued ahead of this half step's MFMAs, not sunk behind them
#pragma unroll
            for (int k = 0; k < SE_S6_PRODUCTS; ++k)   // product outer: consecutive MFMAs go to different accumulators
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    if (sxi != 2) acc[0][nh * 4 + n] = mfma_bf16(w[0].p[SE_S6_W[k]], xf[n].p[SE_S6_X[k]], acc[0][nh * 4 + n]);
                    if (sxi != 0) acc[1][nh * 4 + n] = mfma_bf16(w[sxi == 1 ? 1 : 0].p[SE_S6_W[k]], xf[n].p[SE_S6_X[k]], acc[1][nh * 4 + n]);
                }
            __builtin_amdgcn_sched_barrier(0);         // reads further ahead are not hoisted over these MFMAs (register budget)
            if (nh == 1) {
                // the slot's registers are free: the step two ahead (this chunk's, then the next chunk's first two)
                if (s + 2 < 6) load_w(wr[s & 1], s + 2, sg);
                else if (more) load_w(wr[s & 1], s - 4, sg + 1);
            }
        }
    }

    // lane (vl, h): couts 16 ct + 4 h .. + 3 of pixel (y0 + n, x0 + vl), output row 2 (y0 + n) + pa, columns 2 (x0 + vl), + 1
    const int co0 = ct * 16 + 4 * h;
    const f32x4 bias = *reinterpret_cast<const f32x4*>(a.bias + co0);
    const long long orow = 2LL * a.w, oplane = 2LL * a.h * orow;
    float* o = a.out + ((long long)b * a.cout + co0) * oplane + (2LL * y0 + pa) * orow + 2 * (x0 + vl);
#pragma unroll
    for (int n = 0; n < DC_TR; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            f32x2s v = {acc[0][n][r] + bias[r], acc[1][n][r] + bias[r]};
            if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); }
            *reinterpret_cast<f32x2s*>(o + r * oplane + 2 * n * orow) = v;
        }
}

}  // namespace

extern "C" int se_deconv2d_k4s2_s6_domain(int batch, int cin, int cout, int h, int w) {
    if (batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return 0;
    if ((cin & 31) || cout % DC_COUT_BLOCK || w % DC_TC || h % DC_TR) return 0;
    if ((long long)batch * cin * h * w * 4 >= (1LL << 31)) return 0;                         // 32-bit byte offsets into the input
    if ((long long)(cin / 32) * (cout / 16) * 2 * DC_WAVE_CHUNK_BYTES >= (1LL << 31)) return 0;   // ... and into the split planes
    return 1;
}

extern "C" long long se_deconv2d_k4s2_s6_packed_elems(int cin, int cout) {
    if (cin <= 0 || cout <= 0 || (cin & 31) || cout % DC_COUT_BLOCK) return -1;
    return (long long)(cin / 32) * (cout / 16) * 2 * (DC_WAVE_CHUNK_BYTES / 2);
}

extern "C" int se_deconv2d_k4s2_s6_pack(const float* w, se_bf16* wsplit, int cin, int cout, void* stream) {
    const long long n = se_deconv2d_k4s2_s6_packed_elems(cin, cout);
    if (!w || !wsplit || n <= 0) return SE_ERR_BAD_ARG;
    hipLaunchKernelGGL(deconv_s6_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, se_stream(stream), w,
                       reinterpret_cast<unsigned short*>(wsplit), cout, n);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_deconv2d_k4s2_s6_f32(const void* x, int x_elem_bytes, const se_bf16* wsplit, const float* bias, float* out, int batch,
                                       int cin, int cout, int h, int w, int relu, void* stream) {
    if (!x || !wsplit || !bias || !out || x_elem_bytes != 4 || !se_deconv2d_k4s2_s6_domain(batch, cin, cout, h, w)) return SE_ERR_BAD_ARG;
    if (!se_aligned({x}, 4) || !se_aligned({out}, 8) || !se_aligned({wsplit, bias}, 16)) return SE_ERR_BAD_ARG;
    const DeconvArgs a = {static_cast<const float*>(x), reinterpret_cast<const unsigned short*>(wsplit), bias, out, batch, cin, cout, h, w, relu};
    const dim3 grid((unsigned)(batch * (h / DC_TR) * (w / DC_TC)), (unsigned)(cout / DC_COUT_BLOCK));
    SE_ENSURE_LDS(deconv2d_k4s2_s6_kernel, DC_LDS_BYTES);
    hipLaunchKernelGGL(deconv2d_k4s2_s6_kernel, grid, dim3(512), DC_LDS_BYTES, se_stream(stream), a);
    SE_CHECK_LAUNCH();
    return 0;
}
