// The packed-weight format of the float32 3D convolutions (se_conv3d_pack_f32): which sections a layer's buffer has, where each
// starts, and the value of every element of every section.  Plain C++ (host and device, no HIP header): conv3d_pack.hip writes the
// buffer with one trivial kernel per section, tests/cpp/conv3d_pack_check.cpp compiles this header with g++ and evaluates the same
// functions on the host.  Nothing outside this header computes a section's start or size, or decodes an element index.
#pragma once
#include <math.h>
#include <stddef.h>

#include "wino47_matrices.h"
#include "wino67_matrices.h"

#if defined(__HIPCC__)
#define SE_PACK_FN __host__ __device__ inline
#else
#define SE_PACK_FN inline
#endif

// 7x7x7 tiled kernel: the 343 taps are taken 4 at a time on the MFMA k lanes -> 86 groups (last one has 1 pad tap)
#define SE_K7_TAPS 343
#define SE_K7_GROUPS 86
// 1-D Winograd F(4,3) section (E) of the packed 3x3x3 weights: 9 (dy,dx) x 6 xi x 2 cout tiles x 1 KiB = 108 KB per (16-cin group, 32-cout block)
#define SE_WINO43_CHUNK_FLOATS (9 * 6 * 2 * 256)
// 2-D Winograd F(4,3) x F(2,3) section (G) of the packed 3x3x3 weights (conv3d_wino2d.hip): per (32-cout block, 8-cin chunk)
// 24 xi x 3 dx x 2 cout tiles x 64 lanes x 2 = 73,728 B
#define SE_WINO2D_CHUNK_FLOATS (24 * 3 * 2 * 128)
// 2-D Winograd F(4,3) x F(4,3) section (I) of the packed 3x3x3 weights (conv3d_wino44pp.hip): per (32-cout block, 4-cin chunk)
// 9 xi quads x 3 dx x 2 cout tiles x 64 lanes x 4 = 55,296 B
#define SE_WINO44_CHUNK_FLOATS (9 * 3 * 2 * 256)
// 1-D Winograd F(4,7) section (F) of the packed 7x7x7 weights: per 3-channel chunk 13 (dy,dx) tap groups (the 49 taps 4 at a time on
// the MFMA k lanes) x 10 xi x 64 lanes x 3
#define SE_K7W_GROUPS 13
#define SE_K7F_XI 10
#define SE_K7F_CHUNK_FLOATS (SE_K7W_GROUPS * SE_K7F_XI * 64 * 3)
// 1-D Winograd F(6,7) section (H) of the packed 7x7x7 weights (conv3d_wino67.hip): per 3-channel chunk the 147 (channel, dy, dx)
// taps 4 at a time on the k lanes = 37 groups x 64 lanes x 12 xi
#define SE_K7H_GROUPS 37
#define SE_K7H_CHUNK_FLOATS (SE_K7H_GROUPS * 64 * 12)

SE_PACK_FN int round_up16(int v) { return (v + 15) & ~15; }

// The packed-weight buffer of one layer (se_conv3d_pack_f32): which sections it has, where each starts (in floats; -1: absent), how
// many floats it holds (0: absent) and the buffer's total size.  The ONE place that states a section's size and the condition under
// which it exists: se_conv3d_packed_elems returns `total`, the packer writes every section at these offsets, the launcher points
// ConvArgs::wpack_* at them.
//   A  every layer:        direct form                      [cg][tap][nt][lane][4]
//   B  k = 7:              tap-lane form of the tiled kernel [chunk4][group 86][nt][lane][4]
//   E  k = 3, cout % 32 == 0: 1-D Winograd F(4,3)
//   F  k = 7, cout <= 16:  1-D Winograd F(4,7)               [chunk3][g13][xi10][lane][3]
//   G  k = 3, cout % 32 == 0: 2-D Winograd F(4,3) x F(2,3)
//   H  k = 7, cout <= 16:  1-D Winograd F(6,7)               [chunk3][g37][lane][xi12]
//   I  k = 3, cout % 32 == 0: 2-D Winograd F(4,3) x F(4,3)
// (The letters C and D belonged to the F(2,3) and F(2,7) forms, which no kernel reads any more.)
// Buffer order: A B F H (k = 7), A E G I (k = 3), A alone (k = 1, transposed k = 2).
enum SePackSection { SE_PACK_A, SE_PACK_B, SE_PACK_E, SE_PACK_F, SE_PACK_G, SE_PACK_H, SE_PACK_I, SE_PACK_SECTIONS };
struct SePackLayout {
    long long at[SE_PACK_SECTIONS], elems[SE_PACK_SECTIONS], total;
    const float* section(const float* wpack, int s) const { return at[s] >= 0 ? wpack + at[s] : nullptr; }
};
inline SePackLayout se_conv3d_pack_layout(int cout, int cin_pad, int ksize, int transposed) {
    const long long nts = round_up16(cout) / 16, cb = cout / 32, taps = transposed ? 8 : (long long)ksize * ksize * ksize;
    const bool k7 = !transposed && ksize == 7, k7w = k7 && cout <= 16, k3w = !transposed && ksize == 3 && cout % 32 == 0;
    SePackLayout l;
    l.total = 0;
    auto section = [&l](int s, bool present, long long elems) {
        l.at[s] = present ? l.total : -1LL;
        l.elems[s] = present ? elems : 0LL;
        l.total += l.elems[s];
    };
    section(SE_PACK_A, true, taps * (cin_pad / 16) * nts * 256);
    section(SE_PACK_B, k7, (long long)(cin_pad / 4) * SE_K7_GROUPS * nts * 256);
    section(SE_PACK_E, k3w, (cin_pad / 16) * cb * SE_WINO43_CHUNK_FLOATS);
    section(SE_PACK_F, k7w, (long long)((cin_pad + 2) / 3) * SE_K7F_CHUNK_FLOATS);
    section(SE_PACK_G, k3w, (cin_pad / 8) * cb * SE_WINO2D_CHUNK_FLOATS);
    section(SE_PACK_H, k7w, (long long)((cin_pad + 2) / 3) * SE_K7H_CHUNK_FLOATS);
    section(SE_PACK_I, k3w, (cin_pad / 4) * cb * SE_WINO44_CHUNK_FLOATS);
    return l;
}

// What a layer is packed from: the convolution's weights [cout][cin][k^3] (transposed: [cin][cout][8]) and, with BatchNorm, the
// gamma and running variance its scale is folded from (both NULL without).
struct SePackSource {
    const float* w;
    const float* gamma;
    const float* var;
    float eps;
    int cout, cin, cin_pad, ksize, transposed;
};

// scale = gamma / sqrt(var + eps)    (identity without BN)
SE_PACK_FN float se_pack_scale(const SePackSource& s, int co) { return s.gamma ? s.gamma[co] / sqrtf(s.var[co] + s.eps) : 1.f; }

//   bpack[cout] = (b - mean) * scale + beta,  scale = gamma / sqrt(var + eps)    (identity without BN)
SE_PACK_FN float se_pack_bias(const SePackSource& s, const float* b, const float* beta, const float* mean, int t) {
    float v = 0.f;
    if (t < s.cout) {
        const float sc = se_pack_scale(s, t);
        const float b0 = b ? b[t] : 0.f;
        v = s.gamma ? (b0 - mean[t]) * sc + beta[t] : b0;
    }
    return v;
}

// G of F(4,3), points {0, 1, -1, 2, -2, inf}; G of F(2,3)
static constexpr float SE_W43_G[6][3] = {{0.25f, 0.f, 0.f},          {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                                         {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0.f, 0.f, 1.f}};
static constexpr float SE_W23_G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};

// ------------------------------------------------------------------------------------------------
// The value of element t of each section (t counts from the section's start).
//   section A: wpack[cg][tap][nt][lane][j] = W[cout = 16*nt + (lane&15)][cin = 16*cg + 4*(lane>>4) + j][tap] * scale[cout]
//   section B (k = 7 only, read by the LDS-tiled 7x7x7 kernel: 4-channel chunks, 4 taps on the MFMA k lanes):
//              wpack[A + [ch][g][nt][lane][j]] = W[cout][cin = 4*ch + j][tap = 4*g + (lane>>4)] * scale[cout]
// ------------------------------------------------------------------------------------------------
// sections A and B: one weight of the layer, or zero padding (channels >= cin, couts >= cout, tap 343 of section B)
SE_PACK_FN float se_pack_weight(const SePackSource& s, int co, int ci, int tap, int taps) {
    float v = 0.f;
    if (co < s.cout && ci < s.cin && tap < taps) {
        const float sc = se_pack_scale(s, co);
        const float wv = s.transposed ? s.w[((size_t)ci * s.cout + co) * taps + tap] : s.w[((size_t)co * s.cin + ci) * taps + tap];
        v = wv * sc;
    }
    return v;
}
SE_PACK_FN float se_pack_a(const SePackSource& s, long long t) {
    const int nts = round_up16(s.cout) / 16, taps = s.transposed ? 8 : s.ksize * s.ksize * s.ksize;
    const int j = (int)(t & 3);
    const int lane = (int)((t >> 2) & 63);
    long long r = t >> 8;
    const int nt = (int)(r % nts); r /= nts;
    const int tap = (int)(r % taps); r /= taps;
    const int ci = (int)r * 16 + 4 * (lane >> 4) + j;
    return se_pack_weight(s, nt * 16 + (lane & 15), ci, tap, taps);
}
SE_PACK_FN float se_pack_b(const SePackSource& s, long long t) {
    const int nts = round_up16(s.cout) / 16;
    const int j = (int)(t & 3);
    const int lane = (int)((t >> 2) & 63);
    long long r = t >> 8;
    const int nt = (int)(r % nts); r /= nts;
    const int g = (int)(r % SE_K7_GROUPS); r /= SE_K7_GROUPS;
    const int tap = 4 * g + (lane >> 4);
    const int ci = (int)r * 4 + j;
    return se_pack_weight(s, nt * 16 + (lane & 15), ci, tap, SE_K7_TAPS);
}

// section E: 1-D Winograd F(4,3) along z, U = G g with G = [[1/4,0,0],[-1/6,-1/6,-1/6],[-1/6,1/6,-1/6],
// [1/24,1/12,1/6],[1/24,-1/12,1/6],[0,0,1]]; blocks [cg][cb][tap2d(9)][xi(6)][nt2][lane][j]
SE_PACK_FN float se_pack_e(const SePackSource& s, long long t) {
    const int nts = round_up16(s.cout) / 16;
    const int j = (int)(t & 3);
    const int lane = (int)((t >> 2) & 63);
    long long r = t >> 8;
    const int nt2 = (int)(r % 2); r /= 2;
    const int xi = (int)(r % 6); r /= 6;
    const int tap2d = (int)(r % 9); r /= 9;
    const int n_cb = nts / 2;
    const int cb = (int)(r % n_cb); r /= n_cb;
    const int co = cb * 32 + nt2 * 16 + (lane & 15);
    const int cc = (int)r * 16 + 4 * (lane >> 4) + j;
    float v = 0.f;
    if (co < s.cout && cc < s.cin) {
        const float sc = se_pack_scale(s, co);
        const float* wp = s.w + ((size_t)co * s.cin + cc) * 27 + tap2d;
        const float g0 = wp[0], g1 = wp[9], g2 = wp[18];
        float u;
        switch (xi) {
            case 0: u = g0 * 0.25f; break;
            case 1: u = -(g0 + g1 + g2) * (1.f / 6.f); break;
            case 2: u = -(g0 - g1 + g2) * (1.f / 6.f); break;
            case 3: u = g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f); break;
            case 4: u = g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f); break;
            default: u = g2; break;
        }
        v = u * sc;
    }
    return v;
}

// Section F (k = 7, cout <= 16): 1-D Winograd F(4,7) along z.  U_xi = sum_kz G[xi][kz] * W[..][kz][dy][dx] (G: wino47_matrices.h).
// Per 3-channel chunk and (dy,dx) tap group g (k lane h carries tap 4g+h; taps >= 49 are zero padding) the 10 xi are stored as
// two quads and a tail so that a lane reads 4 xi x 3 channels = 48 B with three ds_read_b128:
//   [chunk3][g(13)] { Q0 [lane][xi 0..3][j] , Q1 [lane][xi 4..7][j] , T [lane][xi 8..9][j] }   (768 + 768 + 384 floats)
SE_PACK_FN float se_pack_f(const SePackSource& s, long long t) {
    const int chunk = (int)(t / SE_K7F_CHUNK_FLOATS);
    int r = (int)(t - (long long)chunk * SE_K7F_CHUNK_FLOATS);
    const int g = r / 1920;
    r -= g * 1920;
    int lane, xi, j;
    if (r < 1536) {
        const int q = r / 768, rr = r - q * 768;
        lane = rr / 12;
        const int e = rr - lane * 12;
        xi = 4 * q + e / 3;
        j = e % 3;
    } else {
        const int rr = r - 1536;
        lane = rr / 6;
        const int e = rr - lane * 6;
        xi = 8 + e / 3;
        j = e % 3;
    }
    const int tap2d = 4 * g + (lane >> 4);
    const int cc = chunk * 3 + j;
    const int co = lane & 15;
    float v = 0.f;
    if (co < s.cout && cc < s.cin && tap2d < 49) {
        const float sc = se_pack_scale(s, co);
        const float* wp = s.w + ((size_t)co * s.cin + cc) * 343 + tap2d;
        float u = 0.f;
#pragma unroll
        for (int kz = 0; kz < 7; ++kz) u += SE_W47_G[xi][kz] * wp[kz * 49];
        v = u * sc;
    }
    return v;
}

// Section G of the packed 3x3x3 weights: per (32-cout block cb, 8-channel chunk)
//   [xi_z 6][q 2][dx 3][ct 2][lane 64][e 2][c 2] = U[xi_z][xi_y = 2q + e][dx] of cout cb*32 + ct*16 + (lane & 15),
//   cin chunk*8 + 2*(lane >> 4) + c;  U = (G43 (x) G23) g over (dz, dy), times the folded BatchNorm scale.
SE_PACK_FN float se_pack_g(const SePackSource& s, long long t) {
    const int e = (int)(t & 1);                 // channel of the k lane's pair
    const int exi = (int)((t >> 1) & 1);        // xi_y inside the pair
    const int lane = (int)((t >> 2) & 63);
    long long r = t >> 8;
    const int ct = (int)(r % 2); r /= 2;
    const int dx = (int)(r % 3); r /= 3;
    const int xy = (int)(r % 2) * 2 + exi; r /= 2;
    const int xz = (int)(r % 6); r /= 6;
    const int chunks = s.cin_pad / 8;
    const int chunk = (int)(r % chunks);
    const int cb = (int)(r / chunks);
    const int co = cb * 32 + ct * 16 + (lane & 15);
    const int ci = chunk * 8 + 2 * (lane >> 4) + e;
    float v = 0.f;
    if (co < s.cout && ci < s.cin) {
        const float sc = se_pack_scale(s, co);
        const float* wp = s.w + ((size_t)co * s.cin + ci) * 27 + dx;
        double u = 0.0;
#pragma unroll
        for (int kz = 0; kz < 3; ++kz)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) u += (double)SE_W43_G[xz][kz] * (double)SE_W23_G[xy][ky] * (double)wp[kz * 9 + ky * 3];
        v = (float)(u * (double)sc);
    }
    return v;
}

// Section H (k = 7, cout <= 16): 1-D Winograd F(6,7) along z for conv3d_wino67.hip.  U_xi = sum_kz G[xi][kz] * W[..][kz][dy][dx]
// (G: wino67_matrices.h).  Per 3-channel chunk the 147 (channel, dy, dx) taps are taken 4 at a time on the MFMA k lanes: k lane h of
// group g carries slot 4g+h = (channel * 49 + dy * 7 + dx), slot 147 is zero padding; a lane's 12 xi are 48 contiguous bytes:
//   [chunk3][g(37)][lane][xi 0..11]
SE_PACK_FN float se_pack_h(const SePackSource& s, long long t) {
    const int chunk = (int)(t / SE_K7H_CHUNK_FLOATS);
    int r = (int)(t - (long long)chunk * SE_K7H_CHUNK_FLOATS);
    const int g = r / 768;
    r -= g * 768;
    const int lane = r / 12, xi = r - lane * 12;
    const int slot = 4 * g + (lane >> 4);
    const int cl = slot / 49, tap2d = slot - cl * 49;
    const int cc = chunk * 3 + cl;
    const int co = lane & 15;
    float v = 0.f;
    if (co < s.cout && cc < s.cin && slot < 147) {
        const float sc = se_pack_scale(s, co);
        const float* wp = s.w + ((size_t)co * s.cin + cc) * 343 + tap2d;
        float u = 0.f;
#pragma unroll
        for (int kz = 0; kz < 7; ++kz) u += SE_W67_G[xi][kz] * wp[kz * 49];
        v = u * sc;
    }
    return v;
}

// Section I of the packed 3x3x3 weights: per (32-cout block cb, 4-channel chunk)
//   [q 9][dx 3][ct 2][lane 64][j 4] = U[xi = 4 q + j][dx] of cout cb*32 + ct*16 + (lane & 15), cin chunk*4 + (lane >> 4);
//   xi = 6 xi_y + xi_z;  U = (G43 (x) G43) g over (dz, dy), times the folded BatchNorm scale.
SE_PACK_FN float se_pack_i(const SePackSource& s, long long t) {
    const int j = (int)(t & 3);
    const int lane = (int)((t >> 2) & 63);
    long long r = t >> 8;
    const int ct = (int)(r % 2); r /= 2;
    const int dx = (int)(r % 3); r /= 3;
    const int q = (int)(r % 9); r /= 9;
    const int chunks = s.cin_pad / 4;
    const int chunk = (int)(r % chunks);
    const int cb = (int)(r / chunks);
    const int xi = 4 * q + j, xy = xi / 6, xz = xi % 6;
    const int co = cb * 32 + ct * 16 + (lane & 15);
    const int ci = chunk * 4 + (lane >> 4);
    float v = 0.f;
    if (co < s.cout && ci < s.cin) {
        const float sc = se_pack_scale(s, co);
        const float* wp = s.w + ((size_t)co * s.cin + ci) * 27 + dx;
        double u = 0.0;
#pragma unroll
        for (int kz = 0; kz < 3; ++kz)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) u += (double)SE_W43_G[xz][kz] * (double)SE_W43_G[xy][ky] * (double)wp[kz * 9 + ky * 3];
        v = (float)(u * (double)sc);
    }
    return v;
}

// ------------------------------------------------------------------------------------------------
// The split planes of a layer (se_conv3d_split6_pack; read by the six-product bf16 forms, split6.h): a buffer of its own beside
// the float32 one, bf16 elements.  Every folded float32 weight v of section A (se_pack_weight: the same value, bit for bit) is
// stored as three bf16 values p + q + r, p = bf16(v), q = bf16(v - p), r = bf16(v - p - q), round to nearest even; the
// subtractions are exact in float32 and |v - p - q - r| <= 2^-27 |v|.  A-fragment order of v_mfma_f32_16x16x32_bf16:
//   [sg = cin_pad / 32][tap][nt][plane 3][lane 64][j 8] = plane of W[cout = 16 nt + (lane & 15)][cin = 32 sg + 8 (lane >> 4) + j][tap]
// taps = k^3 (transposed k = 2: the 8 output parities).  Exists for cin_pad % 32 == 0; -1 otherwise.
// ------------------------------------------------------------------------------------------------
SE_PACK_FN long long se_split6_packed_elems(int cout, int cin_pad, int ksize, int transposed) {
    if (cout <= 0 || cin_pad <= 0 || (cin_pad & 31)) return -1;
    if (transposed ? (ksize != 2) : (ksize != 1 && ksize != 3 && ksize != 7)) return -1;
    const long long taps = transposed ? 8 : (long long)ksize * ksize * ksize;
    return taps * (cin_pad / 32) * (round_up16(cout) / 16) * 3 * 512;
}
// float32 -> bf16 bits, round to nearest even (finite values: what v_cvt_pk_bf16_f32 gives); and back
SE_PACK_FN unsigned short se_bf16_rne_bits(float f) {
    unsigned u;
    __builtin_memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
SE_PACK_FN float se_bf16_bits_value(unsigned short h) {
    const unsigned u = (unsigned)h << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// element t of the split planes, from section A of the layer's packed float32 buffer (the folded weights are read, not recomputed:
// the planes sum to the very value the float32 kernels multiply with)
SE_PACK_FN unsigned short se_split6_value(const float* section_a, int cout, int ksize, int transposed, long long t) {
    const int nts = round_up16(cout) / 16, taps = transposed ? 8 : ksize * ksize * ksize;
    const int j = (int)(t & 7);
    const int lane = (int)((t >> 3) & 63);
    long long r = t >> 9;
    const int plane = (int)(r % 3); r /= 3;
    const int nt = (int)(r % nts); r /= nts;
    const int tap = (int)(r % taps); r /= taps;
    const int ci = (int)r * 32 + 8 * (lane >> 4) + j;
    const int lane_a = ((ci & 15) >> 2) * 16 + (lane & 15);
    float v = section_a[((((long long)(ci >> 4) * taps + tap) * nts + nt) * 64 + lane_a) * 4 + (ci & 3)];
    unsigned short h = se_bf16_rne_bits(v);
    for (int p = 0; p < plane; ++p) {
        v -= se_bf16_bits_value(h);
        h = se_bf16_rne_bits(v);
    }
    return h;
}

SE_PACK_FN float se_pack_value(int section, const SePackSource& s, long long t) {
    switch (section) {
        case SE_PACK_A: return se_pack_a(s, t);
        case SE_PACK_B: return se_pack_b(s, t);
        case SE_PACK_E: return se_pack_e(s, t);
        case SE_PACK_F: return se_pack_f(s, t);
        case SE_PACK_G: return se_pack_g(s, t);
        case SE_PACK_H: return se_pack_h(s, t);
        default: return se_pack_i(s, t);
    }
}
