// Volume renderer: a maximum-intensity projection (MIP) of the 15 per-joint probability volumes along every pixel's ray, composited
// joint by joint, in per-joint colours, over a picture render.hip made (no counterpart in the reference, whose viewer is an open3d
// window; sceneego_amd/render.py drives it: SceneRenderer.render_volumes / overlay_volumes).
//
//   se_render_volume_pack_f32     [B][15][G^3] float32 -> [B][G^3][16] float32 (slot 15 = 0): the 15 values of a cell, which lie
//                                 4 G^3 bytes apart in the network's layout, become one 64-byte line, so that a ray's visit of a cell
//                                 is four 16-byte loads of one line instead of 15 loads of 15 lines.  One thread per cell: the 15 reads
//                                 are coalesced along the plane, the writes are 64 contiguous bytes per lane.
//   se_render_volume_view_f64     one thread per output pixel, 16 x 16 pixel tiles per workgroup (a wave is a 16 x 4 patch: its rays
//   se_render_volume_overlay_f64  stay in neighbouring cells, so the lines one lane fetched serve the others out of L1 / L2).  Slab
//                                 test against the grid's box, Amanatides-Woo cell walk, 15 running maxima in registers, composite.
//
// The maximum is taken on the float32 values and multiplied by the joint's scale once, at the end: for a finite scale > 0 the
// float64 product x -> x * scale is monotone, so scale * max(x) == max(x * scale) bit for bit, which is what the header states.
// The walk itself is float64 and unfused (-ffp-contract=off), in the operation order of include/sceneego_hip.h, so that
// tests/volume_render_model.py can restate it literally.  Every cell boundary is recomputed from its index (no running sum), so the
// parameters of a long walk carry no drift.
//
// Nothing is allocated and no memset node is issued: the entry points are legal inside a hipGraph capture.
#include "common.h"

#pragma clang fp contract(off)

namespace {

#define SE_VOL_JOINTS 15
#define SE_VOL_SLOTS 16
#define SE_VOL_TILE 16

__constant__ unsigned char c_palette[SE_VOL_JOINTS][3] = SE_RENDER_VOLUME_PALETTE;
const unsigned char h_palette[SE_VOL_JOINTS][3] = SE_RENDER_VOLUME_PALETTE;

struct VolParams {
    int G;
    double h;            // S / (G - 1)
    double pos[3];       // (-S / 2, -S / 2, 0)
    double near;
    double gain, opacity;
    unsigned int mask;
};

struct View {
    double v[12];
};

// grid (ceil(G^3 / 256), B)
__global__ __launch_bounds__(256) void render_volume_pack_kernel(const float* __restrict__ vol, float* __restrict__ packed, int cells) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= cells) return;
    const size_t b = blockIdx.y;
    const float* src = vol + b * SE_VOL_JOINTS * (size_t)cells + cell;
    float v[SE_VOL_SLOTS];
#pragma unroll
    for (int j = 0; j < SE_VOL_JOINTS; ++j) v[j] = src[(size_t)j * cells];
    v[15] = 0.0f;
    f32x4* dst = reinterpret_cast<f32x4*>(packed + (b * (size_t)cells + cell) * SE_VOL_SLOTS);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 w = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        dst[q] = w;
    }
}

// boundary k (0..G) of axis a: the lower face of cell k
__device__ __forceinline__ double vol_bnd(const VolParams& P, int a, int k) { return P.pos[a] + ((double)k - 0.5) * P.h; }

__device__ __forceinline__ int vol_start(const VolParams& P, int a, double o, double d, double s0) {
    const double p = o + s0 * d;
    const double u = (p - P.pos[a]) / P.h + 0.5;
    return u >= 0.0 ? (u < (double)P.G ? (int)u : P.G - 1) : 0;       // a NaN lands in cell 0
}

__device__ __forceinline__ void vol_take(float* m, const f32x4 w, int q) {
    if (w.x > m[4 * q]) m[4 * q] = w.x;             // v > m: a NaN never wins
    if (w.y > m[4 * q + 1]) m[4 * q + 1] = w.y;
    if (w.z > m[4 * q + 2]) m[4 * q + 2] = w.z;
    if (q < 3 && w.w > m[4 * q + 3]) m[4 * q + 3] = w.w;
}

// The 15 maxima of the cells the ray o + s d visits for s in [near, limit); false when the ray misses the box or the range is empty.
// `live`: the joints whose maxima are wanted (uniform across the launch's frame); groups of four without a live joint are not read.
__device__ __forceinline__ bool vol_march(const float* __restrict__ cells, const VolParams& P, unsigned int live, double ox, double oy,
                                          double oz, double dx, double dy, double dz, double limit, float* m) {
    if (!(isfinite(dx) && isfinite(dy) && isfinite(dz)) || limit != limit) return false;
    const int G = P.G;
    const double o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
    double inv[3];
    double s0 = P.near, s1 = limit;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = vol_bnd(P, a, 0), hi = vol_bnd(P, a, G);
        if (d[a] == 0.0) {
            inv[a] = 0.0;
            if (!(o[a] >= lo && o[a] < hi)) return false;
        } else {
            inv[a] = 1.0 / d[a];
            const double ta = (lo - o[a]) * inv[a], tb = (hi - o[a]) * inv[a];
            const double tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
            if (tn > s0) s0 = tn;
            if (tf < s1) s1 = tf;
        }
    }
    if (!(s0 < s1)) return false;
    int ix = vol_start(P, 0, ox, dx, s0), iy = vol_start(P, 1, oy, dy, s0), iz = vol_start(P, 2, oz, dz, s0);
    const int stx = dx > 0.0 ? 1 : dx < 0.0 ? -1 : 0, sty = dy > 0.0 ? 1 : dy < 0.0 ? -1 : 0, stz = dz > 0.0 ? 1 : dz < 0.0 ? -1 : 0;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double tx = stx ? (vol_bnd(P, 0, ix + (stx > 0)) - ox) * inv[0] : inf;
    double ty = sty ? (vol_bnd(P, 1, iy + (sty > 0)) - oy) * inv[1] : inf;
    double tz = stz ? (vol_bnd(P, 2, iz + (stz > 0)) - oz) * inv[2] : inf;
    // every step moves one index one cell towards its face of the box: at most 3 (G - 1) steps
    for (int guard = 0; guard <= 3 * G; ++guard) {
        const f32x4* c = reinterpret_cast<const f32x4*>(cells + ((size_t)(ix * G + iy) * G + iz) * SE_VOL_SLOTS);
        if (live & 0x000fu) vol_take(m, c[0], 0);
        if (live & 0x00f0u) vol_take(m, c[1], 1);
        if (live & 0x0f00u) vol_take(m, c[2], 2);
        if (live & 0x7000u) vol_take(m, c[3], 3);
        // the nearest of the three next faces; of equal ones x before y before z
        int a = 0;
        double t = tx;
        if (ty < t) { a = 1; t = ty; }
        if (tz < t) { a = 2; t = tz; }
        if (!(t < s1)) break;                       // the next cell's entry parameter: it counts only when < s1
        if (a == 0) {
            ix += stx;
            if (ix < 0 || ix >= G) break;
            tx = (vol_bnd(P, 0, ix + (stx > 0)) - ox) * inv[0];
        } else if (a == 1) {
            iy += sty;
            if (iy < 0 || iy >= G) break;
            ty = (vol_bnd(P, 1, iy + (sty > 0)) - oy) * inv[1];
        } else {
            iz += stz;
            if (iz < 0 || iz >= G) break;
            tz = (vol_bnd(P, 2, iz + (stz > 0)) - oz) * inv[2];
        }
    }
    return true;
}

// the joints that take part: bit j of the mask set and scale[j] finite and > 0
__device__ __forceinline__ unsigned int vol_live(const double* __restrict__ scale, unsigned int mask) {
    unsigned int live = 0;
    for (int j = 0; j < SE_VOL_JOINTS; ++j) {
        const double s = scale[j];
        if (((mask >> j) & 1u) && isfinite(s) && s > 0.0) live |= 1u << j;
    }
    return live;
}

__device__ __forceinline__ void vol_composite(const unsigned char* __restrict__ base, unsigned char* __restrict__ out, const float* m,
                                              const double* __restrict__ scale, unsigned int live, bool hit, const VolParams& P) {
    double c[3] = {(double)base[0], (double)base[1], (double)base[2]};
    if (hit) {
        for (int j = 0; j < SE_VOL_JOINTS; ++j) {
            if (!((live >> j) & 1u)) continue;
            const double g = P.gain * ((double)m[j] * scale[j]);
            const double a = (g < 1.0 ? g : 1.0) * P.opacity;
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = c[k] + a * ((double)c_palette[j][k] - c[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = floor(c[k] + 0.5);
        out[k] = (unsigned char)(v >= 0.0 ? (v <= 255.0 ? (int)v : 255) : 0);      // a NaN writes 0
    }
}

// pixel of this thread in a launch of 16 x 16 tiles: grid (tiles_x * tiles_y, B)
__device__ __forceinline__ bool vol_pixel(int H, int W, int* y, int* x) {
    const int tiles_x = (W + SE_VOL_TILE - 1) / SE_VOL_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    *y = ty * SE_VOL_TILE + (int)(threadIdx.x >> 4);
    *x = tx * SE_VOL_TILE + (int)(threadIdx.x & 15);
    return *y < H && *x < W;
}

__global__ __launch_bounds__(256) void render_volume_view_kernel(const float* __restrict__ packed, const double* __restrict__ scale,
                                                                 const double* __restrict__ rays, View view,
                                                                 const unsigned long long* __restrict__ zbuf,
                                                                 const unsigned char* base, unsigned char* out, int H, int W, VolParams P) {
    int y, x;
    if (!vol_pixel(H, W, &y, &x)) return;
    const size_t b = blockIdx.y;
    const size_t pix = (size_t)y * W + x;
    const double* sc = scale + b * SE_VOL_JOINTS;
    const unsigned int live = vol_live(sc, P.mask);
    const double* r = rays + pix * 3;
    const double px = r[0], py = r[1], pz = r[2];
    const double* v = view.v;
    // q = R p + t: the eye is -R^T t and the pixel's direction R^T d, so that s stays view-space z
    const double ox = -((v[0] * v[9] + v[3] * v[10]) + v[6] * v[11]);
    const double oy = -((v[1] * v[9] + v[4] * v[10]) + v[7] * v[11]);
    const double oz = -((v[2] * v[9] + v[5] * v[10]) + v[8] * v[11]);
    const double dx = (v[0] * px + v[3] * py) + v[6] * pz;
    const double dy = (v[1] * px + v[4] * py) + v[7] * pz;
    const double dz = (v[2] * px + v[5] * py) + v[8] * pz;
    double limit = __longlong_as_double(0x7ff0000000000000ll);
    if (zbuf) {
        const unsigned long long z = zbuf[b * H * W + pix];
        if (z != ~0ull) limit = (double)__uint_as_float((unsigned int)(z >> 32));
    }
    float m[SE_VOL_SLOTS];
#pragma unroll
    for (int j = 0; j < SE_VOL_SLOTS; ++j) m[j] = 0.0f;
    const size_t cells = (size_t)P.G * P.G * P.G;
    const bool hit = live != 0 && vol_march(packed + b * cells * SE_VOL_SLOTS, P, live, ox, oy, oz, dx, dy, dz, limit, m);
    const size_t o3 = (b * H * W + pix) * 3;
    vol_composite(base + o3, out + o3, m, sc, live, hit, P);
}

__global__ __launch_bounds__(256) void render_volume_overlay_kernel(const float* __restrict__ packed, const double* __restrict__ scale,
                                                                    const double* __restrict__ rays, const float* __restrict__ depth,
                                                                    const unsigned char* base, unsigned char* out, int H, int W, int dh,
                                                                    int dw, VolParams P) {
    int y, x;
    if (!vol_pixel(H, W, &y, &x)) return;
    const size_t b = blockIdx.y;
    const size_t pix = (size_t)y * W + x;
    const double* sc = scale + b * SE_VOL_JOINTS;
    const unsigned int live = vol_live(sc, P.mask);
    const double* r = rays + pix * 3;
    double limit = __longlong_as_double(0x7ff0000000000000ll);
    if (depth) {
        const int sy = (int)(((long long)y * dh) / H), sx = (int)(((long long)x * dw) / W);
        limit = (double)depth[(b * dh + sy) * dw + sx];          // a cell shows where s < depth: nothing for a NaN
    }
    float m[SE_VOL_SLOTS];
#pragma unroll
    for (int j = 0; j < SE_VOL_SLOTS; ++j) m[j] = 0.0f;
    const size_t cells = (size_t)P.G * P.G * P.G;
    const bool hit = live != 0 && vol_march(packed + b * cells * SE_VOL_SLOTS, P, live, 0.0, 0.0, 0.0, r[0], r[1], r[2], limit, m);
    const size_t o3 = (b * H * W + pix) * 3;
    vol_composite(base + o3, out + o3, m, sc, live, hit, P);
}

inline bool vol_pixels_ok(int h, int w) { return h > 0 && w > 0 && (long long)h * w <= 0x7fffff00ll; }

inline bool vol_params(VolParams* P, int grid, double side, double near, unsigned int mask, double gain, double opacity) {
    if (grid < 2 || grid > 1024) return false;
    if (!(side > 0.0) || !(side <= 1e6) || !(near >= 0.0) || !(near <= 1e6)) return false;        // a NaN fails each
    if (!(gain >= 0.0) || !(gain <= 1e30) || !(opacity >= 0.0) || !(opacity <= 1.0)) return false;
    if (mask & ~0x7fffu) return false;
    P->G = grid;
    P->h = side / (double)(grid - 1);
    P->pos[0] = -(side / 2.0);
    P->pos[1] = -(side / 2.0);
    P->pos[2] = 0.0;
    P->near = near;
    P->gain = gain;
    P->opacity = opacity;
    P->mask = mask;
    return true;
}

inline unsigned vol_tiles(int h, int w) {
    return (unsigned)(((h + SE_VOL_TILE - 1) / SE_VOL_TILE) * ((w + SE_VOL_TILE - 1) / SE_VOL_TILE));
}

}  // namespace

extern "C" void se_render_volume_palette(unsigned char* rgb) {
    for (int j = 0; j < SE_VOL_JOINTS; ++j)
        for (int k = 0; k < 3; ++k) rgb[3 * j + k] = h_palette[j][k];
}

extern "C" long long se_render_volume_packed_bytes(int batch, int grid) {
    if (batch <= 0 || batch > 65535 || grid < 2 || grid > 1024) return SE_ERR_BAD_ARG;
    return (long long)batch * grid * grid * grid * SE_VOL_SLOTS * (long long)sizeof(float);
}

extern "C" int se_render_volume_pack_f32(const float* volumes, float* packed, long long packed_bytes, int batch, int grid, void* stream) {
    if (!volumes || !packed) return SE_ERR_BAD_ARG;
    const long long need = se_render_volume_packed_bytes(batch, grid);
    if (need < 0 || packed_bytes < need || (reinterpret_cast<uintptr_t>(packed) & 15)) return SE_ERR_BAD_ARG;
    const int cells = grid * grid * grid;
    hipLaunchKernelGGL(render_volume_pack_kernel, dim3((cells + 255) / 256, batch), dim3(256), 0, se_stream(stream), volumes, packed, cells);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_render_volume_view_f64(const float* packed, const double* scale, const double* rays, const double* view,
                                         const unsigned long long* zbuf, const unsigned char* base, unsigned char* out, int batch,
                                         int out_h, int out_w, int grid, double cuboid_side, double near, unsigned int joint_mask,
                                         double gain, double opacity, void* stream) {
    if (!packed || !scale || !rays || !view || !base || !out) return SE_ERR_BAD_ARG;
    if (batch <= 0 || batch > 65535 || !vol_pixels_ok(out_h, out_w) || (reinterpret_cast<uintptr_t>(packed) & 15)) return SE_ERR_BAD_ARG;
    VolParams P;
    if (!vol_params(&P, grid, cuboid_side, near, joint_mask, gain, opacity)) return SE_ERR_BAD_ARG;
    View v;
    for (int i = 0; i < 12; ++i) {
        if (!(view[i] - view[i] == 0.0)) return SE_ERR_BAD_ARG;      // a non-finite view
        v.v[i] = view[i];
    }
    hipLaunchKernelGGL(render_volume_view_kernel, dim3(vol_tiles(out_h, out_w), batch), dim3(256), 0, se_stream(stream), packed, scale,
                       rays, v, zbuf, base, out, out_h, out_w, P);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_render_volume_overlay_f64(const float* packed, const double* scale, const double* rays, const float* depth,
                                            const unsigned char* base, unsigned char* out, int batch, int height, int width, int depth_h,
                                            int depth_w, int grid, double cuboid_side, double near, unsigned int joint_mask, double gain,
                                            double opacity, void* stream) {
    if (!packed || !scale || !rays || !base || !out) return SE_ERR_BAD_ARG;
    if (batch <= 0 || batch > 65535 || !vol_pixels_ok(height, width) || (reinterpret_cast<uintptr_t>(packed) & 15)) return SE_ERR_BAD_ARG;
    if (depth && (depth_h <= 0 || depth_w <= 0)) return SE_ERR_BAD_ARG;
    VolParams P;
    if (!vol_params(&P, grid, cuboid_side, near, joint_mask, gain, opacity)) return SE_ERR_BAD_ARG;
    hipLaunchKernelGGL(render_volume_overlay_kernel, dim3(vol_tiles(height, width), batch), dim3(256), 0, se_stream(stream), packed, scale,
                       rays, depth, base, out, height, width, depth_h, depth_w, P);
    SE_CHECK_LAUNCH();
    return 0;
}
