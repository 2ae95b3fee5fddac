// Headless renderer: the scene point cloud of a depth map and the predicted skeleton, drawn on the device (stands in for the
// reference's visualize.py: utils/depth2pointcloud.py + utils/skeleton.py joints_2_mesh in an open3d window).
//
//   se_render_splat_f64    one thread per frame pixel: depth * calibrated ray -> view space -> pinhole pixel -> 64-bit atomicMin of
//                          (float bits of view z) << 32 | 0x00RRGGBB into the z-buffer.  Positive floats order like their bit
//                          patterns, so the minimum is the nearest point and, among equal depths, the lowest colour word: the
//                          result does not depend on the launch order and is bitwise reproducible.
//   se_render_resolve_f64  one thread per output pixel: ray-cast 15 spheres + 15 capless cylinders along the pixel's ray, then
//   se_render_overlay_f64  compose with the z-buffer (resolve) or with the fisheye frame, optionally hidden behind its depth (overlay).
//                          Both views share one device function: a table of ray directions through the origin per pixel makes the
//                          pinhole (hit parameter = view z) and the fisheye (unit rays: hit parameter = distance) the same problem.
//
// All arithmetic is float64 and unfused (built with -ffp-contract=off), in the operation order of include/sceneego_hip.h, so that
// tests/render_model.py can restate it literally: the splat is tested bit for bit.  None of this is bandwidth- or matrix-bound:
// 28 B per frame pixel in (4 depth + 24 ray), 24 B per output pixel in.
#include "common.h"

#pragma clang fp contract(off)

namespace {

#define SE_RENDER_JOINTS 15
// Skeleton.lines of the reference (utils/skeleton.py:20-21)
__constant__ int c_bones[SE_RENDER_JOINTS][2] = {{0, 1}, {0, 4}, {1, 2}, {2, 3}, {4, 5}, {5, 6}, {1, 7}, {4, 11}, {7, 8}, {8, 9},
                                                 {9, 10}, {11, 12}, {12, 13}, {13, 14}, {7, 11}};

struct Colours {
    float joint[3], bone[3];
};

// The z-buffer is cleared by a kernel, not by hipMemsetAsync: a memset node captured into a hipGraph replayed with garbage on
// ROCm 7.2 (see zero_kernel in voxelize.hip), and these entry points have to be legal inside a capture.
__global__ __launch_bounds__(256) void render_fill_kernel(unsigned long long* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = ~0ull;
}

// grid (ceil(H * W / 256), B): thread = frame pixel (y, x), x fastest, so depth rows, rays and colours are read coalesced
__global__ __launch_bounds__(256) void render_splat_kernel(const float* __restrict__ depth, const double* __restrict__ ray_tab,
                                                           const unsigned char* __restrict__ image, const double* __restrict__ view,
                                                           unsigned long long* __restrict__ zbuf, int dh, int dw, int H, int W,
                                                           int Hout, int Wout, double f, double cx, double cy, int splat,
                                                           double min_z, double max_depth, double near) {
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const int y = pix / W, x = pix - y * W;
    const int sy = (int)(((long long)y * dh) / H), sx = (int)(((long long)x * dw) / W);
    const double d = (double)depth[((size_t)b * dh + sy) * dw + sx];
    if (!(d > 0.0 && d <= max_depth)) return;          // NaN fails both
    const double* r = ray_tab + (size_t)pix * 3;
    const double px = r[0] * d, py = r[1] * d, pz = r[2] * d;
    if (!(pz > min_z)) return;
    const double qx = ((view[0] * px + view[1] * py) + view[2] * pz) + view[9];
    const double qy = ((view[3] * px + view[4] * py) + view[5] * pz) + view[10];
    const double qz = ((view[6] * px + view[7] * py) + view[8] * pz) + view[11];
    if (!(qz > near)) return;
    const double u = (f * qx) / qz + cx, v = (f * qy) / qz + cy;
    // the range is checked on the doubles, before any conversion to int
    if (!(u >= -4.0 && u < (double)(Wout + 4) && v >= -4.0 && v < (double)(Hout + 4))) return;
    const int iu = (int)floor(u), iv = (int)floor(v);
    const unsigned char* c = image + ((size_t)b * H * W + pix) * 3;      // B, G, R
    const unsigned long long colour = ((unsigned long long)c[2] << 16) | ((unsigned long long)c[1] << 8) | (unsigned long long)c[0];
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)qz) << 32) | colour;
    unsigned long long* zb = zbuf + (size_t)b * Hout * Wout;
    const int off = (splat - 1) / 2;
    for (int dy = 0; dy < splat; ++dy) {
        const int oy = iv - off + dy;
        if (oy < 0 || oy >= Hout) continue;
        for (int dx = 0; dx < splat; ++dx) {
            const int ox = iu - off + dx;
            if (ox < 0 || ox >= Wout) continue;
            unsigned long long* slot = zb + (size_t)oy * Wout + ox;
            // keys only ever decrease: a (possibly stale) stored key <= ours means ours can never win; the atomic decides the rest
            if (*slot <= key) continue;
            atomicMin(slot, key);
        }
    }
}

struct Hit {
    double s;        // ray parameter of the nearest hit (valid when kind >= 0)
    int kind;        // -1 none, 0 sphere, 1 cylinder
    double nx, ny, nz;   // surface normal at the hit, not normalised
};

__device__ __forceinline__ bool finite3(const double* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// Nearest intersection with s > near of the ray s * (dx, dy, dz) with the skeleton `J` (15 joints, LDS).  Spheres first, then bones,
// each in index order; a candidate replaces the current one only when strictly smaller.
__device__ __forceinline__ Hit render_trace(const double* J, double dx, double dy, double dz, double r_joint, double r_bone, double near) {
    Hit h;
    h.s = 0.0; h.kind = -1; h.nx = h.ny = h.nz = 0.0;
    const double a = (dx * dx + dy * dy) + dz * dz;
    for (int j = 0; j < SE_RENDER_JOINTS; ++j) {
        const double* c = J + 3 * j;
        if (!finite3(c)) continue;
        const double bq = (dx * c[0] + dy * c[1]) + dz * c[2];
        const double cq = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) - r_joint * r_joint;
        const double disc = bq * bq - a * cq;
        if (!(disc >= 0.0)) continue;
        const double sq = sqrt(disc);
        const double roots[2] = {(bq - sq) / a, (bq + sq) / a};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double s = roots[k];
            if (s > near && (h.kind < 0 || s < h.s)) {
                h.s = s; h.kind = 0;
                h.nx = s * dx - c[0]; h.ny = s * dy - c[1]; h.nz = s * dz - c[2];
            }
        }
    }
    for (int e = 0; e < SE_RENDER_JOINTS; ++e) {
        const double* A = J + 3 * c_bones[e][0];
        const double* B = J + 3 * c_bones[e][1];
        if (!finite3(A) || !finite3(B)) continue;
        const double vx = B[0] - A[0], vy = B[1] - A[1], vz = B[2] - A[2];
        const double vv = (vx * vx + vy * vy) + vz * vz;
        if (!(sqrt(vv) >= 1e-9)) continue;                 // a bone shorter than 1e-9 m
        const double dv = (dx * vx + dy * vy) + dz * vz;
        const double av = (A[0] * vx + A[1] * vy) + A[2] * vz;
        const double kd = dv / vv, ka = av / vv;
        // the parts of the direction and of A perpendicular to the axis
        const double ex = dx - kd * vx, ey = dy - kd * vy, ez = dz - kd * vz;
        const double gx = A[0] - ka * vx, gy = A[1] - ka * vy, gz = A[2] - ka * vz;
        const double qa = (ex * ex + ey * ey) + ez * ez;
        if (!(qa > 0.0)) continue;                         // ray along the axis
        const double qb = (ex * gx + ey * gy) + ez * gz;
        const double qc = ((gx * gx + gy * gy) + gz * gz) - r_bone * r_bone;
        const double disc = qb * qb - qa * qc;
        if (!(disc >= 0.0)) continue;
        const double sq = sqrt(disc);
        const double roots[2] = {(qb - sq) / qa, (qb + sq) / qa};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double s = roots[k];
            const double t = (s * dv - av) / vv;           // axial parameter: 0 at A, 1 at B
            if (s > near && t >= 0.0 && t <= 1.0 && (h.kind < 0 || s < h.s)) {
                h.s = s; h.kind = 1;
                h.nx = s * ex - gx; h.ny = s * ey - gy; h.nz = s * ez - gz;
            }
        }
    }
    return h;
}

// colour of a hit: base * (0.3 + 0.7 * max(0, n . l)), l = -dir / |dir|, per channel (int)(255 * base * shade + 0.5)
__device__ __forceinline__ void render_shade(const Hit& h, double dx, double dy, double dz, const Colours& col, unsigned char* rgb) {
    const double nn = sqrt((h.nx * h.nx + h.ny * h.ny) + h.nz * h.nz);
    const double dn = sqrt((dx * dx + dy * dy) + dz * dz);
    const double ndl = -(((h.nx * dx + h.ny * dy) + h.nz * dz) / (nn * dn));
    const double shade = 0.3 + 0.7 * (ndl > 0.0 ? ndl : 0.0);       // a NaN (degenerate normal) shades as 0.3
    const float* base = h.kind == 0 ? col.joint : col.bone;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = (255.0 * (double)base[c]) * shade + 0.5;
        const int q = (int)v;
        rgb[c] = (unsigned char)(q < 0 ? 0 : q > 255 ? 255 : q);
    }
}

__device__ __forceinline__ void load_joints(double* J, const double* __restrict__ joints, int b) {
    if (threadIdx.x < 3 * SE_RENDER_JOINTS) J[threadIdx.x] = joints[(size_t)b * 3 * SE_RENDER_JOINTS + threadIdx.x];
    __syncthreads();
}

// grid (ceil(Hout * Wout / 256), B)
__global__ __launch_bounds__(256) void render_resolve_kernel(const double* __restrict__ rays, const double* __restrict__ joints,
                                                             const unsigned long long* __restrict__ zbuf, unsigned char* __restrict__ out,
                                                             int npix, double r_joint, double r_bone, double near, Colours col,
                                                             unsigned int background) {
    __shared__ double J[3 * SE_RENDER_JOINTS];
    const int b = blockIdx.y;
    load_joints(J, joints, b);
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    const double* r = rays + (size_t)pix * 3;
    const double dx = r[0], dy = r[1], dz = r[2];
    const Hit h = render_trace(J, dx, dy, dz, r_joint, r_bone, near);
    const unsigned long long z = zbuf[(size_t)b * npix + pix];
    const bool empty = z == ~0ull;
    unsigned char rgb[3];
    // strict: a tie goes to the scene
    if (h.kind >= 0 && (empty || h.s < (double)__uint_as_float((unsigned int)(z >> 32)))) {
        render_shade(h, dx, dy, dz, col, rgb);
    } else {
        const unsigned int w = empty ? background : (unsigned int)z;
        rgb[0] = (unsigned char)(w >> 16); rgb[1] = (unsigned char)(w >> 8); rgb[2] = (unsigned char)w;
    }
    unsigned char* o = out + ((size_t)b * npix + pix) * 3;
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

// grid (ceil(H * W / 256), B)
__global__ __launch_bounds__(256) void render_overlay_kernel(const double* __restrict__ rays, const double* __restrict__ joints,
                                                             const unsigned char* __restrict__ frame, const float* __restrict__ depth,
                                                             unsigned char* __restrict__ out, int H, int W, int dh, int dw,
                                                             double r_joint, double r_bone, double near, Colours col) {
    __shared__ double J[3 * SE_RENDER_JOINTS];
    const int b = blockIdx.y;
    load_joints(J, joints, b);
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    const double* r = rays + (size_t)pix * 3;
    const double dx = r[0], dy = r[1], dz = r[2];
    const Hit h = render_trace(J, dx, dy, dz, r_joint, r_bone, near);
    bool show = h.kind >= 0;
    if (show && depth) {
        const int y = pix / W, x = pix - y * W;
        const int sy = (int)(((long long)y * dh) / H), sx = (int)(((long long)x * dw) / W);
        show = h.s < (double)depth[((size_t)b * dh + sy) * dw + sx];     // false for a NaN depth
    }
    const unsigned char* c = frame + ((size_t)b * H * W + pix) * 3;      // B, G, R
    unsigned char rgb[3] = {c[2], c[1], c[0]};
    if (show) render_shade(h, dx, dy, dz, col, rgb);
    unsigned char* o = out + ((size_t)b * H * W + pix) * 3;
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

inline bool pixels_ok(int h, int w) { return h > 0 && w > 0 && (long long)h * w <= 0x7fffff00ll; }

}  // namespace

extern "C" int se_render_splat_f64(const float* depth, const double* ray_tab, const unsigned char* image, const double* view,
                                   unsigned long long* zbuf, int batch, int depth_h, int depth_w, int height, int width, int out_h,
                                   int out_w, double f, double cx, double cy, int splat, double min_z, double max_depth, double near,
                                   void* stream) {
    if (!depth || !ray_tab || !image || !view || !zbuf) return SE_ERR_BAD_ARG;
    if (batch <= 0 || batch > 65535 || depth_h <= 0 || depth_w <= 0 || !pixels_ok(height, width) || !pixels_ok(out_h, out_w))
        return SE_ERR_BAD_ARG;
    if (splat < 1 || splat > 4 || !(near >= 0.0) || !(f > 0.0)) return SE_ERR_BAD_ARG;     // near >= 0: the key needs a positive float
    hipStream_t s = se_stream(stream);
    const size_t n = (size_t)batch * out_h * out_w;
    const unsigned fgrid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(render_fill_kernel, dim3(fgrid), dim3(256), 0, s, zbuf, n);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(render_splat_kernel, dim3((height * width + 255) / 256, batch), dim3(256), 0, s, depth, ray_tab, image, view, zbuf,
                       depth_h, depth_w, height, width, out_h, out_w, f, cx, cy, splat, min_z, max_depth, near);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_render_resolve_f64(const double* rays, const double* joints, const unsigned long long* zbuf, unsigned char* out,
                                     int batch, int out_h, int out_w, double r_joint, double r_bone, double near,
                                     const float* joint_rgb, const float* bone_rgb, const unsigned char* background, void* stream) {
    if (!rays || !joints || !zbuf || !out || !joint_rgb || !bone_rgb || !background) return SE_ERR_BAD_ARG;
    if (batch <= 0 || batch > 65535 || !pixels_ok(out_h, out_w)) return SE_ERR_BAD_ARG;
    Colours col;
    for (int c = 0; c < 3; ++c) { col.joint[c] = joint_rgb[c]; col.bone[c] = bone_rgb[c]; }
    const unsigned int bg = ((unsigned int)background[0] << 16) | ((unsigned int)background[1] << 8) | (unsigned int)background[2];
    const int npix = out_h * out_w;
    hipLaunchKernelGGL(render_resolve_kernel, dim3((npix + 255) / 256, batch), dim3(256), 0, se_stream(stream), rays, joints, zbuf, out,
                       npix, r_joint, r_bone, near, col, bg);
    SE_CHECK_LAUNCH();
    return 0;
}

extern "C" int se_render_overlay_f64(const double* rays, const double* joints, const unsigned char* frame, const float* depth,
                                     unsigned char* out, int batch, int height, int width, int depth_h, int depth_w, double r_joint,
                                     double r_bone, double near, const float* joint_rgb, const float* bone_rgb, void* stream) {
    if (!rays || !joints || !frame || !out || !joint_rgb || !bone_rgb) return SE_ERR_BAD_ARG;
    if (batch <= 0 || batch > 65535 || !pixels_ok(height, width)) return SE_ERR_BAD_ARG;
    if (depth && (depth_h <= 0 || depth_w <= 0)) return SE_ERR_BAD_ARG;
    Colours col;
    for (int c = 0; c < 3; ++c) { col.joint[c] = joint_rgb[c]; col.bone[c] = bone_rgb[c]; }
    hipLaunchKernelGGL(render_overlay_kernel, dim3((height * width + 255) / 256, batch), dim3(256), 0, se_stream(stream), rays, joints,
                       frame, depth, out, height, width, depth_h, depth_w, r_joint, r_bone, near, col);
    SE_CHECK_LAUNCH();
    return 0;
}
