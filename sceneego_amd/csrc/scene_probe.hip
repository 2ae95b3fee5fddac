// Scene probe: every scene point of a depth map against up to 64 probe points per frame (the joints of a predicted skeleton and
// samples along its bones; sceneego_amd/scene_check.py drives it).  Per probe: the nearest scene point, and the pixel whose ray
// points at the probe (its line of sight) with the depth surface there.  No counterpart in the reference.
//
//   scene_probe_tile_kernel    one workgroup per (pixel tile, frame): 256 threads x 8 pixels.  The scene point s = ray * d and the ray
//                              of each pixel stay in registers, the frame's probes in LDS; the probes are walked in the outer loop.
//                              Per probe a lexicographic (value, pixel index) minimum of |s - c|^2 and maximum of ray . c: in the
//                              thread, across the wave by shuffles, across the 4 waves through LDS.  One partial record per
//                              (frame, probe, tile) goes to `scratch`.  blockIdx.x = tile * B + frame: the B workgroups that read
//                              one tile of the ray table are neighbours in the dispatch order.  Measured (profiles/
//                              scene_check_cost.txt): the L2s still fetch 3.1 x "table once + B depth maps" at B = 8, because
//                              neighbouring workgroups land on different XCDs; the launch is bound by arithmetic either way.
//   scene_probe_finish_kernel  one wave per (frame, probe): reduces the tile records the same way and writes the out / index rows.
//
// (value, index) pairs under a lexicographic order have one minimum whatever the order of the reduction: no floating-point atomics,
// nothing depends on the launch order, two calls give the same bits.  Nothing is allocated: legal under hipGraph capture.
//
// All arithmetic is float64 and unfused (built with -ffp-contract=off), in the operation order of include/sceneego_hip.h; every dot
// product is (x x + y y) + z z.  There are no square roots and no divisions: every value written is a correctly rounded sum or
// product, or a copy, so tests/scene_model.py restates it literally and the output is tested bit for bit.
#include <limits.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

#define SE_PROBE_MAX 64
#define SE_PROBE_THREADS 256
#define SE_PROBE_PPT 8                                      // pixels per thread: 12 VGPRs each (s and the ray)
#define SE_PROBE_TILE (SE_PROBE_THREADS * SE_PROBE_PPT)     // 2048 pixels per workgroup
#define SE_PROBE_WAVES (SE_PROBE_THREADS / SE_WAVE)

struct ProbePartial {      // of one (frame, probe, tile); 24 bytes
    double q, t;           // least |s - c|^2 over the tile's scene points (+inf: none), greatest ray . c (-inf: none)
    int qi, ti;            // the lowest pixel index that attains each (INT_MAX: none)
};

__device__ __forceinline__ bool lex_less(double a, int ai, double b, int bi) { return a < b || (a == b && ai < bi); }
__device__ __forceinline__ bool lex_greater(double a, int ai, double b, int bi) { return a > b || (a == b && ai < bi); }

__device__ __forceinline__ void wave_lex_min(double& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (lex_less(ov, oi, v, i)) { v = ov; i = oi; }
    }
}
__device__ __forceinline__ void wave_lex_max(double& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (lex_greater(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// grid (tiles * B): tile = blockIdx.x / B, frame = blockIdx.x % B.  Thread t owns the pixels tile * 2048 + k * 256 + t, k = 0..7:
// coalesced loads, and inside a thread the pixel index grows with k, so a strict comparison keeps the lowest index.
__global__ __launch_bounds__(SE_PROBE_THREADS) void scene_probe_tile_kernel(const float* __restrict__ depth,
                                                                           const double* __restrict__ ray_tab,
                                                                           const double* __restrict__ probes,
                                                                           ProbePartial* __restrict__ part, int B, int dh, int dw, int H,
                                                                           int W, int P, int tiles, double min_z, double max_depth) {
    __shared__ double sc[SE_PROBE_MAX * 3];
    __shared__ ProbePartial sw[SE_PROBE_MAX][SE_PROBE_WAVES];
    const int tile = blockIdx.x / B, b = blockIdx.x - tile * B;
    const int tid = threadIdx.x;
    if (tid < 3 * P) sc[tid] = probes[(size_t)b * P * 3 + tid];

    const int npix = H * W;
    const int base = tile * SE_PROBE_TILE + tid;
    double sx[SE_PROBE_PPT], sy[SE_PROBE_PPT], sz[SE_PROBE_PPT], rx[SE_PROBE_PPT], ry[SE_PROBE_PPT], rz[SE_PROBE_PPT];
    unsigned scene = 0, sight = 0;                          // bit k: pixel k of this thread is a scene point / has a finite ray
#pragma unroll
    for (int k = 0; k < SE_PROBE_PPT; ++k) {
        const int pix = base + k * SE_PROBE_THREADS;
        sx[k] = sy[k] = sz[k] = rx[k] = ry[k] = rz[k] = 0.0;
        if (pix < npix) {
            const double* r = ray_tab + (size_t)pix * 3;
            rx[k] = r[0]; ry[k] = r[1]; rz[k] = r[2];
            if (isfinite(rx[k]) && isfinite(ry[k]) && isfinite(rz[k])) {
                sight |= 1u << k;
                const int y = pix / W, x = pix - y * W;
                const int py = (int)(((long long)y * dh) / H), px = (int)(((long long)x * dw) / W);
                const double d = (double)depth[((size_t)b * dh + py) * dw + px];
                if (d > 0.0 && d <= max_depth) {            // NaN fails both
                    sx[k] = rx[k] * d; sy[k] = ry[k] * d; sz[k] = rz[k] * d;
                    if (sz[k] > min_z) scene |= 1u << k;
                }
            }
        }
    }
    __syncthreads();

    const int lane = tid & (SE_WAVE - 1), wave = tid / SE_WAVE;
    for (int p = 0; p < P; ++p) {
        const double cx = sc[3 * p], cy = sc[3 * p + 1], cz = sc[3 * p + 2];
        double q = __longlong_as_double(0x7ff0000000000000ll), t = -__longlong_as_double(0x7ff0000000000000ll);
        int qi = INT_MAX, ti = INT_MAX;
#pragma unroll
        for (int k = 0; k < SE_PROBE_PPT; ++k) {
            const int pix = base + k * SE_PROBE_THREADS;
            const double ex = sx[k] - cx, ey = sy[k] - cy, ez = sz[k] - cz;
            const double qq = (ex * ex + ey * ey) + ez * ez;
            const double tt = (rx[k] * cx + ry[k] * cy) + rz[k] * cz;
            if (((scene >> k) & 1u) && lex_less(qq, pix, q, qi)) { q = qq; qi = pix; }
            if (((sight >> k) & 1u) && lex_greater(tt, pix, t, ti)) { t = tt; ti = pix; }
        }
        wave_lex_min(q, qi);
        wave_lex_max(t, ti);
        if (lane == 0) {
            ProbePartial r;
            r.q = q; r.t = t; r.qi = qi; r.ti = ti;
            sw[p][wave] = r;
        }
    }
    __syncthreads();
    if (tid < P) {
        ProbePartial r = sw[tid][0];
#pragma unroll
        for (int w = 1; w < SE_PROBE_WAVES; ++w) {
            const ProbePartial o = sw[tid][w];
            if (lex_less(o.q, o.qi, r.q, r.qi)) { r.q = o.q; r.qi = o.qi; }
            if (lex_greater(o.t, o.ti, r.t, r.ti)) { r.t = o.t; r.ti = o.ti; }
        }
        part[((size_t)b * P + tid) * tiles + tile] = r;
    }
}

// grid (B * P), one wave: row = frame * P + probe
__global__ __launch_bounds__(SE_WAVE) void scene_probe_finish_kernel(const float* __restrict__ depth, const double* __restrict__ ray_tab,
                                                                    const double* __restrict__ probes,
                                                                    const ProbePartial* __restrict__ part, double* __restrict__ out,
                                                                    int* __restrict__ index, int dh, int dw, int H, int W, int P,
                                                                    int tiles, double min_z, double max_depth) {
    const int row = blockIdx.x, b = row / P, lane = threadIdx.x;
    const double cx = probes[(size_t)row * 3], cy = probes[(size_t)row * 3 + 1], cz = probes[(size_t)row * 3 + 2];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double* o = out + (size_t)row * 8;
    int* ix = index + (size_t)row * 2;
    if (!(isfinite(cx) && isfinite(cy) && isfinite(cz))) {
        if (lane < 8) o[lane] = nan;
        if (lane < 2) ix[lane] = -1;
        return;
    }
    double q = __longlong_as_double(0x7ff0000000000000ll), t = -__longlong_as_double(0x7ff0000000000000ll);
    int qi = INT_MAX, ti = INT_MAX;
    const ProbePartial* pr = part + (size_t)row * tiles;
    for (int i = lane; i < tiles; i += SE_WAVE) {
        const ProbePartial r = pr[i];
        if (lex_less(r.q, r.qi, q, qi)) { q = r.q; qi = r.qi; }
        if (lex_greater(r.t, r.ti, t, ti)) { t = r.t; ti = r.ti; }
    }
    wave_lex_min(q, qi);
    wave_lex_max(t, ti);
    if (lane != 0) return;
    o[0] = q;
    if (qi == INT_MAX) {
        o[1] = o[2] = o[3] = nan;
        ix[0] = -1;
    } else {
        const int y = qi / W, x = qi - y * W;
        const int py = (int)(((long long)y * dh) / H), px = (int)(((long long)x * dw) / W);
        const double d = (double)depth[((size_t)b * dh + py) * dw + px];
        const double* r = ray_tab + (size_t)qi * 3;
        o[1] = r[0] * d; o[2] = r[1] * d; o[3] = r[2] * d;
        ix[0] = qi;
    }
    o[4] = (cx * cx + cy * cy) + cz * cz;
    o[5] = t;
    double surface = nan;
    if (ti != INT_MAX) {
        const int y = ti / W, x = ti - y * W;
        const int py = (int)(((long long)y * dh) / H), px = (int)(((long long)x * dw) / W);
        const double d = (double)depth[((size_t)b * dh + py) * dw + px];
        if (d > 0.0 && d <= max_depth) surface = d;
    }
    o[6] = surface;
    o[7] = 0.0;
    ix[1] = ti == INT_MAX ? -1 : ti;
}

inline bool probe_shape_ok(int batch, int height, int width, int probes) {
    return batch > 0 && batch <= 65535 && height > 0 && width > 0 && (long long)height * width <= 0x7fff0000ll && probes >= 1 &&
           probes <= SE_PROBE_MAX;
}
inline long long probe_tiles(int height, int width) { return ((long long)height * width + SE_PROBE_TILE - 1) / SE_PROBE_TILE; }

}  // namespace

extern "C" long long se_scene_probe_scratch_bytes(int batch, int height, int width, int probes) {
    if (!probe_shape_ok(batch, height, width, probes)) return -1;
    return (long long)batch * probes * probe_tiles(height, width) * (long long)sizeof(ProbePartial);
}

extern "C" int se_scene_probe_f64(const float* depth, const double* ray_tab, const double* probes, double* out, int* index,
                                  void* scratch, long long scratch_bytes, int batch, int depth_h, int depth_w, int height, int width,
                                  int n_probes, double min_z, double max_depth, void* stream) {
    if (!depth || !ray_tab || !probes || !out || !index || !scratch) return SE_ERR_BAD_ARG;
    if (!probe_shape_ok(batch, height, width, n_probes) || depth_h <= 0 || depth_w <= 0) return SE_ERR_BAD_ARG;
    if (!(min_z >= 0.0) || !(max_depth > 0.0)) return SE_ERR_BAD_ARG;            // a NaN fails both
    if (scratch_bytes < se_scene_probe_scratch_bytes(batch, height, width, n_probes)) return SE_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(scratch) & 7) return SE_ERR_BAD_ARG;
    const long long tiles = probe_tiles(height, width);
    if (tiles * batch > 0x7fffffffll) return SE_ERR_BAD_ARG;
    hipStream_t s = se_stream(stream);
    ProbePartial* part = static_cast<ProbePartial*>(scratch);
    hipLaunchKernelGGL(scene_probe_tile_kernel, dim3((unsigned)(tiles * batch)), dim3(SE_PROBE_THREADS), 0, s, depth, ray_tab, probes, part,
                       batch, depth_h, depth_w, height, width, n_probes, (int)tiles, min_z, max_depth);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(scene_probe_finish_kernel, dim3((unsigned)(batch * n_probes)), dim3(SE_WAVE), 0, s, depth, ray_tab, probes, part, out,
                       index, depth_h, depth_w, height, width, n_probes, (int)tiles, min_z, max_depth);
    SE_CHECK_LAUNCH();
    return 0;
}
