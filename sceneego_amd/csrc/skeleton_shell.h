// What the two passes over the kinematic tree share: skeleton_prior.hip (sum-product, se_skeleton_couple_f32) and skeleton_pose.hip
// (max-product, se_skeleton_pose_f32) walk the same tree over the same dense shell blocks with the same workgroup tiling.  Stated once
// here: the limits, the tree and row maps handed to the kernels by value, the check of parent[] that builds them (sk_build_tree), the
// chunk rule of a row, the run table of a block of taps (sk_runs_kernel) and the launch geometry of a shell pass over G^3 outputs.
// skeleton_prior.hip describes the tiling.
//
// No `fp contract` pragma here: nothing below rounds.
#pragma once
#include "common.h"

#define SK_THREADS 256
#define SK_MAX_J 32
#define SK_MAX_G 128
#define SK_MAX_R 24
#define SK_TJ 16                 // output rows j per workgroup
#define SK_JR 4                  // ... per wave
#define SK_KC 64                 // output columns k per workgroup: one per lane
#define SK_MAX_CH 64
#define SK_GROUP 4               // frames in flight inside se_skeleton_couple_f32 and se_skeleton_pose_f32

namespace {

struct SkTree {
    int J;
    signed char parent[SK_MAX_J];
};
// rows of a launch inside the tree: row r = (frame r / n, joint slot[r % n])
struct SkRows {
    int n;
    unsigned char slot[SK_MAX_J];
};

__host__ __device__ inline int sk_chunks(int voxels) { return min(SK_MAX_CH, (voxels + 255) / 256); }
__host__ __device__ inline int sk_chunk(int voxels) { const int ch = sk_chunks(voxels); return (voxels + ch - 1) / ch; }
inline long long sk_runs_ints(int tap_rows, int R) { return (long long)tap_rows * (2 * R + 1) * (2 * R + 2) * 4; }

// grid (2R+1, tap_rows), block 64
__global__ __launch_bounds__(64) void sk_runs_kernel(const float* __restrict__ taps, int* __restrict__ runs, int R) {
    const int W = 2 * R + 1, t = threadIdx.x, dI = blockIdx.x, row = blockIdx.y;
    const float* w = taps + (size_t)row * W * W * W + (size_t)dI * W * W;
    int lo1 = 1, hi1 = 0, lo2 = 1, hi2 = 0, mid = 0;                     // dj + R; lo > hi: empty
    if (t < W) {
        int a = 0;
        while (a < W && w[a * W + t] == 0.f) ++a;
        if (a < W) {
            int b = a;
            while (b + 1 < W && w[(b + 1) * W + t] != 0.f) ++b;
            lo1 = a; hi1 = b;
            int d = W - 1;
            while (w[d * W + t] == 0.f) --d;                             // stops at b at the latest
            if (d > b) {
                int c = d;
                while (w[(c - 1) * W + t] != 0.f) --c;                   // stops above b: w[b + 1] is zero
                lo2 = c; hi2 = d;
                for (int e = b + 1; e < c; ++e) mid |= w[e * W + t] != 0.f;
            }
        }
    }
    const int any = __syncthreads_or(lo1 <= hi1);
    int* o = runs + (((size_t)row * W + dI) * (W + 1)) * 4;
    if (t < W) { o[t * 4 + 0] = lo1; o[t * 4 + 1] = hi1; o[t * 4 + 2] = lo2; o[t * 4 + 3] = hi2 | (mid << 8); }
    if (t == 0) { o[W * 4 + 0] = any; o[W * 4 + 1] = 0; o[W * 4 + 2] = 0; o[W * 4 + 3] = 0; }
}

inline bool sk_shape_ok(int G, int R) { return G >= 2 && G <= SK_MAX_G && R >= 0 && R <= SK_MAX_R && R <= G - 1; }
inline int sk_lds_bytes(int R) { return (SK_TJ + 2 * R) * (SK_KC + 2 * R) * 4; }
inline dim3 sk_corr_grid(int G, int rows) {
    return dim3(G * ((G + SK_TJ - 1) / SK_TJ) * ((G + SK_KC - 1) / SK_KC), rows);
}

// The tree of a call: false unless parent[0] == 0 and 0 <= parent[j] < j behind it (parents come first, so one ascending pass gives
// every depth).  Fills the tree handed to the kernels, the depth of every joint and the deepest level.
inline bool sk_build_tree(const int* parent, int J, SkTree& tree, int* depth, int& deepest) {
    if (parent[0] != 0) return false;
    tree.J = J;
    tree.parent[0] = 0;
    depth[0] = 0;
    deepest = 0;
    for (int j = 1; j < J; ++j) {
        if (parent[j] < 0 || parent[j] >= j) return false;
        tree.parent[j] = (signed char)parent[j];
        depth[j] = depth[parent[j]] + 1;
        deepest = max(deepest, depth[j]);
    }
    return true;
}

}  // namespace

// The upward pass of se_skeleton_couple_f32 on its own, with one level more for the root (skeleton_prior.hip: the third mode of sk_walk);
// se_skeleton_upward_f32 in skeleton_sample.hip is its entry point and checks the pointers and the scratch size.  SE_ERR_BAD_ARG with
// nothing launched for a bad shape, floor or tree; the size is 0 for a shape out of range.
int sk_upward_walk(const float* prob, const float* taps, const int* parent, float* upward, float* sums, int* valid, void* scratch,
                   int frames, int J, int voxels, int G, int R, float floor, void* stream);
long long sk_upward_scratch_bytes(int frames, int J, int G, int R);
