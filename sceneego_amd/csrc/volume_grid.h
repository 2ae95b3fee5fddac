// What the operators over the joint volumes of a sequence share on the host side: volume_filter.hip (the grid Bayes filter and its
// backward smoother) and volume_viterbi.hip (the max-product pass) take the same [frames][rows][G^3] volumes, the same taps and the same
// floor, cut a plane over the same 256 threads and a row over the same chunks.  Stated once here: the limits, the shape predicate,
// the elements of a frame, the launch parameters every call derives from (G, voxels, floor) and the argument gate of the three
// se_volume_*_f32 entry points.  Python guards all three with the one pair _lib.FILTER_MAX_GRID / FILTER_MAX_RADIUS.
//
// No `fp contract` pragma here: nothing below rounds on the device, and the two host divisions are single operations.
#pragma once
#include "common.h"

#define SE_VG_THREADS 256
#define SE_VG_MAX_G 128
#define SE_VG_MAX_R 16
#define SE_VG_MAX_CHUNKS 64

namespace {

inline bool vg_shape_ok(int rows, int G, int R) {
    return rows >= 1 && rows <= 65535 && G >= 2 && G <= SE_VG_MAX_G && R >= 0 && R <= SE_VG_MAX_R && R <= G - 1;
}
inline long long vg_elems(int rows, int G) { return (long long)rows * G * G * G; }

// frames, shape, voxels == G^3 and a floor in [0, 1]
inline bool vg_args_ok(int frames, int rows, int voxels, int G, int R, float floor) {
    if (frames < 1 || !vg_shape_ok(rows, G, R)) return false;
    if ((long long)G * G * G != (long long)voxels) return false;
    return floor >= 0.f && floor <= 1.f;                                                  // a NaN fails
}

// A thread owns column k = t & (W - 1) of a staged plane, W = 1 << wshift the power of two >= G (<= 128); a row pass runs over
// `chunks` workgroups of 4 voxels per lane; u = keep q + uniform is the floor.
struct VgLaunch {
    int wshift, chunks;
    float keep, uniform;
};
inline VgLaunch vg_launch(int voxels, int G, float floor) {
    VgLaunch l;
    l.wshift = 0;
    while ((1 << l.wshift) < G) ++l.wshift;
    l.chunks = min(SE_VG_MAX_CHUNKS, (voxels + SE_VG_THREADS * 4 - 1) / (SE_VG_THREADS * 4));
    l.keep = 1.0f - floor;
    l.uniform = floor / (float)voxels;
    return l;
}

}  // namespace
