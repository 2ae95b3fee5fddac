// Draw primitives of the samplers: the Philox4x32-10 counter-based generator, its uniforms and the categorical draw by a sequential
// running sum.  volume_sample.hip (forward-filter backward-sampling over the joint volumes of a sequence) and skeleton_sample.hip
// (ancestral sampling of whole poses down the kinematic tree) stand on them; categorical_sums.h holds the sums pass both launch.
// tests/volume_sampler_model.py restates each in numpy and every draw of either sampler is compared with it bit for bit.  Nothing here touches memory
// other than the array it is given, and every function is plain C++ that compiles for the host as well.
//
// Include it from a file built with -ffp-contract=off: a running sum is one rounded addition per entry, a threshold one rounded product.
#pragma once
#include <float.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): the multipliers and the Weyl
// constants of the key schedule.  Pure 32-bit integer arithmetic.
#define SE_PHILOX_M0 0xD2511F53u
#define SE_PHILOX_M1 0xCD9E8D57u
#define SE_PHILOX_W0 0x9E3779B9u
#define SE_PHILOX_W1 0xBB67AE85u

struct SePhilox4 {
    uint32_t x[4];
};

// ten rounds on the counter (c0, c1, c2, c3) under the key (k0, k1), the key bumped by the Weyl constants between rounds
__host__ __device__ inline SePhilox4 se_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)SE_PHILOX_M0 * c0, p1 = (uint64_t)SE_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += SE_PHILOX_W0; k1 += SE_PHILOX_W1;
    }
    SePhilox4 r;
    r.x[0] = c0; r.x[1] = c1; r.x[2] = c2; r.x[3] = c3;
    return r;
}

// a uniform in [0, 1) from two words: the top 53 bits of (hi << 32 | lo) times 2^-53, exact
__host__ __device__ inline double se_uniform53(uint32_t hi, uint32_t lo) {
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1p-53;
}

// a total that a draw can be taken from: a finite number > 0 (a NaN fails both comparisons)
__host__ __device__ inline bool se_draw_mass_ok(double total) { return total > 0.0 && total <= DBL_MAX; }

// THE CATEGORICAL DRAW over the non-negative values v[0..n-1] with a uniform u in [0, 1): c_m = c_{m-1} + v_m (c_{-1} = 0, ascending
// m, one rounding per addition), total = c_{n-1}; the draw is the first m with c_m > u total, or, where rounding leaves none, the
// last m with v_m > 0.  A value of 0 is never drawn: its c_m equals c_{m-1}, which did not pass.  A total that is not a finite number
// > 0 gives no draw (-1).  Two halves, for one caller (one lane) at a time:
//   se_draw_scan    overwrites v with the running sums, returns the total and *last (the last m with v_m > 0, or -1)
//   se_draw_search  the draw from the running sums c, the total and u
__host__ __device__ inline double se_draw_scan(double* v, int n, int* last) {
    double c = 0.0;
    int l = -1;
    for (int m = 0; m < n; ++m) {
        const double x = v[m];
        if (x > 0.0) l = m;
        c = c + x;
        v[m] = c;
    }
    *last = l;
    return c;
}
__host__ __device__ inline int se_draw_search(const double* c, int n, int last, double total, double u) {
    if (!se_draw_mass_ok(total)) return -1;
    const double thr = u * total;
    for (int m = 0; m < n; ++m)
        if (c[m] > thr) return m;
    return last;
}
__host__ __device__ inline int se_draw(double* v, int n, double u) {
    int last;
    const double total = se_draw_scan(v, n, &last);
    return se_draw_search(v, n, last, total, u);
}
