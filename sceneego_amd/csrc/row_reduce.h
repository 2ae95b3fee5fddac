// The split-row reduction over [rows, voxels]: everything a kernel needs to take part in it, stated once.
//
// THE SCHEME.  A row of `voxels` values (a multiple of 4) is cut into splits = se_sa_splits(rows) chunks of se_row_chunk(voxels, splits)
// values, a multiple of 4, so that rows x splits workgroups fill the CUs at every batch size.  Chunk k covers [k chunk, min((k + 1) chunk,
// voxels)); it is EMPTY iff k chunk >= voxels (SE_CHUNK_EMPTY) - the last chunks of a short row - and an empty chunk is skipped by its
// position, never for the value of its record: a NaN that a chunk produced must reach the row's result.
//   pass 1  grid (splits, rows), block 256: thread t takes the quads at c0 + 4 t, + 1024, ... of its chunk in sequence (load_quad: four
//           values and their de-interleaved coordinates), the workgroup folds the per-lane sums (block_fold_stage: a butterfly over
//           the lanes of each wave; block_fold_sum: the four waves as (0 + 1) + (2 + 3)) and writes one record per chunk into scratch
//           (block_fold_record does all three for sums with a peak).
//   pass 2  one wave folds the row's records (wave_fold_chunks; wave_fold_records without the skip and the peak: lane k takes records
//           k, k + 64, ... in sequence, then a butterfly over the lanes) and the caller's epilogue writes the row's result.
// The per-voxel loop stays in each kernel, over load_quad: a loop body handed to a shared skeleton is optimised apart from the kernel
// around it and came out scheduled worse (joint statistics at batch 32: 0.165 -> 0.198 ms).
// DETERMINISM.  No atomics.  Which values a lane adds, and in which order, follows from (rows, voxels) and the launch geometry alone; the
// butterfly, the four-wave fold and the record fold are fixed trees.  So every float32 sum is bitwise identical from run to run, and
// every workgroup that folds the same records (softargmax_finish_kernel, vf_finish_kernel) holds the same value, bit for bit.
// THE PEAK is the pair (p, index) under the order "larger p first, then lower index": peak_combine is commutative and associative, so
// any reduction tree gives the same pair.  PEAK_NONE (-inf, INT_MAX) is its neutral element; it survives only where nothing was offered.
// A NaN value is carried in the same pair as PEAK_NAN (+inf, -1), which wins every combine: a row whose folded index is negative
// held a NaN.  In a record the peak follows the N sums: p at [N], the index's bits at [N + 1].
// Who writes which records: softargmax.hip and the fused V2V tails (conv3d_tail.hip, conv3d_bf16.hip) write SE_SA_PART records that
// softargmax_finish_kernel reads; joint_stats.hip and scene_constraint.hip write and fold their own; volume_filter.hip uses the
// workgroup fold and the record fold over its G records per row (no peak, no empty record).
//
// No `fp contract` pragma here: the code below takes the setting of the file that includes it.
#pragma once
#include <limits.h>

#include "common.h"

// floats per soft-argmax pass-1 record: m, l, sx, sy, sz, pad
#define SE_SA_PART 8
// chunks per row: 32 from batch 8 on (15 rows per sample: 120 rows x 32 chunks = 3840 workgroups for the two-pass form, 256 for the
// fused tail, which runs one workgroup per (chunk, sample)); fewer rows get more chunks so that the fused tail still has ~256
// workgroups (batch 1: 256 chunks of 1024 voxels at 64^3 - it ran 32 workgroups on 256 CUs before: 116 us of a 3.3 ms frame)
inline int se_sa_splits(int rows) { return rows >= 120 ? 32 : rows >= 60 ? 64 : rows >= 30 ? 128 : 256; }
// values per chunk: ceil(voxels / splits), rounded up to whole quads
__host__ __device__ __forceinline__ int se_row_chunk(int voxels, int splits) { return (((voxels + splits - 1) / splits) + 3) & ~3; }
// chunk k holds nothing (a macro: as a function it left softargmax_finish_kernel with two instructions in another order)
#define SE_CHUNK_EMPTY(k, chunk, voxels) ((k) * (chunk) >= (voxels))

struct Peak {
    float p;
    int idx;
};
#define PEAK_NONE (Peak{-INFINITY, INT_MAX})
#define PEAK_NAN (Peak{INFINITY, -1})
__device__ __forceinline__ Peak peak_combine(Peak a, Peak b) {
    const bool take_b = b.p > a.p || (b.p == a.p && b.idx < a.idx);
    return take_b ? b : a;
}
__device__ __forceinline__ Peak wave_reduce_peak(Peak v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Peak o;
        o.p = __shfl_xor(v.p, off, 64);
        o.idx = __shfl_xor(v.idx, off, 64);
        v = peak_combine(v, o);
    }
    return v;
}

// the four waves of a workgroup, always in this order
__device__ __forceinline__ float fold4(float w0, float w1, float w2, float w3) { return (w0 + w1) + (w2 + w3); }

// One value per thread to one value per workgroup of 256, returned to every thread; sm[4] may be reused from call to call.
__device__ __forceinline__ float block_reduce_max(float v, float* sm) {
    v = wave_reduce_max(v);
    const int wid = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[wid] = v;
    __syncthreads();
    return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}
__device__ __forceinline__ float block_reduce_sum(float v, float* sm) {
    v = wave_reduce_sum(v);
    const int wid = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[wid] = v;
    __syncthreads();
    return fold4(sm[0], sm[1], sm[2], sm[3]);
}

// Four values at i .. i + 3 of a row and their coordinates from the interleaved [voxels][3] table: four 16-byte loads (i a multiple
// of 4, both bases 16-byte aligned).
struct Quad {
    f32x4 p, cx, cy, cz;   // indexed [0..3]
};
__device__ __forceinline__ Quad load_quad(const float* v, const float* coord, int i) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(v + i);
    const f32x4 c_a = *reinterpret_cast<const f32x4*>(coord + (size_t)i * 3);
    const f32x4 c_b = *reinterpret_cast<const f32x4*>(coord + (size_t)i * 3 + 4);
    const f32x4 c_c = *reinterpret_cast<const f32x4*>(coord + (size_t)i * 3 + 8);
    return Quad{x, {c_a.x, c_a.w, c_b.z, c_c.y}, {c_a.y, c_b.x, c_b.w, c_c.z}, {c_a.z, c_b.y, c_c.x, c_c.w}};
}

// Workgroup fold, first half: N per-lane sums (and a peak, in slots N and N + 1) through the butterfly into sm[wave]; ends with the
// barrier.  Second half: block_fold_sum / block_fold_peak below, by whichever threads write the record.
template <int N, int PART>
__device__ __forceinline__ void block_fold_stage(float (&acc)[N], float (*sm)[PART]) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = wave_reduce_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sm[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
}
template <int N, int PART>
__device__ __forceinline__ void block_fold_stage(float (&acc)[N], Peak pk, float (*sm)[PART]) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = wave_reduce_sum(acc[k]);
    pk = wave_reduce_peak(pk);
    if ((threadIdx.x & 63) == 0) {
        const int wid = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < N; ++k) sm[wid][k] = acc[k];
        sm[wid][N] = pk.p;
        sm[wid][N + 1] = __int_as_float(pk.idx);
    }
    __syncthreads();
}
template <int PART>
__device__ __forceinline__ float block_fold_sum(float (*sm)[PART], int k) {
    return fold4(sm[0][k], sm[1][k], sm[2][k], sm[3][k]);
}
template <int PART>
__device__ __forceinline__ Peak block_fold_peak(float (*sm)[PART], int n) {
    Peak r = {sm[0][n], __float_as_int(sm[0][n + 1])};
#pragma unroll
    for (int w = 1; w < 4; ++w) r = peak_combine(r, Peak{sm[w][n], __float_as_int(sm[w][n + 1])});
    return r;
}

// Pass 1 ends: the workgroup's N sums and its peak (PEAK_NAN when a lane saw a NaN) become the chunk's record, written by thread 0:
// the N sums, then the peak.
template <int N, int PART>
__device__ __forceinline__ void block_fold_record(float (&acc)[N], Peak pk, float (*sm)[PART], float* out) {
    block_fold_stage<N, PART>(acc, pk, sm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = block_fold_sum<PART>(sm, k);
        const Peak r = block_fold_peak<PART>(sm, N);
        out[N] = r.p;
        out[N + 1] = __int_as_float(r.idx);
    }
}

// Pass 2: the calling wave (lane = 0..63) folds the first N floats of the records first .. first + count - 1 (PART floats each) into
// acc, on every lane.
template <int N, int PART>
__device__ __forceinline__ void wave_fold_records(const float* part, size_t first, int count, int lane, float (&acc)[N]) {
    for (int k = lane; k < count; k += 64) {
        const float* p = part + (first + k) * PART;
#pragma unroll
        for (int a = 0; a < N; ++a) acc[a] += p[a];
    }
#pragma unroll
    for (int a = 0; a < N; ++a) acc[a] = wave_reduce_sum(acc[a]);
}
// The same over the `splits` chunk records of a row that row_partial wrote: empty chunks skipped by position, the peak returned.
template <int N, int PART>
__device__ __forceinline__ Peak wave_fold_chunks(const float* part, int splits, int voxels, int lane, float (&acc)[N]) {
    const int chunk = se_row_chunk(voxels, splits);
#pragma unroll
    for (int a = 0; a < N; ++a) acc[a] = 0.f;
    Peak pk = PEAK_NONE;
    for (int k = lane; k < splits; k += 64) {
        if (SE_CHUNK_EMPTY(k, chunk, voxels)) continue;   // its record holds the neutral element, skipped by position all the same
        const float* p = part + k * PART;
#pragma unroll
        for (int a = 0; a < N; ++a) acc[a] += p[a];
        pk = peak_combine(pk, Peak{p[N], __float_as_int(p[N + 1])});
    }
#pragma unroll
    for (int a = 0; a < N; ++a) acc[a] = wave_reduce_sum(acc[a]);
    return wave_reduce_peak(pk);
}
