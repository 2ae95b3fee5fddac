// The float32 3x3x3 kernels of the small pyramid levels (a few thousand voxels, 128 -> 128 channels): grid split-K with its
// reduce, in-workgroup split-K, and the 64-voxel tiles staged through LDS.  Which of them a call runs on is the plan's decision
// (se_conv3d_plan, conv3d.hip); operand maps: conv3d.hip.
#include "common.h"

#include "conv3d_plan.h"
#include "split6.h"

namespace {

// ------------------------------------------------------------------------------------------------
// split-K variant for the small pyramid levels (8^3, 4^3, 2^3: 128 -> 128 channels, a few thousand voxels).
// There the direct kernel has only a handful of workgroups, each walking all 27 x 8 steps serially
// (0.24 ms per conv, MFMA-latency-bound on <10 % of the chip).  Here grid.z splits the 27 taps, every
// (voxel tile, cout tile, tap slice) is its own workgroup writing a partial sum to the workspace, and a second
// tiny kernel adds the slices in a FIXED order (bitwise deterministic, no atomics) and applies the epilogue.
// ------------------------------------------------------------------------------------------------
// Round 5 tried ONE launch (arrival counter per tile in the workspace, the last-arriving block reduces in the same fixed order):
// with device-scope release / acquire fences it cost +50 us per launch (a cache-wide write-back / invalidate per wave, 864 blocks),
// with device-scope (sc1) stores / loads of the partials it measured EQUAL to the two launches (the reduce launches are ~4.5 us each)
// and was not bit-stable from launch to launch - not shipped (profiles/r05_fork_and_splitk_ab.txt).
template <int N_T>
__global__ __launch_bounds__(256) void conv3d_k3_splitk_kernel(ConvArgs a, float* __restrict__ ws, int taps_per_split) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int vl = lane & 15;
    const int h = lane >> 4;
    const int dim = a.dim;
    const int cgs = (a.cin + 15) >> 4;
    const int nt0 = blockIdx.y * N_T;
    const int split = blockIdx.z;

    const long long vid = ((long long)blockIdx.x * 4 + wave) * 16 + vl;
    const bool vok = vid < a.total_vox;
    long long t = vok ? vid : 0;
    const int vx = (int)(t % dim); t /= dim;
    const int vy = (int)(t % dim); t /= dim;
    const int vz = (int)(t % dim); t /= dim;
    const int vb = (int)t;

    f32x4 acc[N_T];
#pragma unroll
    for (int n = 0; n < N_T; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f32x4* wp = reinterpret_cast<const f32x4*>(a.wpack);
    const int tap0 = split * taps_per_split;
    for (int tap = tap0; tap < tap0 + taps_per_split; ++tap) {
        const int zz = vz + tap / 9 - 1, yy = vy + (tap / 3) % 3 - 1, xx = vx + tap % 3 - 1;
        const bool ok = vok && (unsigned)zz < (unsigned)dim && (unsigned)yy < (unsigned)dim && (unsigned)xx < (unsigned)dim;
        const float* src = a.in + (ok ? ((((long long)vb * dim + zz) * dim + yy) * dim + xx) * a.cin_pad + 4 * h : 0);
        // the launch is latency-bound: issue the loads of 4 channel groups (4 x (1 + N_T) x 16 B per lane) before their MFMAs
        for (int cg0 = 0; cg0 < cgs; cg0 += 4) {
            f32x4 xf[4], wf[4][N_T];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int cg = cg0 + u < cgs ? cg0 + u : cgs - 1;
                xf[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (ok && cg0 + u < cgs) xf[u] = *reinterpret_cast<const f32x4*>(src + cg * 16);
                const f32x4* wrow = wp + ((size_t)(cg * 27 + tap) * a.nts + nt0) * 64 + lane;
#pragma unroll
                for (int n = 0; n < N_T; ++n) wf[u][n] = wrow[n * 64];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int n = 0; n < N_T; ++n) {
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u][n].x, xf[u].x, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u][n].y, xf[u].y, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u][n].z, xf[u].z, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u][n].w, xf[u].w, acc[n], 0, 0, 0);
                }
            }
        }
    }
    if (!vok) return;
    float* o = ws + ((size_t)split * a.total_vox + vid) * a.cout;
#pragma unroll
    for (int n = 0; n < N_T; ++n) *reinterpret_cast<f32x4*>(o + (nt0 + n) * 16 + 4 * h) = acc[n];
}

// In-workgroup split-K for the small pyramid levels (8^3, 4^3, 2^3; 128 -> 128 channels): the WAVES waves of a workgroup share ONE
// set of N_T voxel tiles x 2 cout tiles and split the 27 x cin/16 (tap, channel group) steps between them; the partial sums meet
// in LDS in a fixed order (deterministic) and the epilogue runs in the same launch - no workspace round trip, no second kernel.
//
// Round 3: the float32 MFMA runs on the vector ALUs (64 FLOP/clk/SIMD = the VALU rate; tools/diag/mfma_selfmix.hip: one VALU
// instruction per MFMA costs 17 % of the matrix rate), so the per-step address arithmetic of the first form - tap decomposition,
// three bounds compares, 64-bit address adds and a branch per load: ~6 VALU instructions per MFMA - took as long as the MFMAs.
// Now the whole k-step walk lives in scalar registers (the wave index goes through readfirstlane), loads are raw buffer loads
// whose uniform part (tap shift, channel group, weight block) sits in the descriptor base / scalar offset, a lane's voxel offset
// is computed once, and a neighbour outside the volume is one bit of a 27-bit per-lane mask that turns the voxel offset into an
// out-of-range one (the load returns zeros; no branch): 2 VALU instructions per activation load, none per weight load.
// Loads of block i+1 (U steps) are in flight under the MFMAs of block i (two named register sets).
template <int N_T, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void conv3d_k3_wavesplit_kernel(ConvArgs a) {
    __shared__ f32x4 red[WAVES][2 * N_T][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int vl = lane & 15;
    const int h = lane >> 4;
    const int dim = a.dim;
    const int cgs = (a.cin + 15) >> 4;
    const int nt0 = blockIdx.y * 2;
    constexpr unsigned OOB = 0x80000000u;
    // per lane, once: byte offset of the voxel's record (+ this k lane's channel quad) and the mask of taps that leave the volume
    unsigned voff[N_T], bad[N_T];
#pragma unroll
    for (int n = 0; n < N_T; ++n) {
        const long long vid = ((long long)blockIdx.x * N_T + n) * 16 + vl;
        const bool vok = vid < a.total_vox;
        long long t = vok ? vid : 0;
        const int vx = (int)(t % dim); t /= dim;
        const int vy = (int)(t % dim); t /= dim;
        const int vz = (int)(t % dim);
        voff[n] = (unsigned)((vok ? vid : 0) * a.cin_pad + 4 * h) * 4u;
        unsigned m = 0;
        for (int tap = 0; tap < 27; ++tap) {
            const int zz = vz + tap / 9 - 1, yy = vy + (tap / 3) % 3 - 1, xx = vx + tap % 3 - 1;
            const bool ok = vok && (unsigned)zz < (unsigned)dim && (unsigned)yy < (unsigned)dim && (unsigned)xx < (unsigned)dim;
            m |= (ok ? 0u : 1u) << tap;
        }
        bad[n] = m;
    }
    const unsigned in_bytes = (unsigned)(a.total_vox * a.cin_pad * 4);       // launcher: total_vox <= 8192, fits 32 bits
    const unsigned w_bytes = (unsigned)(27 * cgs * a.nts * 1024);
    const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wpack), 0, (int)w_bytes, 0x00020000);
    const int woff = lane * 16;

    f32x4 acc[2][N_T];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < N_T; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int steps = 27 * cgs;
    constexpr int U = 4;
    struct Ops { f32x4 wf[U][2], xf[U][N_T]; };
    // the wave's k steps: s = wave, wave + WAVES, ...; (tap, cg) of the next step to LOAD, advanced incrementally (scalar)
    int ld_s = wave, ld_tap = wave / cgs, ld_cg = wave - (wave / cgs) * cgs;
    auto load_block = [&](Ops& o) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = ld_s < steps;                                   // uniform
            const int tap = live ? ld_tap : 0, cg = live ? ld_cg : 0;
            const int dz = tap / 9 - 1, dy = (tap / 3) % 3 - 1, dx = tap % 3 - 1;
            // activations: descriptor base = in + (tap shift, channel group); a dead step reads through a zero-record descriptor
            const float* xb = a.in + ((long long)(dz * dim + dy) * dim + dx) * a.cin_pad + cg * 16;
            const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, live ? (int)in_bytes : 0, 0x00020000);
#pragma unroll
            for (int n = 0; n < N_T; ++n) {
                const unsigned sel = (unsigned)__builtin_amdgcn_sbfe(bad[n], tap, 1);      // all ones when the tap leaves the volume
                o.xf[u][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)(voff[n] | (sel & OOB)), 0, 0));
            }
            const int wso = live ? ((cg * 27 + tap) * a.nts + nt0) * 1024 : 0;
            o.wf[u][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, woff, wso, 0));
            o.wf[u][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, woff, wso + 1024, 0));
            ld_s += WAVES;
            ld_cg += WAVES;
            while (ld_cg >= cgs) { ld_cg -= cgs; ++ld_tap; }
        }
    };
    auto mfma_block = [&](const Ops& o) {      // a dead k step carries zero activations: it adds exact zeros
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float wv[2][4] = {{o.wf[u][0].x, o.wf[u][0].y, o.wf[u][0].z, o.wf[u][0].w}, {o.wf[u][1].x, o.wf[u][1].y, o.wf[u][1].z, o.wf[u][1].w}};
#pragma unroll
            for (int c = 0; c < 4; ++c)        // component outer: consecutive MFMAs go to different accumulators
#pragma unroll
                for (int n = 0; n < N_T; ++n) {
                    const float xv[4] = {o.xf[u][n].x, o.xf[u][n].y, o.xf[u][n].z, o.xf[u][n].w};
#pragma unroll
                    for (int m = 0; m < 2; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[m][c], xv[c], acc[m][n], 0, 0, 0);
                }
        }
    };
    Ops oa, ob;
    load_block(oa);
    for (int s0 = wave; s0 < steps; s0 += 2 * U * WAVES) {
        load_block(ob);                         // beyond the last block: dead steps (zero-record descriptor, zero operands)
        mfma_block(oa);
        if (s0 + U * WAVES >= steps) break;
        load_block(oa);
        mfma_block(ob);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < N_T; ++n) red[wave][m * N_T + n][lane] = acc[m][n];
    __syncthreads();
    // 2 * N_T fragments, WAVES waves: wave w finishes fragments w, w + WAVES, ... (partials added in wave order: deterministic)
    const long long per_b = (long long)dim * dim * dim;
    for (int f = wave; f < 2 * N_T; f += WAVES) {
        const int m = f / N_T, n = f - m * N_T;
        f32x4 v = red[0][f][lane];
#pragma unroll
        for (int w2 = 1; w2 < WAVES; ++w2) v += red[w2][f][lane];
        const long long ov = ((long long)blockIdx.x * N_T + n) * 16 + vl;
        if (ov < a.total_vox) {
            const int b = (int)(ov / per_b);
            conv_epilogue(a, v, b, ov - (long long)b * per_b, per_b, (nt0 + m) * 16 + 4 * h);
        }
    }
}

// 4096-voxel levels with wide channels (8^3 at batch 8, 16^3 at batch 1; 128 -> 128): the in-workgroup split-K form above reads
// every operand of every k step straight from the vector cache - each voxel record 27 times, the weights once per 32 voxels:
// 442 MB of cache traffic per launch, 30 of its 45 us with the MFMAs knocked out (round 5, profiles/r05_small_levels.txt).
// This form stages the activations through LDS and shares a weight fragment between four voxel tiles:
//   workgroup = 64 consecutive voxels (whole rows: one z slab at dim 8, four rows at dim 16) x 32 couts, 8 waves;
//   per 32-channel stage the 3 x (R+2) x (DIM+2) halo of the tile is staged once (raw buffer loads, a voxel outside the volume
//   reads zeros through an out-of-range offset; global -> registers under the previous stage's MFMAs -> LDS, two buffers, one
//   barrier per stage); a halo voxel takes 144 bytes of LDS (128 + 16 pad: every 8 lanes of a ds_read_b128 cover the 32 banks);
//   the 54 (tap, 16-channel group) k steps of a stage are dealt to the waves (step = wave + 8 j: 7, 7, 7, 7, 7, 7, 6, 6); a k step
//   = 2 weight fragments (global; the whole next stage's seven steps in flight in a register ring) + 4 ds_read_b128 + 32 MFMAs;
//   the waves' partial sums meet in LDS in wave order (deterministic) and the epilogue runs in the same launch, its bias and
//   skip-tensor loads issued ahead of the last stage's MFMAs.
template <int DIM>
struct Halo64 {
    static constexpr int R = 64 / DIM;                // rows of a tile
    static constexpr int HX = DIM + 2, HY = R + 2;
    static constexpr int HV = 3 * HY * HX;            // halo voxels: 300 (dim 8) / 324 (dim 16)
    static constexpr int PITCH = 144;
    static constexpr int HB = HV * PITCH;
    static constexpr int PIECES = HV * 8;             // 16-byte pieces of a stage
    static constexpr int HP = (PIECES + 511) / 512;
    static constexpr int MT_OFF = (16 / DIM) * HX * PITCH;   // LDS bytes between consecutive voxel tiles (16 voxels = 16 / DIM rows)
    static constexpr int LDS_BYTES = 2 * HB > 65536 ? 2 * HB : 65536;
};

template <int DIM>
__global__ __launch_bounds__(512) void conv3d_k3_halo64_kernel(ConvArgs a) {
    using G = Halo64<DIM>;
    constexpr int HX = G::HX, HY = G::HY, PITCH = G::PITCH, HP = G::HP;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int vl = lane & 15, h = lane >> 4;
    const int stages = a.cin >> 5;
    const int nt0 = blockIdx.y * 2;
    constexpr unsigned OOB = 0x80000000u;
    int t = blockIdx.x;
    const int ty = t % (DIM / G::R); t /= (DIM / G::R);
    const int z = t % DIM;
    const int b = t / DIM;
    const int y0 = ty * G::R;
    const long long vid0 = (((long long)b * DIM + z) * DIM + y0) * DIM;       // the tile's 64 voxels are consecutive in memory

    // this thread's halo pieces: byte offset in the input tensor (out of range for a voxel outside the volume) - fixed over the stages
    unsigned goff[HP];
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        const int p = tid + 512 * j;
        const int hv = p >> 3, q = p & 7;
        const int hx = hv % HX, hy = (hv / HX) % HY, hz = hv / (HX * HY);
        const int gz = z + hz - 1, gy = y0 + hy - 1, gx = hx - 1;
        const bool ok = p < G::PIECES && (unsigned)gz < (unsigned)DIM && (unsigned)gy < (unsigned)DIM && (unsigned)gx < (unsigned)DIM;
        goff[j] = ok ? (unsigned)(((((long long)b * DIM + gz) * DIM + gy) * DIM + gx) * a.cin_pad * 4 + q * 16) : OOB;
    }
    const int lpiece = (tid >> 3) * PITCH + (tid & 7) * 16;                   // piece j: + j * 64 * PITCH
    const unsigned in_bytes = (unsigned)(a.total_vox * a.cin_pad * 4);        // launcher: fits 31 bits
    const unsigned w_bytes = (unsigned)(27 * (a.cin >> 4) * a.nts * 1024);
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, (int)in_bytes, 0x00020000);
    const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wpack), 0, (int)w_bytes, 0x00020000);
    const int woff = lane * 16;
    // operand reads: lane (vl, h) = voxel vl of the tile's first 16, channels 4 h .. 4 h + 3, at the tap (-1, -1, -1) corner
    const int lrow = DIM == 8 ? (vl >> 3) : 0, lx = DIM == 8 ? (vl & 7) : vl;
    const int lbase = (lrow * HX + lx) * PITCH + h * 16;

    f32x4 st[HP];
    auto load_stage = [&](int sg) {
#pragma unroll
        for (int j = 0; j < HP; ++j) st[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)goff[j], sg * 128, 0));
    };
    auto commit_stage = [&](unsigned char* buf) {
#pragma unroll
        for (int j = 0; j < HP; ++j)
            if (tid + 512 * j < G::PIECES) *reinterpret_cast<f32x4*>(buf + lpiece + j * 64 * PITCH) = st[j];
    };
    f32x4 wr[7][2];
    auto load_w = [&](int j, int sg) {                 // slot j of stage sg: step wave + 8 j = (tap, group); slot 6 of waves 6, 7: dead, never used
        const int step = wave + 8 * j;
        const int tap = step >> 1, cg = sg * 2 + (step & 1);
        const int wso = step < 54 ? ((cg * 27 + tap) * a.nts + nt0) * 1024 : 0;
        wr[j][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, woff, wso, 0));
        wr[j][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, woff, wso + 1024, 0));
    };
    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // the epilogue's operands (wave w finishes fragment w = (cout tile w >> 2, voxel tile w & 3))
    const long long per_b = (long long)DIM * DIM * DIM;
    const int co0 = (nt0 + (wave >> 2)) * 16 + 4 * h;
    const long long ooff = (vid0 + (wave & 3) * 16 + vl) * a.cout + co0;
    f32x4 ebias = (f32x4){0.f, 0.f, 0.f, 0.f}, eres = (f32x4){0.f, 0.f, 0.f, 0.f};

    load_stage(0);
#pragma unroll
    for (int j = 0; j < 7; ++j) load_w(j, 0);
    for (int sg = 0; sg < stages; ++sg) {
        unsigned char* buf = lds + (sg & 1) * G::HB;
        commit_stage(buf);
        __syncthreads();          // the stage is in LDS; every wave has left the stage before the previous one (the buffer written next)
        const bool more = sg + 1 < stages;
        if (more) {
            load_stage(sg + 1);
        } else {
            ebias = *reinterpret_cast<const f32x4*>(a.bpack + co0);
            if (a.res) eres = *reinterpret_cast<const f32x4*>(a.res + ooff);
        }
        f32x4 xf[2][4];
        auto read_x = [&](f32x4 (&x)[4], int j) {
            int step = wave + 8 * j;
            step = step < 54 ? step : 53;
            const int tap = step >> 1;
            const int toff = (((tap / 9) * HY + (tap / 3) % 3) * HX + tap % 3) * PITCH + (step & 1) * 64;     // wave-uniform
            const unsigned char* p = buf + lbase + toff;
#pragma unroll
            for (int n = 0; n < 4; ++n) x[n] = *reinterpret_cast<const f32x4*>(p + n * G::MT_OFF);
        };
        read_x(xf[0], 0);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            if (j + 1 < 7) read_x(xf[(j + 1) & 1], j + 1);
            if (wave + 8 * j < 54) {                   // uniform
                const f32x4(&x)[4] = xf[j & 1];
                const float wv[2][4] = {{wr[j][0].x, wr[j][0].y, wr[j][0].z, wr[j][0].w}, {wr[j][1].x, wr[j][1].y, wr[j][1].z, wr[j][1].w}};
#pragma unroll
                for (int c = 0; c < 4; ++c)            // component outer: consecutive MFMAs go to different accumulators
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const float xv[4] = {x[n].x, x[n].y, x[n].z, x[n].w};
#pragma unroll
                        for (int m = 0; m < 2; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[m][c], xv[c], acc[m][n], 0, 0, 0);
                    }
            }
            if (more) load_w(j, sg + 1);               // the slot's registers are free: next stage's weights, seven steps ahead
        }
    }
    __syncthreads();              // every wave is done with the halo buffers: the partial sums go on top of them
    f32x4(*red)[8][64] = reinterpret_cast<f32x4(*)[8][64]>(lds);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) red[wave][m * 4 + n][lane] = acc[m][n];
    __syncthreads();
    f32x4 v = red[0][wave][lane];                      // partials added in wave order
#pragma unroll
    for (int w2 = 1; w2 < 8; ++w2) v += red[w2][wave][lane];
    v += ebias;
    if ((a.flags & SE_EPI_RES_PRE_RELU) && a.res) v += eres;
    if (a.flags & SE_EPI_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    if ((a.flags & SE_EPI_RES_POST_RELU) && a.res) v += eres;
    *reinterpret_cast<f32x4*>(a.out + ooff) = v;
    (void)per_b;
}

// The split form of the kernel above (split6.h: a float32 product as six bf16 products on v_mfma_f32_16x16x32_bf16): same tiles,
// stages, wave roles, reduction and epilogue; what changes is the k step and the operands.
//   A k step is one TAP over the stage's 32 channels (K = 32 of one MFMA): 27 steps per stage, step = wave + 8 j (4, 4, 4, 3, 3, 3,
//   3, 3 per wave; waves w and w + 4 share a SIMD: 7, 7, 7, 6 steps per SIMD), 48 MFMAs each (6 products x 2 cout x 4 voxel tiles).
//   Activations are split ONCE, when the stage is committed: a thread loads 8 channels of a halo voxel (two 16-byte loads) and
//   writes its three bf16 planes, [plane 3][octet 4][16 B] per voxel = 192 of a 224-byte record (6 B per element instead of 4; the
//   pitch leaves the 16 lanes of a ds_read_b128 group on 16 different 16-byte slots at dim 16, two per slot at dim 8).
//   Weights are the layer's split planes (conv3d_pack.h), [stage][tap][nt][plane][lane] x 16 B: 6 loads per step, two steps in
//   flight in a register ring (slot j & 1; a step's 48 MFMAs cover the next one's loads).
template <int DIM>
struct Halo64S6 {
    using F = Halo64<DIM>;
    static constexpr int PITCH = 224;
    static constexpr int HB = F::HV * PITCH;
    static constexpr int PIECES = F::HV * 4;          // (voxel, channel octet) pieces of a stage: 1200 (dim 8) / 1296 (dim 16)
    static constexpr int HP = (PIECES + 511) / 512;
    static constexpr int MT_OFF = (16 / DIM) * F::HX * PITCH;
    static constexpr int LDS_BYTES = 2 * HB > 65536 ? 2 * HB : 65536;
    static_assert(LDS_BYTES <= 160 * 1024, "two stage buffers in LDS");
};

template <int DIM>
__global__ __launch_bounds__(512) void conv3d_k3_halo64_s6_kernel(ConvArgs a) {
    using G = Halo64<DIM>;
    using S = Halo64S6<DIM>;
    constexpr int HX = G::HX, HY = G::HY, PITCH = S::PITCH, HP = S::HP;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int vl = lane & 15, h = lane >> 4;
    const int stages = a.cin >> 5;
    const int nt0 = blockIdx.y * 2;
    constexpr unsigned OOB = 0x80000000u;
    int t = blockIdx.x;
    const int ty = t % (DIM / G::R); t /= (DIM / G::R);
    const int z = t % DIM;
    const int b = t / DIM;
    const int y0 = ty * G::R;
    const long long vid0 = (((long long)b * DIM + z) * DIM + y0) * DIM;

    // this thread's halo pieces (voxel hv, channel octet q): byte offset in the input tensor, out of range outside the volume
    unsigned goff[HP];
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        const int p = tid + 512 * j;
        const int hv = p >> 2, q = p & 3;
        const int hx = hv % HX, hy = (hv / HX) % HY, hz = hv / (HX * HY);
        const int gz = z + hz - 1, gy = y0 + hy - 1, gx = hx - 1;
        const bool ok = p < S::PIECES && (unsigned)gz < (unsigned)DIM && (unsigned)gy < (unsigned)DIM && (unsigned)gx < (unsigned)DIM;
        goff[j] = ok ? (unsigned)(((((long long)b * DIM + gz) * DIM + gy) * DIM + gx) * a.cin_pad * 4 + q * 32) : OOB;
    }
    const int lpiece = (tid >> 2) * PITCH + (tid & 3) * 16;                   // piece j: + j * 128 * PITCH; plane k: + 64 k
    const unsigned in_bytes = (unsigned)(a.total_vox * a.cin_pad * 4);        // launcher: fits 31 bits
    const unsigned w_bytes = (unsigned)(27 * (a.cin_pad >> 5) * a.nts * 3072);
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, (int)in_bytes, 0x00020000);
    const auto wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(a.wsplit6), 0, (int)w_bytes, 0x00020000);
    const int woff = lane * 16;
    // operand reads: lane (vl, h) = voxel vl of the tile's first 16, channels 8 h .. 8 h + 7 of the stage, at the tap (-1, -1, -1) corner
    const int lrow = DIM == 8 ? (vl >> 3) : 0, lx = DIM == 8 ? (vl & 7) : vl;
    const int lbase = (lrow * HX + lx) * PITCH + h * 16;

    f32x4 st[HP][2];
    auto load_stage = [&](int sg) {
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            st[j][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)goff[j], sg * 128, 0));
            st[j][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)(goff[j] + 16u), sg * 128, 0));
        }
    };
    auto commit_stage = [&](unsigned char* buf) {
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            const Split6Frag f = se_split3_x8(st[j][0], st[j][1]);
            if (tid + 512 * j < S::PIECES) {
#pragma unroll
                for (int k = 0; k < 3; ++k) *reinterpret_cast<u16x8*>(buf + lpiece + j * 128 * PITCH + k * 64) = f.p[k];
            }
        }
    };
    Split6Frag wr[2][2];
    auto load_w = [&](Split6Frag (&w)[2], int j, int sg) {      // step wave + 8 j of stage sg; a step past the 27 taps is dead: nothing loaded
        const int tap = wave + 8 * j;
        if (tap >= 27) return;                         // uniform
        const int wso = ((sg * 27 + tap) * a.nts + nt0) * 3072;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                w[m].p[k] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, woff, wso + (m * 3 + k) * 1024, 0));
    };
    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // the epilogue's operands (wave w finishes fragment w = (cout tile w >> 2, voxel tile w & 3))
    const int co0 = (nt0 + (wave >> 2)) * 16 + 4 * h;
    const long long ooff = (vid0 + (wave & 3) * 16 + vl) * a.cout + co0;
    f32x4 ebias = (f32x4){0.f, 0.f, 0.f, 0.f}, eres = (f32x4){0.f, 0.f, 0.f, 0.f};

    load_stage(0);
    load_w(wr[0], 0, 0);
    load_w(wr[1], 1, 0);
    for (int sg = 0; sg < stages; ++sg) {
        unsigned char* buf = lds + (sg & 1) * S::HB;
        commit_stage(buf);
        __syncthreads();          // the stage is in LDS; every wave has left the stage before the previous one (the buffer written next)
        const bool more = sg + 1 < stages;
        if (more) {
            load_stage(sg + 1);
        } else {
            ebias = *reinterpret_cast<const f32x4*>(a.bpack + co0);
            if (a.res) eres = *reinterpret_cast<const f32x4*>(a.res + ooff);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int tap = wave + 8 * j;
            if (tap < 27) {                            // uniform
                const int toff = (((tap / 9) * HY + (tap / 3) % 3) * HX + tap % 3) * PITCH;
                const unsigned char* p = buf + lbase + toff;
                Split6Frag x[4];
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int k = 0; k < 3; ++k) x[n].p[k] = *reinterpret_cast<const u16x8*>(p + n * S::MT_OFF + k * 64);
                const Split6Frag(&w)[2] = wr[j & 1];
#pragma unroll
                for (int k = 0; k < SE_S6_PRODUCTS; ++k)   // product outer: consecutive MFMAs go to different accumulators
#pragma unroll
                    for (int n = 0; n < 4; ++n)
#pragma unroll
                        for (int m = 0; m < 2; ++m) acc[m][n] = mfma_bf16(w[m].p[SE_S6_W[k]], x[n].p[SE_S6_X[k]], acc[m][n]);
            }
            // the slot's registers are free: the step two ahead (this stage's, then the next stage's first two)
            if (j + 2 < 4) load_w(wr[j & 1], j + 2, sg);
            else if (more) load_w(wr[j & 1], j - 2, sg + 1);
        }
    }
    __syncthreads();              // every wave is done with the halo buffers: the partial sums go on top of them
    f32x4(*red)[8][64] = reinterpret_cast<f32x4(*)[8][64]>(lds);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) red[wave][m * 4 + n][lane] = acc[m][n];
    __syncthreads();
    f32x4 v = red[0][wave][lane];                      // partials added in wave order
#pragma unroll
    for (int w2 = 1; w2 < 8; ++w2) v += red[w2][wave][lane];
    v += ebias;
    if ((a.flags & SE_EPI_RES_PRE_RELU) && a.res) v += eres;
    if (a.flags & SE_EPI_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    if ((a.flags & SE_EPI_RES_POST_RELU) && a.res) v += eres;
    *reinterpret_cast<f32x4*>(a.out + ooff) = v;
}

// thread = (voxel, cout quad): sum the split partials in order, then the usual epilogue
__global__ __launch_bounds__(256) void splitk_reduce_kernel(ConvArgs a, const float* __restrict__ ws, int splits) {
    const int cq = a.cout >> 2;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.total_vox * cq) return;
    const long long vid = t / cq;
    const int q = (int)(t - vid * cq);
    // all partials requested before the first add (splits is 3, 9 or 27; the sum keeps its fixed order): the kernel is pure load
    // latency, one dependent round trip per split otherwise
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const float* p0 = ws + vid * a.cout + q * 4;
    const size_t sstride = (size_t)a.total_vox * a.cout;
    for (int s0 = 0; s0 < splits; s0 += 9) {
        f32x4 part[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) part[u] = (s0 + u < splits) ? *reinterpret_cast<const f32x4*>(p0 + (size_t)(s0 + u) * sstride) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 9; ++u) v += part[u];
    }
    const long long per_b = (long long)a.dim * a.dim * a.dim;
    const int b = (int)(vid / per_b);
    conv_epilogue(a, v, b, vid - (long long)b * per_b, per_b, q * 4);
}

}  // namespace

// The plan has checked: 3^3, channels-last tensors, an even number of cout tiles, no planar output; halo64 / in-workgroup split-K:
// at most 8192 voxels and 32-bit byte offsets into the input, halo64 also dim 8 or 16 and cin % 32 == 0; grid split-K: a workspace of
// p.splits * total_vox * cout floats.
int se_conv3d_small_launch(const ConvArgs& a, const SeConvPlan& p, hipStream_t s) {
    const long long tiles = (a.total_vox + 15) / 16;
    switch (p.kernel) {
        case SE_CONV_HALO64: {   // 64-voxel tiles, activations through LDS
            const dim3 grid((unsigned)(a.total_vox / 64), a.nts / 2);
            if (p.form == 8) {
                SE_ENSURE_LDS(conv3d_k3_halo64_kernel<8>, Halo64<8>::LDS_BYTES);
                hipLaunchKernelGGL((conv3d_k3_halo64_kernel<8>), grid, dim3(512), Halo64<8>::LDS_BYTES, s, a);
            } else {
                SE_ENSURE_LDS(conv3d_k3_halo64_kernel<16>, Halo64<16>::LDS_BYTES);
                hipLaunchKernelGGL((conv3d_k3_halo64_kernel<16>), grid, dim3(512), Halo64<16>::LDS_BYTES, s, a);
            }
            break;
        }
        case SE_CONV_HALO64_S6: {   // the same tiles, six-product bf16 form (the plan has checked se_conv3d_halo64_s6_domain and a.wsplit6)
            const dim3 grid((unsigned)(a.total_vox / 64), a.nts / 2);
            if (p.form == 8) {
                SE_ENSURE_LDS(conv3d_k3_halo64_s6_kernel<8>, Halo64S6<8>::LDS_BYTES);
                hipLaunchKernelGGL((conv3d_k3_halo64_s6_kernel<8>), grid, dim3(512), Halo64S6<8>::LDS_BYTES, s, a);
            } else {
                SE_ENSURE_LDS(conv3d_k3_halo64_s6_kernel<16>, Halo64S6<16>::LDS_BYTES);
                hipLaunchKernelGGL((conv3d_k3_halo64_s6_kernel<16>), grid, dim3(512), Halo64S6<16>::LDS_BYTES, s, a);
            }
            break;
        }
        case SE_CONV_WAVESPLIT:
            if (p.form == 4) hipLaunchKernelGGL((conv3d_k3_wavesplit_kernel<2, 4>), dim3((unsigned)((tiles + 1) / 2), a.nts / 2), dim3(256), 0, s, a);
            else if (p.form == 8) hipLaunchKernelGGL((conv3d_k3_wavesplit_kernel<1, 8>), dim3((unsigned)tiles, a.nts / 2), dim3(512), 0, s, a);
            else hipLaunchKernelGGL((conv3d_k3_wavesplit_kernel<1, 16>), dim3((unsigned)tiles, a.nts / 2), dim3(1024), 0, s, a);
            break;
        case SE_CONV_SPLITK_GRID: {
            hipLaunchKernelGGL((conv3d_k3_splitk_kernel<2>), dim3((unsigned)((a.total_vox + 63) / 64), a.nts / 2, p.splits), dim3(256), 0, s, a, a.ws,
                               27 / p.splits);
            SE_CHECK_LAUNCH();
            const long long threads = a.total_vox * (a.cout / 4);
            hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a, a.ws, p.splits);
            break;
        }
        default: return SE_ERR_BAD_ARG;
    }
    SE_CHECK_LAUNCH();
    return 0;
}
