// Baseline JPEG frames decoded on the device: the restart segments of any number of same-sized files -> uint8 B, G, R.
//
// Stands in for PIL's decode in sceneego_amd/preprocess.py load_image_bgr (libjpeg-turbo with its defaults): ISLOW IDCT (jidctint.c),
// libjpeg v6b fancy upsampling for h2v1 / h2v2 (jdsample.c; box replication when the chroma plane has at most 2 columns, as
// libjpeg-turbo selects it), jdmainct.c's repeated edge rows and jdcolor.c's fixed-point YCbCr -> RGB.  It is bit-identical to PIL on
// every file whose blocks are all *plain*: every dequantised coefficient and every pass-1 workspace value fits int16 and every
// pass-2 value after its descale (before the +128) lies in [-512, 511].  Outside that domain libjpeg-turbo's SIMD IDCT (int16 lanes,
// saturating packs) and jidctint.c's C code (64-bit sums, a wrapping range-limit table), which this file follows, part ways: such a
// block is reported as status 4 in its segment's entry and sceneego_amd/jpeg_device.py decodes the file with PIL instead, as it does
// for any file with a non-zero status.  Ordinary files are far inside (tests/test_jpeg_craft_host.py: the margin test).
//
// The entropy-coded data of a segment (between RSTn markers, unstuffed on the host) is one serial bit stream.  It is decoded in
// parallel by self-synchronisation (Weissenberger & Schmidt, ICPP 2018): every segment is cut into lanes of JPEG_LANE_BITS bits,
// one per thread.  A decoder state at a codeword boundary is (bit offset p, block k of the MCU, coefficient index z); k and z pick
// the DC or AC table.  A lane decodes the codewords that start inside its bits and records its exit state.
//
//   se_jpeg_sync_intra_kernel   speculative pass (lane j starts at its first bit as (k=0, z=0); a segment's first lane starts at
//                               the segment's true state), then rounds in LDS: a lane whose entry differs from its predecessor's exit
//                               re-decodes from that exit, until no lane of the workgroup changes.
//   se_jpeg_sync_inter_kernel   launched `rounds` times: a workgroup whose first lane's entry differs from its predecessor
//                               workgroup's last exit (a snapshot of the previous launch) re-decodes and re-runs the LDS rounds;
//                               every other workgroup exits at once.  No workgroup waits on another (no grid-wide spin).
//   se_jpeg_sync_repair_kernel  one thread per segment walks its workgroup boundaries in order and re-decodes lanes until an exit
//                               matches: afterwards every lane holds its true entry state, whatever the number of rounds.
//   se_jpeg_scan_kernel, se_jpeg_scan_top_kernel
//                               exclusive scan of the lanes' DC-code counts -> the first block each lane writes.
//   se_jpeg_write_kernel        every lane re-decodes from its true entry and scatters coefficients (natural order, DC as its
//                               difference) into the zero-filled int16 [blocks][64] scratch; a segment stops at exactly its block
//                               count; the lane that meets a bad code or the end of the bits reports it.
//   se_jpeg_dc_kernel           DC prediction: running sum of the differences per (segment, component) in MCU order.
//   se_jpeg_idct_kernel         dequantisation + ISLOW IDCT, 8 threads per block, into per-component uint8 planes (padded MCU grid);
//                               a block that is not plain (above) sets status 4 in its segment's entry unless a code is there already.
//   se_jpeg_color_kernel        upsampling + YCbCr -> B, G, R (gray: B = G = R = Y), cropped to the image.
//
// Bounds: every segment and image descriptor is checked on the device against payload_bytes and the scratch layout before use
// (status 1 otherwise); bit reads stay inside the segment's slot of the payload ((len + 3) & ~3) + 8 bytes, bits past its length
// are never consumed; Huffman value indices are range-checked.
#include "common.h"

#define JPEG_LANE_BITS 128        // bits per lane (sceneego_amd/jpeg_device.py LANE_BITS)
#define JPEG_WG 256               // lanes per workgroup of the synchronisation kernels
#define JPEG_ROUNDS 3             // default inter-workgroup synchronisation launches
#define JPEG_TABLE_BYTES 1536
#define JPEG_LOOKAHEAD 9

#define SE_JPEG_OK 0
#define SE_JPEG_BAD_DESC 1
#define SE_JPEG_NO_CODE 2         // value: bit offset in the segment
#define SE_JPEG_STREAM_END 3      // value: blocks completed
#define SE_JPEG_NOT_PLAIN 4       // value: a block of the segment (counted from the segment's first) outside the plain domain

#define ST_ERR (1ull << 16)
#define ST_END (1ull << 17)
#define ST_DEAD 0xFFFFFFFF00010000ull     // exit of a lane whose entry was a stopped state

namespace {

struct SegDesc {                  // int64[8] per segment, see include/sceneego_hip.h
    long long off, len, img, mcu0, mcus, lane0, lanes, block0;
};

struct Ctx {
    const uint8_t* payload;
    long long payload_bytes;
    const int* imgs;              // int32 [n_images][64]
    int n_images;
    const SegDesc* segs;
    int n_segs;
    const uint8_t* tables;        // [n_images][8][JPEG_TABLE_BYTES]
    long long blocks, lanes, plane_bytes;
};

__device__ __forceinline__ const int* img_row(const Ctx& c, int i) { return c.imgs + 64 * i; }

__device__ bool img_ok(const Ctx& c, int i) {
    if (i < 0 || i >= c.n_images) return false;
    const int* d = img_row(c, i);
    const int W = d[0], H = d[1], nc = d[2], mx = d[3], my = d[4], bpm = d[5];
    if (W <= 0 || H <= 0 || (nc != 1 && nc != 3) || mx <= 0 || my <= 0 || bpm < 1 || bpm > 10) return false;
    const int hmax = d[9], vmax = d[10];
    if (hmax < 1 || hmax > 2 || vmax < 1 || vmax > 2) return false;
    if ((long long)mx * 8 * hmax < W || (long long)my * 8 * vmax < H) return false;
    if (d[36] < 0 || (long long)d[36] + (long long)mx * my * bpm > c.blocks) return false;
    int nb = 0;
    for (int f = 0; f < nc; ++f) {
        const int h = d[12 + f], v = d[15 + f];
        if (h < 1 || h > hmax || v < 1 || v > vmax || d[21 + f] < 0 || d[21 + f] > 3 || d[24 + f] < 4 || d[24 + f] > 7) return false;
        if (d[27 + f] != 8 * h * mx || d[30 + f] != 8 * v * my || d[33 + f] < 0 || d[33 + f] + h * v > bpm) return false;
        if (d[37 + f] < 0 || (long long)d[37 + f] + (long long)d[27 + f] * d[30 + f] > c.plane_bytes) return false;
        nb += h * v;
    }
    if (nb != bpm) return false;
    for (int k = 0; k < bpm; ++k)
        if (d[40 + k] < 0 || d[40 + k] >= nc) return false;
    return true;
}

__device__ bool seg_ok(const Ctx& c, const SegDesc& s) {
    if (s.img < 0 || s.img >= c.n_images || !img_ok(c, (int)s.img)) return false;
    const int* d = img_row(c, (int)s.img);
    const long long nmcu = (long long)d[3] * d[4];
    if (s.len < 0 || s.off < 0 || (s.off & 3) || s.len > (1ll << 28) || s.off + ((s.len + 3) & ~3ll) + 8 > c.payload_bytes) return false;
    if (s.mcu0 < 0 || s.mcus < 1 || s.mcu0 + s.mcus > nmcu) return false;
    if (s.lane0 < 0 || s.lanes < 1 || s.lane0 + s.lanes > c.lanes) return false;
    if (s.lanes != (8 * s.len + JPEG_LANE_BITS - 1) / JPEG_LANE_BITS + (s.len == 0)) return false;
    return s.block0 == d[36] + s.mcu0 * d[5] && s.block0 + s.mcus * d[5] <= c.blocks;
}

// the segment holding lane `lane` (segments are ordered by lane0)
__device__ int find_seg(const Ctx& c, long long lane) {
    int lo = 0, hi = c.n_segs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.segs[mid].lane0 <= lane) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long pack(long long p, int k, int z) {
    return ((unsigned long long)(uint32_t)p << 32) | ((unsigned long long)k << 8) | (unsigned long long)z;
}

// one segment's decode context: its bits, its image's block -> table maps
struct Dec {
    const uint32_t* words;        // the segment's slot, 4-byte aligned
    long long nbits;
    const uint8_t* tab;           // the image's 8 tables
    uint32_t kmap;                // 2 bits per block k: component
    uint32_t dcmap, acmap;        // 2 bits per component: DC table, AC table (0..3)
    int bpm;
};

__device__ __forceinline__ Dec make_dec(const Ctx& c, const SegDesc& s) {
    Dec d;
    const int* im = img_row(c, (int)s.img);
    d.words = reinterpret_cast<const uint32_t*>(c.payload + s.off);
    d.nbits = 8 * s.len;
    d.tab = c.tables + (long long)s.img * 8 * JPEG_TABLE_BYTES;
    d.bpm = im[5];
    d.kmap = 0;
    for (int k = 0; k < d.bpm; ++k) d.kmap |= (uint32_t)im[40 + k] << (2 * k);
    d.dcmap = d.acmap = 0;
    for (int f = 0; f < im[2]; ++f) {
        d.dcmap |= (uint32_t)im[21 + f] << (2 * f);
        d.acmap |= (uint32_t)(im[24 + f] - 4) << (2 * f);
    }
    return d;
}

// 32 bits of the stream from bit p (p < nbits + 32; the slot's padding words are zero)
__device__ __forceinline__ uint32_t peek32(const Dec& d, long long p) {
    const long long w = p >> 5;
    const unsigned long long hi = __builtin_bswap32(d.words[w]), lo = __builtin_bswap32(d.words[w + 1]);
    return (uint32_t)((((hi << 32) | lo) << (p & 31)) >> 32);
}

// One codeword (code + extra bits) from (p, k, z).  Returns the new state or a stopped state (ST_ERR: no code matches, ST_END: the
// code or its bits run past the segment).  *val / *pos: the coefficient and its natural index (pos 0: a DC difference), pos -1 none.
__device__ __forceinline__ unsigned long long step(const Dec& d, unsigned long long st, int* val, int* pos) {
    long long p = (long long)(st >> 32);
    int k = (int)((st >> 8) & 0xFF), z = (int)(st & 0xFF);
    const int f = (d.kmap >> (2 * k)) & 3;
    const int slot = z == 0 ? ((d.dcmap >> (2 * f)) & 3) : 4 + ((d.acmap >> (2 * f)) & 3);
    const uint8_t* t = d.tab + slot * JPEG_TABLE_BYTES;
    const uint32_t bits = peek32(d, p);
    uint32_t e = reinterpret_cast<const uint16_t*>(t)[bits >> (32 - JPEG_LOOKAHEAD)];
    int ln, sym;
    if (e) {
        ln = (int)(e >> 8);
        sym = (int)(e & 255);
    } else {
        const int* maxcode = reinterpret_cast<const int*>(t + 1024);
        const int* valoff = reinterpret_cast<const int*>(t + 1096);
        const int code16 = (int)(bits >> 16);
        ln = JPEG_LOOKAHEAD + 1;
        while (ln <= 16 && (code16 >> (16 - ln)) > maxcode[ln]) ++ln;
        if (ln > 16) return (st & 0xFFFFFFFF0000FFFFull) | ST_ERR;
        const int idx = (code16 >> (16 - ln)) + valoff[ln];
        if (idx < 0 || idx > 255) return (st & 0xFFFFFFFF0000FFFFull) | ST_ERR;
        sym = t[1168 + idx];
    }
    const int s = z == 0 ? sym : (sym & 15);
    if (s > 15) return (st & 0xFFFFFFFF0000FFFFull) | ST_ERR;
    if (p + ln + s > d.nbits) return (st & 0xFFFFFFFF0000FFFFull) | ST_END;
    int v = 0;
    if (s) {
        v = (int)((bits << ln) >> (32 - s));          // ln + s <= 31
        if (v < (1 << (s - 1))) v += 1 - (1 << s);
    }
    p += ln + s;
    *pos = -1;
    if (z == 0) {
        *val = v;
        *pos = 0;
        z = 1;
    } else {
        const int run = sym >> 4;
        if (s) {
            z += run;
            *val = v;
            *pos = z;             // zigzag index (<= 78); the caller maps it through the natural order with guard entries
            z += 1;
        } else if (run == 15) {
            z += 16;
        } else {
            z = 64;
        }
    }
    if (z >= 64) {
        z = 0;
        if (++k == d.bpm) k = 0;
    }
    return pack(p, k, z);
}

__device__ __forceinline__ bool stopped(unsigned long long st) { return (st & (ST_ERR | ST_END)) != 0; }

// decode from `st` while the position is before `end` -> exit state; *count = DC codes decoded
__device__ unsigned long long run_lane(const Dec& d, unsigned long long st, long long end, int* count) {
    int n = 0;
    if (stopped(st)) { *count = 0; return ST_DEAD; }
    while ((long long)(st >> 32) < end) {
        const bool dc = (st & 0xFF) == 0;
        int val, pos;
        const unsigned long long nx = step(d, st, &val, &pos);
        if (stopped(nx)) { *count = n; return nx; }
        n += dc;
        st = nx;
    }
    *count = n;
    return st;
}

__device__ __forceinline__ long long lane_start(const SegDesc& s, long long lane) { return (lane - s.lane0) * JPEG_LANE_BITS; }
__device__ __forceinline__ long long lane_end(const SegDesc& s, long long lane) {
    const long long e = lane_start(s, lane) + JPEG_LANE_BITS;
    return e < 8 * s.len ? e : 8 * s.len;
}

// LDS rounds: lanes whose entry differs from the predecessor's exit re-decode until nothing changes in the workgroup
__device__ void chain(unsigned long long* ex, bool active, bool first, const Dec& dec, long long end,
                      unsigned long long& en, unsigned long long& my_ex, int& cnt) {
    const int tid = threadIdx.x;
    for (;;) {
        const unsigned long long pred = tid > 0 ? ex[tid - 1] : 0;
        const bool need = active && !first && tid > 0 && pred != en;
        if (!__syncthreads_or(need)) break;
        if (need) {
            en = pred;
            my_ex = run_lane(dec, en, end, &cnt);
        }
        __syncthreads();
        if (need) ex[tid] = my_ex;
        __syncthreads();
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JPEG_WG) se_jpeg_sync_intra_kernel(Ctx c, unsigned long long* __restrict__ entry,
                                                                     unsigned long long* __restrict__ exitv, int* __restrict__ cnt,
                                                                     unsigned long long* __restrict__ snap) {
    __shared__ unsigned long long ex[JPEG_WG];
    const long long lane = (long long)blockIdx.x * JPEG_WG + threadIdx.x;
    bool active = lane < c.lanes;
    SegDesc s{};
    if (active) {
        s = c.segs[find_seg(c, lane)];
        active = lane >= s.lane0 && lane < s.lane0 + s.lanes && seg_ok(c, s);
    }
    const bool first = active && lane == s.lane0;
    Dec dec{};
    unsigned long long en = ST_DEAD, my_ex = ST_DEAD;
    int n = 0;
    long long end = 0;
    if (active) {
        dec = make_dec(c, s);
        end = lane_end(s, lane);
        en = pack(lane_start(s, lane), 0, 0);
        my_ex = run_lane(dec, en, end, &n);
    }
    ex[threadIdx.x] = my_ex;
    __syncthreads();
    chain(ex, active, first, dec, end, en, my_ex, n);
    if (lane < c.lanes) {
        entry[lane] = en;
        exitv[lane] = my_ex;
        cnt[lane] = n;
    }
    const long long last = (long long)blockIdx.x * JPEG_WG + JPEG_WG - 1;
    if (lane == (last < c.lanes ? last : c.lanes - 1)) snap[blockIdx.x] = my_ex;
}

__global__ void __launch_bounds__(JPEG_WG) se_jpeg_sync_inter_kernel(Ctx c, unsigned long long* __restrict__ entry,
                                                                     unsigned long long* __restrict__ exitv, int* __restrict__ cnt,
                                                                     const unsigned long long* __restrict__ snap_in,
                                                                     unsigned long long* __restrict__ snap_out) {
    __shared__ unsigned long long ex[JPEG_WG];
    const long long lane0 = (long long)blockIdx.x * JPEG_WG, lane = lane0 + threadIdx.x;
    long long last = lane0 + JPEG_WG - 1;
    if (last > c.lanes - 1) last = c.lanes - 1;
    // uniform test: does the first lane continue a segment from the previous workgroup, with an entry that no longer matches?
    bool redo = false;
    if (blockIdx.x > 0) {
        const SegDesc s0 = c.segs[find_seg(c, lane0)];
        redo = lane0 > s0.lane0 && lane0 < s0.lane0 + s0.lanes && seg_ok(c, s0) && snap_in[blockIdx.x - 1] != entry[lane0];
    }
    if (!redo) {
        if (threadIdx.x == 0) snap_out[blockIdx.x] = exitv[last];
        return;
    }
    bool active = lane < c.lanes;
    SegDesc s{};
    if (active) {
        s = c.segs[find_seg(c, lane)];
        active = lane >= s.lane0 && lane < s.lane0 + s.lanes && seg_ok(c, s);
    }
    const bool first = active && lane == s.lane0;
    Dec dec{};
    unsigned long long en = ST_DEAD, my_ex = ST_DEAD;
    int n = 0;
    long long end = 0;
    if (active) {
        dec = make_dec(c, s);
        end = lane_end(s, lane);
        en = entry[lane];
        my_ex = exitv[lane];
        n = cnt[lane];
        if (threadIdx.x == 0) {
            en = snap_in[blockIdx.x - 1];
            my_ex = run_lane(dec, en, end, &n);
        }
    }
    ex[threadIdx.x] = my_ex;
    __syncthreads();
    chain(ex, active, first, dec, end, en, my_ex, n);
    if (lane < c.lanes) {
        entry[lane] = en;
        exitv[lane] = my_ex;
        cnt[lane] = n;
    }
    if (lane == last) snap_out[blockIdx.x] = my_ex;
}

__global__ void __launch_bounds__(JPEG_WG) se_jpeg_sync_repair_kernel(Ctx c, unsigned long long* __restrict__ entry,
                                                                      unsigned long long* __restrict__ exitv, int* __restrict__ cnt) {
    const int si = blockIdx.x * JPEG_WG + threadIdx.x;
    if (si >= c.n_segs) return;
    const SegDesc s = c.segs[si];
    if (!seg_ok(c, s)) return;
    const Dec dec = make_dec(c, s);
    const long long hi_lane = s.lane0 + s.lanes;
    for (long long w = s.lane0 / JPEG_WG + 1; w * JPEG_WG < hi_lane; ++w) {
        long long j = w * JPEG_WG;
        unsigned long long e = exitv[j - 1];
        const long long hi = (w + 1) * JPEG_WG < hi_lane ? (w + 1) * JPEG_WG : hi_lane;
        for (; j < hi; ++j) {
            if (entry[j] == e) break;
            entry[j] = e;
            int n;
            const unsigned long long x = run_lane(dec, e, lane_end(s, j), &n);
            cnt[j] = n;
            if (x == exitv[j]) break;
            exitv[j] = x;
            e = x;
        }
    }
}

// exclusive scan of the DC-code counts inside each workgroup of lanes
__global__ void __launch_bounds__(JPEG_WG) se_jpeg_scan_kernel(long long lanes, const int* __restrict__ cnt, int* __restrict__ loc,
                                                               int* __restrict__ wg_tot) {
    __shared__ int sh[JPEG_WG];
    const long long lane = (long long)blockIdx.x * JPEG_WG + threadIdx.x;
    const int v = lane < lanes ? cnt[lane] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < JPEG_WG; o <<= 1) {
        const int t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    if (lane < lanes) loc[lane] = sh[threadIdx.x] - v;
    if (threadIdx.x == JPEG_WG - 1) wg_tot[blockIdx.x] = sh[threadIdx.x];
}

__global__ void __launch_bounds__(1024) se_jpeg_scan_top_kernel(int n, const int* __restrict__ wg_tot, int* __restrict__ wg_pre) {
    __shared__ int sh[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < n ? wg_tot[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < n) wg_pre[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
}

__constant__ unsigned char c_natural[80] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33,
                                            40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
                                            29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                                            47, 55, 62, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};

__global__ void __launch_bounds__(JPEG_WG) se_jpeg_write_kernel(Ctx c, const unsigned long long* __restrict__ entry,
                                                                const int* __restrict__ loc, const int* __restrict__ wg_pre,
                                                                short* __restrict__ coef, int* __restrict__ status) {
    const long long lane = (long long)blockIdx.x * JPEG_WG + threadIdx.x;
    if (lane >= c.lanes) return;
    const int si = find_seg(c, lane);
    const SegDesc s = c.segs[si];
    if (lane < s.lane0 || lane >= s.lane0 + s.lanes) return;
    if (!seg_ok(c, s)) {
        if (lane == s.lane0) { status[2 * si] = SE_JPEG_BAD_DESC; status[2 * si + 1] = 0; }
        return;
    }
    unsigned long long st = entry[lane];
    if (stopped(st)) return;
    const Dec dec = make_dec(c, s);
    const long long nblocks = s.mcus * dec.bpm;
    const long long g0 = (long long)wg_pre[s.lane0 / JPEG_WG] + loc[s.lane0];
    long long nb = (long long)wg_pre[lane / JPEG_WG] + loc[lane] - g0;
    const long long end = lane_end(s, lane);
    const bool last = lane == s.lane0 + s.lanes - 1;
    if (nb > nblocks || (nb == nblocks && (st & 0xFF) == 0)) return;
    short* cb = coef + 64 * s.block0;
    int code = SE_JPEG_OK, value = 0;
    while ((long long)(st >> 32) < end) {
        const bool dc = (st & 0xFF) == 0;
        if (dc && nb == nblocks) break;
        int val = 0, pos = -1;
        const unsigned long long nx = step(dec, st, &val, &pos);
        if (stopped(nx)) {
            code = (nx & ST_ERR) ? SE_JPEG_NO_CODE : SE_JPEG_STREAM_END;
            value = (nx & ST_ERR) ? (int)(st >> 32) : (int)(dc ? nb : nb - 1);
            break;
        }
        if (dc) {
            cb[64 * nb] = (short)val;
            ++nb;
        } else if (pos >= 0 && nb >= 1) {
            cb[64 * (nb - 1) + c_natural[pos]] = (short)val;
        }
        st = nx;
    }
    if (code == SE_JPEG_OK && last && !((st & 0xFF) == 0 && nb == nblocks)) {
        code = SE_JPEG_STREAM_END;
        value = (int)((st & 0xFF) == 0 ? nb : nb - 1);
    }
    if (code != SE_JPEG_OK) {
        status[2 * si] = code;
        status[2 * si + 1] = value;
    }
}

// DC prediction per (segment, component): per_thread = 1: one thread walks the item; 0: one workgroup per item
__global__ void __launch_bounds__(JPEG_WG) se_jpeg_dc_kernel(Ctx c, short* __restrict__ coef, int per_thread) {
    __shared__ int sh[JPEG_WG];
    const long long item = per_thread ? (long long)blockIdx.x * JPEG_WG + threadIdx.x : blockIdx.x;
    if (item >= 3ll * c.n_segs) return;                      // uniform when !per_thread
    const SegDesc s = c.segs[item / 3];
    const int f = (int)(item % 3);
    if (!seg_ok(c, s)) return;
    const int* im = img_row(c, (int)s.img);
    if (f >= im[2]) return;
    const int hv = im[12 + f] * im[15 + f], k0 = im[33 + f], bpm = im[5];
    const long long n = s.mcus * hv;
    short* cb = coef + 64 * s.block0;
    auto at = [&](long long t) -> short& { return cb[64 * ((t / hv) * bpm + k0 + t % hv)]; };
    if (per_thread) {
        int acc = 0;
        for (long long t = 0; t < n; ++t) {
            acc += at(t);
            at(t) = (short)acc;
        }
        return;
    }
    const long long chunk = (n + JPEG_WG - 1) / JPEG_WG;
    const long long t0 = threadIdx.x * chunk, t1 = t0 + chunk < n ? t0 + chunk : n;
    int sum = 0;
    for (long long t = t0; t < t1; ++t) sum += at(t);
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < JPEG_WG; o <<= 1) {
        const int t = threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    int acc = sh[threadIdx.x] - sum;
    for (long long t = t0; t < t1; ++t) {
        acc += at(t);
        at(t) = (short)acc;
    }
}

namespace {
#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

// jidctint.c's 1-D kernel on JLONG (64-bit) values: o[0..7] before the final descale
__device__ __forceinline__ void idct8(const long long* v, long long* o) {
    long long z2 = v[2], z3 = v[6];
    long long z1 = (z2 + z3) * FIX_0_541196100;
    long long tmp2 = z1 + z3 * (-FIX_1_847759065);
    long long tmp3 = z1 + z2 * FIX_0_765366865;
    long long tmp0 = (v[0] + v[4]) * (1ll << 13);
    long long tmp1 = (v[0] - v[4]) * (1ll << 13);
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    long long z4 = tmp1 + tmp3;
    const long long z5 = (z3 + z4) * FIX_1_175875602;
    tmp0 *= FIX_0_298631336; tmp1 *= FIX_2_053119869; tmp2 *= FIX_3_072711026; tmp3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3; o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1; o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}

// range_limit[x & RANGE_MASK] of jidctint.c
__device__ __forceinline__ uint32_t range_limit(long long x) {
    const int i = (int)(x & 1023);
    return i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896;
}

// the image holding global block `b` (images are ordered by block base)
__device__ int find_img(const Ctx& c, long long b) {
    int lo = 0, hi = c.n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (img_row(c, mid)[36] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}
}  // namespace

__global__ void __launch_bounds__(JPEG_WG) se_jpeg_idct_kernel(Ctx c, const short* __restrict__ coef, const int* __restrict__ quant,
                                                               uint8_t* __restrict__ planes, int* __restrict__ status) {
    __shared__ int ws[JPEG_WG / 8][64];
    const int sub = threadIdx.x >> 3, t = threadIdx.x & 7;
    const long long b = (long long)blockIdx.x * (JPEG_WG / 8) + sub;
    bool ok = b < c.blocks, plain = true;
    int ii = 0;
    if (ok) {
        ii = find_img(c, b);
        ok = img_ok(c, ii) && b >= img_row(c, ii)[36];
    }
    const int* im = img_row(c, ii);
    long long rel = 0;
    int f = 0;
    if (ok) {
        rel = b - im[36];
        ok = rel < (long long)im[3] * im[4] * im[5];
        f = im[40 + (int)(rel % im[5])];
    }
    if (ok) {                     // pass 1: column t
        const short* in = coef + 64 * b;
        const int* q = quant + 64 * (4 * ii + f);
        long long v[8], o[8];
        for (int r = 0; r < 8; ++r) v[r] = (long long)(int)((uint32_t)(int)in[8 * r + t] * (uint32_t)q[8 * r + t]);
        idct8(v, o);
        for (int r = 0; r < 8; ++r) {
            const long long w = (o[r] + (1ll << 10)) >> 11;
            ws[sub][8 * r + t] = (int)w;
            plain = plain && v[r] == (short)v[r] && w == (short)w;
        }
    }
    __syncthreads();
    if (!ok) return;
    long long v[8], o[8];          // pass 2: row t
    for (int i = 0; i < 8; ++i) v[i] = ws[sub][8 * t + i];
    idct8(v, o);
    const int k = (int)(rel % im[5]), m = (int)(rel / im[5]);
    const int h = im[12 + f], kk = k - im[33 + f];
    const int bx = (m % im[3]) * h + kk % h, by = (m / im[3]) * im[15 + f] + kk / h;
    uint32_t lo = 0, hi = 0;
    for (int i = 0; i < 8; ++i) {
        const long long x = (o[i] + (1ll << 17)) >> 18;
        plain = plain && x >= -512 && x <= 511;
        (i < 4 ? lo : hi) |= range_limit(x) << (8 * (i & 3));
    }
    uint8_t* dst = planes + im[37 + f] + (long long)(8 * by + t) * im[27 + f] + 8 * bx;
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    if (!plain) {                 // rare: the block's segment entry, from the image's first segment, restart interval and the MCU
        // a block wholly outside the component's samples (MCU padding) reaches no pixel, and libjpeg never transforms it
        const bool real = 8 * bx < (im[0] * h + im[9] - 1) / im[9] && 8 * by < (im[1] * im[15 + f] + im[10] - 1) / im[10];
        const long long si = (long long)im[6] + (im[50] > 0 ? m / im[50] : 0);
        if (real && si >= 0 && si < c.n_segs && c.segs[si].img == ii && status[2 * si] == SE_JPEG_OK) {
            status[2 * si + 1] = (int)(rel - c.segs[si].mcu0 * im[5]);
            status[2 * si] = SE_JPEG_NOT_PLAIN;
        }
    }
}

namespace {
// one upsampled chroma sample of component f at output (x, y) (jdsample.c)
__device__ __forceinline__ int chroma(const int* im, const uint8_t* planes, int f, int x, int y) {
    const uint8_t* pl = planes + im[37 + f];
    const int pw = im[27 + f], h = im[12 + f], v = im[15 + f], hmax = im[9], vmax = im[10];
    if (h == hmax && v == vmax) return pl[(long long)y * pw + x];
    const int wc = (im[0] * h + hmax - 1) / hmax, hc = (im[1] * v + vmax - 1) / vmax;
    const int j = x >> 1;
    if (wc <= 2) return pl[(long long)(vmax == 2 ? y >> 1 : y) * pw + j];     // h2v1_upsample / h2v2_upsample
    const int jn = (x & 1) ? (j + 1 < wc ? j + 1 : wc - 1) : (j > 0 ? j - 1 : 0);
    if (vmax == 1) {
        const uint8_t* row = pl + (long long)y * pw;
        return (3 * row[j] + row[jn] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int near = y >> 1, far = (y & 1) ? (near + 1 < hc ? near + 1 : hc - 1) : (near > 0 ? near - 1 : 0);
    const uint8_t* r0 = pl + (long long)near * pw;
    const uint8_t* r1 = pl + (long long)far * pw;
    const int cj = 3 * r0[j] + r1[j], cn = 3 * r0[jn] + r1[jn];
    return (3 * cj + cn + ((x & 1) ? 7 : 8)) >> 4;
}
__device__ __forceinline__ uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
}  // namespace

__global__ void __launch_bounds__(JPEG_WG) se_jpeg_color_kernel(Ctx c, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out,
                                                                int n_out, int H, int W) {
    const int ii = blockIdx.y;
    const long long px = (long long)blockIdx.x * JPEG_WG + threadIdx.x;
    if (px >= (long long)H * W || !img_ok(c, ii)) return;
    const int* im = img_row(c, ii);
    if (im[0] != W || im[1] != H || im[8] < 0 || im[8] >= n_out) return;
    const int x = (int)(px % W), y = (int)(px / W);
    uint8_t* o = out + (((long long)im[8] * H + y) * W + x) * 3;
    const int Y = im[2] == 1 ? planes[im[37] + (long long)y * im[27] + x] : chroma(im, planes, 0, x, y);
    if (im[2] == 1) {
        o[0] = o[1] = o[2] = (uint8_t)Y;
        return;
    }
    const int cb = chroma(im, planes, 1, x, y) - 128, cr = chroma(im, planes, 2, x, y) - 128;
    o[0] = clamp255(Y + ((116130 * cb + 32768) >> 16));
    o[1] = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    o[2] = clamp255(Y + ((91881 * cr + 32768) >> 16));
}

// ------------------------------------------------------------------------------------------------------------------------------
namespace {
struct Layout {
    long long coef, planes, entry, exitv, cnt, loc, wg_tot, wg_pre, snap, total;
};
Layout layout_of(long long blocks, long long lanes, long long plane_bytes) {
    auto al = [](long long x) { return (x + 255) & ~255ll; };
    const long long nwg = (lanes + JPEG_WG - 1) / JPEG_WG;
    Layout L;
    L.coef = 0;
    L.planes = al(L.coef + blocks * 128);
    L.entry = al(L.planes + plane_bytes);
    L.exitv = al(L.entry + 8 * lanes);
    L.cnt = al(L.exitv + 8 * lanes);
    L.loc = al(L.cnt + 4 * lanes);
    L.wg_tot = al(L.loc + 4 * lanes);
    L.wg_pre = al(L.wg_tot + 4 * nwg);
    L.snap = al(L.wg_pre + 4 * nwg);
    L.total = al(L.snap + 16 * nwg);
    return L;
}
}  // namespace

extern "C" long long se_jpeg_scratch_bytes(int* img_desc, int n_images, long long* seg_desc, int n_segs, long long* layout) {
    if (n_images <= 0 || n_segs <= 0 || !img_desc || !seg_desc || !layout) return SE_ERR_BAD_ARG;
    long long blocks = 0, planes = 0, lanes = 0, max_run = 0;
    for (int i = 0; i < n_images; ++i) {
        int* d = img_desc + 64 * i;
        const int nc = d[2], mx = d[3], my = d[4], bpm = d[5];
        if ((nc != 1 && nc != 3) || mx <= 0 || my <= 0 || bpm < 1 || bpm > 10 || (long long)mx * my > (1 << 24)) return SE_ERR_BAD_ARG;
        d[36] = (int)blocks;
        blocks += (long long)mx * my * bpm;
        for (int f = 0; f < nc; ++f) {
            const long long bytes = (long long)d[27 + f] * d[30 + f];
            if (d[27 + f] <= 0 || d[30 + f] <= 0 || bytes > (1ll << 28)) return SE_ERR_BAD_ARG;
            d[37 + f] = (int)planes;
            planes += (bytes + 255) & ~255ll;
        }
        if (blocks > (1ll << 26) || planes > (1ll << 30)) return SE_ERR_BAD_ARG;
    }
    for (int j = 0; j < n_segs; ++j) {
        long long* s = seg_desc + 8 * j;
        const long long img = s[2], len = s[1];
        if (img < 0 || img >= n_images || len < 0 || len > (1ll << 28) || s[4] < 1) return SE_ERR_BAD_ARG;
        const int* d = img_desc + 64 * img;
        s[5] = lanes;
        s[6] = (8 * len + JPEG_LANE_BITS - 1) / JPEG_LANE_BITS + (len == 0);
        s[7] = d[36] + s[3] * d[5];
        lanes += s[6];
        for (int f = 0; f < d[2]; ++f) {
            const long long run = s[4] * d[12 + f] * d[15 + f];
            if (run > max_run) max_run = run;
        }
    }
    if (lanes > (1ll << 30)) return SE_ERR_BAD_ARG;
    layout[0] = blocks;
    layout[1] = lanes;
    layout[2] = planes;
    layout[3] = max_run;
    return layout_of(blocks, lanes, planes).total;
}

extern "C" int se_jpeg_decode_bgr_u8(const void* payload, long long payload_bytes, const int* img_desc, int n_images,
                                     const long long* seg_desc, int n_segs, const void* tables, const int* quant,
                                     const long long* layout, unsigned char* out, int n_out, int out_h, int out_w, void* scratch,
                                     long long scratch_bytes, int* status, int rounds, void* stream) {
    if (!payload || !img_desc || !seg_desc || !tables || !quant || !layout || !out || !status || !scratch) return SE_ERR_BAD_ARG;
    if (n_images <= 0 || n_segs <= 0 || n_out <= 0 || out_h <= 0 || out_w <= 0 || payload_bytes < 0) return SE_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(payload) & 3) || (reinterpret_cast<uintptr_t>(img_desc) & 3) ||
        (reinterpret_cast<uintptr_t>(seg_desc) & 7) || (reinterpret_cast<uintptr_t>(quant) & 3) ||
        (reinterpret_cast<uintptr_t>(tables) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 255))
        return SE_ERR_BAD_ARG;
    const long long blocks = layout[0], lanes = layout[1], plane_bytes = layout[2], max_run = layout[3];
    if (blocks <= 0 || lanes <= 0 || plane_bytes <= 0) return SE_ERR_BAD_ARG;
    const Layout L = layout_of(blocks, lanes, plane_bytes);
    if (L.total > scratch_bytes) return SE_ERR_BAD_ARG;
    if (rounds < 0) rounds = JPEG_ROUNDS;
    const hipStream_t s = se_stream(stream);
    uint8_t* sc = static_cast<uint8_t*>(scratch);
    Ctx c{static_cast<const uint8_t*>(payload), payload_bytes, img_desc, n_images, reinterpret_cast<const SegDesc*>(seg_desc), n_segs,
          static_cast<const uint8_t*>(tables), blocks, lanes, plane_bytes};
    auto* entry = reinterpret_cast<unsigned long long*>(sc + L.entry);
    auto* exitv = reinterpret_cast<unsigned long long*>(sc + L.exitv);
    auto* cnt = reinterpret_cast<int*>(sc + L.cnt);
    auto* loc = reinterpret_cast<int*>(sc + L.loc);
    auto* wg_tot = reinterpret_cast<int*>(sc + L.wg_tot);
    auto* wg_pre = reinterpret_cast<int*>(sc + L.wg_pre);
    auto* snap = reinterpret_cast<unsigned long long*>(sc + L.snap);
    auto* coef = reinterpret_cast<short*>(sc + L.coef);
    const int nwg = (int)((lanes + JPEG_WG - 1) / JPEG_WG);
    if (hipMemsetAsync(coef, 0, blocks * 128, s) != hipSuccess) return SE_ERR_BAD_ARG;
    if (hipMemsetAsync(status, 0, 8ll * n_segs, s) != hipSuccess) return SE_ERR_BAD_ARG;
    hipLaunchKernelGGL(se_jpeg_sync_intra_kernel, dim3(nwg), dim3(JPEG_WG), 0, s, c, entry, exitv, cnt, snap);
    SE_CHECK_LAUNCH();
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(se_jpeg_sync_inter_kernel, dim3(nwg), dim3(JPEG_WG), 0, s, c, entry, exitv, cnt, snap + (r & 1) * nwg,
                           snap + ((r + 1) & 1) * nwg);
        SE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(se_jpeg_sync_repair_kernel, dim3((n_segs + JPEG_WG - 1) / JPEG_WG), dim3(JPEG_WG), 0, s, c, entry, exitv, cnt);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(se_jpeg_scan_kernel, dim3(nwg), dim3(JPEG_WG), 0, s, lanes, cnt, loc, wg_tot);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(se_jpeg_scan_top_kernel, dim3(1), dim3(1024), 0, s, nwg, wg_tot, wg_pre);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(se_jpeg_write_kernel, dim3(nwg), dim3(JPEG_WG), 0, s, c, entry, loc, wg_pre, coef, status);
    SE_CHECK_LAUNCH();
    const int per_thread = max_run <= 64;
    const long long items = 3ll * n_segs;
    hipLaunchKernelGGL(se_jpeg_dc_kernel, dim3((unsigned)(per_thread ? (items + JPEG_WG - 1) / JPEG_WG : items)), dim3(JPEG_WG), 0, s,
                       c, coef, per_thread);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(se_jpeg_idct_kernel, dim3((unsigned)((blocks + JPEG_WG / 8 - 1) / (JPEG_WG / 8))), dim3(JPEG_WG), 0, s, c, coef,
                       quant, sc + L.planes, status);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(se_jpeg_color_kernel, dim3((unsigned)(((long long)out_h * out_w + JPEG_WG - 1) / JPEG_WG), n_images),
                       dim3(JPEG_WG), 0, s, c, sc + L.planes, out, n_out, out_h, out_w);
    SE_CHECK_LAUNCH();
    return 0;
}
