// Lossless PNG encoder on the device: uint8 [B,H,W,3] or [B,H,W] frames -> the zlib stream of every frame (78 01, one deflate block
// per PE_SEG bytes of the filtered rows, Adler-32), ready to sit in one IDAT chunk.  sceneego_amd/png_encode.py writes the chunks.
//
// Every byte is decided by integer rules with one right answer (tests/png_encode_model.py restates them):
//
//   png_filter_kernel    one workgroup per row: the five filters' sums of min(v, 256 - v), the smallest (ties: lowest number),
//                        the row [type][bytes] into the filtered stream F
//   png_deflate_kernel   one workgroup per (segment, frame), one thread per 64 bytes:
//                          runs     per candidate distance a 64-bit equality mask per thread; run lengths by a backward walk of the
//                                   masks with the carry of the (at most five) chunks after it, capped at 258 and the segment's end
//                          parse    best (length, distance) per position; exit position of every chunk for every entry position
//                                   (backward, per thread); one thread hops from chunk to chunk; every thread then walks its own
//                                   tokens: the greedy sequential parse
//                          codes    histograms by LDS atomics; (count, symbol) rank sort by all threads; minimum-redundancy depths,
//                                   limit repair and canonical codes by one thread per alphabet; the code-length code by thread 0
//                          block    stored / fixed / dynamic bits from the histograms; the smallest (ties in that order)
//                          bits     per-thread bit counts, exclusive scan, codes into a zeroed LDS bit buffer (shared words by
//                                   atomicOr), then the buffer, its byte count and the segment's Adler partial to the scratch
//   png_place_kernel     one workgroup per frame: exclusive scan of the segment sizes, 78 01, the Adler-32 combined in segment
//                        order, length and status
//   png_copy_kernel      one workgroup per (segment, frame): the segment's bytes to their place in out[b]
//
// A segment never takes more than len + 10 bytes (the stored form is chosen on a tie), so the slot of a segment in the scratch and
// the caller's capacity (checked on the host against the bound) hold every write; no length known only on the device sizes a write.
#include "common.h"

namespace {

#define PE_SEG 16384                    // bytes of the filtered stream per deflate block (SEG of tests/png_encode_model.py)
#define PE_NT 256
#define PE_CH (PE_SEG / PE_NT)          // 64 positions per thread: one 64-bit equality mask per distance
#define PE_SLOT (PE_SEG + 16)           // bytes of a segment's slot in the scratch (len + 10 at most, rounded to 16)
#define PE_MAXD 2                       // candidate distances: (1, bpp); the kernel takes any ordered list of this many
#define PE_MAXLEN 258
#define PE_ADLER 65521u

struct PngParams {
    int H, W, bpp, R;
    int n, nseg;                        // bytes of F per frame, segments per frame
    int nd, d[PE_MAXD];
    long long fstride;                  // bytes between the F of two frames
    long long cap;                      // bytes between two frames of `out`
};

struct PngScratch {
    unsigned char* f;                   // [B][fstride]
    unsigned char* slot;                // [B][nseg][PE_SLOT]
    int* segbytes;                      // [B][nseg]
    int* segoff;                        // [B][nseg]  offset of the segment in out[b]
    uint2* adler;                       // [B][nseg]  (sum of bytes, sum of (n - i) * byte_i), both mod 65521
};

// ---------------------------------------------------------------------------------------------------------------- reductions
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive scan of v over the 256 threads; sm holds 4 ints and may be reused right after the call returns
__device__ __forceinline__ int block_excl_scan(int v, int* sm, int& total) {
    const int inc = wave_incl_scan(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) sm[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < PE_NT / 64; ++w) {
        const int s = sm[w];
        if (w < wave) base += s;
        tot += s;
    }
    total = tot;
    return base + inc - v;
}

__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return sm[0] + sm[1] + sm[2] + sm[3];
}

// ---------------------------------------------------------------------------------------------------------------- filter
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int predict(int type, int a, int b, int c) {
    return type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c);
}

// grid (H, B)
__global__ __launch_bounds__(256) void png_filter_kernel(const unsigned char* __restrict__ frames, PngScratch s, PngParams p) {
    __shared__ unsigned long long sm[4];
    const int y = blockIdx.x, b = blockIdx.y;
    const int rb = p.W * p.bpp;
    const unsigned char* cur = frames + ((size_t)b * p.H + y) * rb;
    const unsigned char* up = y > 0 ? cur - rb : cur;           // read only when y > 0
    unsigned long long sum[5] = {0, 0, 0, 0, 0};
    for (int x = threadIdx.x; x < rb; x += 256) {
        const int v = cur[x];
        const int a = x >= p.bpp ? cur[x - p.bpp] : 0;
        const int u = y > 0 ? up[x] : 0;
        const int c = (y > 0 && x >= p.bpp) ? up[x - p.bpp] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int f = (v - predict(t, a, u, c)) & 255;
            sum[t] += (unsigned)min(f, 256 - f);
        }
    }
    unsigned long long best = 0;
    int type = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const unsigned long long total = block_sum(sum[t], sm);
        if (t == 0 || total < best) {                           // strictly smaller: ties stay with the lower number
            best = total;
            type = t;
        }
    }
    unsigned char* row = s.f + (size_t)b * p.fstride + (size_t)y * p.R;
    if (threadIdx.x == 0) row[0] = (unsigned char)type;
    for (int x = threadIdx.x; x < rb; x += 256) {
        const int v = cur[x];
        const int a = x >= p.bpp ? cur[x - p.bpp] : 0;
        const int u = y > 0 ? up[x] : 0;
        const int c = (y > 0 && x >= p.bpp) ? up[x - p.bpp] : 0;
        row[1 + x] = (unsigned char)((v - predict(type, a, u, c)) & 255);
    }
}

// ---------------------------------------------------------------------------------------------------------------- deflate tables
// length 3..258 -> (symbol - 257, extra bits, extra value)
__device__ __forceinline__ void length_code(int len, int& k, int& eb, int& ev) {
    const int l = len - 3;
    if (len == PE_MAXLEN) { k = 28; eb = 0; ev = 0; return; }
    if (l < 8) { k = l; eb = 0; ev = 0; return; }
    eb = 29 - __clz(l);                                         // floor(log2 l) - 2
    k = 4 * eb + 4 + ((l >> eb) & 3);
    ev = l & ((1 << eb) - 1);
}
__host__ __device__ __forceinline__ int length_extra_bits(int k) { return (k < 8 || k == 28) ? 0 : (k >> 2) - 1; }
__host__ __device__ __forceinline__ int dist_extra_bits(int k) { return k < 4 ? 0 : (k >> 1) - 1; }
// distance 1..32768 -> (symbol, extra value)
inline void dist_code(int dist, int& k, int& ev) {
    const int dd = dist - 1;
    if (dd < 4) { k = dd; ev = 0; return; }
    int top = 31;
    while (!((dd >> top) & 1)) --top;
    k = 2 * top + ((dd >> (top - 1)) & 1);
    ev = dd & ((1 << (top - 1)) - 1);
}
__device__ __forceinline__ int fixed_lit_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

struct DistCodes {
    int k[PE_MAXD], ev[PE_MAXD];       // symbol and extra value of every candidate distance
};

// ---------------------------------------------------------------------------------------------------------------- code construction
// The small state of one segment, behind the two 32 KiB arrays in the dynamic LDS block
struct Small {
    int lit_cnt[288], dist_cnt[32], dist_bld[32], cl_cnt[19];
    int lit_a[288], dist_a[32], cl_a[19];                       // sorted counts -> depths
    int num[3][16];
    unsigned short lit_sym[288], dist_sym[32], cl_sym[19];      // sorted symbols
    unsigned short lit_code[288], dist_code[32], cl_code[19];   // bit-reversed canonical codes
    unsigned short cl_tok[320];                                 // symbol | extra value << 5
    unsigned short head[PE_MAXD][PE_NT];
    unsigned short entry[PE_NT];
    unsigned char lit_len[288], dist_len[32], cl_len[19];
    unsigned long long red[4];
    int scan[4];
    int kind, hdr_bits, hlit, hdist, hclen, ncl, nbytes;
};

// fewer than two counted symbols: symbols 0 and 1 are counted once where unused
__device__ void two_symbols(int* cnt, int nalpha) {
    int used = 0;
    for (int s = 0; s < nalpha; ++s) used += cnt[s] != 0;
    for (int s = 0; s < 2; ++s)
        if (used < 2 && cnt[s] == 0) { cnt[s] = 1; ++used; }
}

// all threads: the counted symbols of cnt[] sorted by (count, symbol) into a[] / sym[]
__device__ __forceinline__ void rank_sort(const int* cnt, int nalpha, int* a, unsigned short* sym) {
    for (int s = threadIdx.x; s < nalpha; s += PE_NT) {
        const int c = cnt[s];
        if (c == 0) continue;
        int rank = 0;
        for (int o = 0; o < nalpha; ++o) {
            const int co = cnt[o];
            rank += (co != 0 && (co < c || (co == c && o < s))) ? 1 : 0;
        }
        a[rank] = c;
        sym[rank] = (unsigned short)s;
    }
}

// one thread: a[0..n) ascending counts -> code lengths (limit bits at most) and bit-reversed canonical codes of the alphabet
__device__ void build_codes(const int* cnt, int nalpha, int limit, int* a, const unsigned short* sym, int* num, unsigned char* len,
                            unsigned short* code) {
    int n = 0;
    for (int s = 0; s < nalpha; ++s) {
        n += cnt[s] != 0;
        len[s] = 0;
    }
    // Moffat / Katajainen in place (n >= 2 by the two-symbol rule)
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = next; }
        else a[next] = a[leaf++];
        if (leaf >= n || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = next; }
        else a[next] += a[leaf++];
    }
    a[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
    int avbl = 1, used = 0, depth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && a[root] == depth) { ++used; --root; }
        while (avbl > used) { a[next--] = depth; --avbl; }
        avbl = 2 * used;
        ++depth;
        used = 0;
    }
    for (int i = 0; i <= limit; ++i) num[i] = 0;
    for (int i = 0; i < n; ++i) ++num[min(a[i], limit)];
    unsigned total = 0;
    for (int i = 1; i <= limit; ++i) total += (unsigned)num[i] << (limit - i);
    while (total != (1u << limit)) {
        --num[limit];
        for (int i = limit - 1; i > 0; --i)
            if (num[i]) { --num[i]; num[i + 1] += 2; break; }
        --total;
    }
    int j = n;
    for (int i = 1; i <= limit; ++i)
        for (int l = num[i]; l > 0; --l) len[sym[--j]] = (unsigned char)i;
    // canonical codes: num[i] becomes the next code of length i
    unsigned c = 0;
    int prev = 0;
    for (int i = 1; i <= limit; ++i) {
        c = (c + (unsigned)prev) << 1;
        prev = num[i];
        num[i] = (int)c;
    }
    for (int s = 0; s < nalpha; ++s) {
        const int l = len[s];
        code[s] = l ? (unsigned short)(__brev((unsigned)num[l]++) >> (32 - l)) : 0;
    }
}

// one thread: v (n bits, n <= 32) at bit `pos` of the zeroed buffer
__device__ __forceinline__ void put_at(unsigned* w, int& pos, unsigned v, int n) {
    if (n == 0) return;
    const int i = pos >> 5, sh = pos & 31;
    atomicOr(&w[i], v << sh);
    if (sh + n > 32) atomicOr(&w[i + 1], v >> (32 - sh));
    pos += n;
}

// a thread's run of tokens: the first and the last word it touches are shared with its neighbours, the words between are its own
struct Emit {
    unsigned* w;
    int wi, n;
    unsigned long long acc;
    bool first;
    __device__ __forceinline__ void put(unsigned v, int bits) {            // bits <= 28, v below 1 << bits
        acc |= (unsigned long long)v << n;
        n += bits;
        if (n >= 32) {
            if (first) atomicOr(&w[wi], (unsigned)acc);
            else w[wi] = (unsigned)acc;
            first = false;
            ++wi;
            acc >>= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if (n > 0) atomicOr(&w[wi], (unsigned)acc);
    }
};

#define PE_IS_MATCH 0x8000          // best[]: PE_IS_MATCH | length << 3 | index into D, or the literal byte

// grid (nseg, B); dynamic LDS: best u16 [PE_SEG], area u16 [PE_SEG] (exit positions, then the bit buffer), Small
__global__ __launch_bounds__(PE_NT) void png_deflate_kernel(PngScratch s, PngParams p, DistCodes dc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned short* best = reinterpret_cast<unsigned short*>(lds);
    unsigned short* ex = reinterpret_cast<unsigned short*>(lds + 2 * PE_SEG);
    unsigned* bitbuf = reinterpret_cast<unsigned*>(lds + 2 * PE_SEG);
    Small& m = *reinterpret_cast<Small*>(lds + 4 * PE_SEG);
    const int t = threadIdx.x, seg = blockIdx.x, b = blockIdx.y;
    const int s0 = seg * PE_SEG;
    const int len = min(PE_SEG, p.n - s0);
    const bool last = seg == p.nseg - 1;
    const unsigned char* F = s.f + (size_t)b * p.fstride;
    const int q0 = t * PE_CH;
    const int cn = min(max(len - q0, 0), PE_CH);
    const int g0 = s0 + q0;

    for (int i = t; i < 288; i += PE_NT) m.lit_cnt[i] = 0;
    if (t < 32) m.dist_cnt[t] = 0;
    if (t < 19) m.cl_cnt[t] = 0;
    m.entry[t] = 0xFFFF;

    // ---- runs: equality masks, their leading runs, the Adler partial of the chunk
    unsigned long long mask[PE_MAXD] = {};
    unsigned asum = 0, bsum = 0;
    for (int i = 0; i < cn; ++i) {
        const int c = F[g0 + i];
        asum += (unsigned)c;
        bsum += (unsigned)(cn - i) * (unsigned)c;
#pragma unroll
        for (int k = 0; k < PE_MAXD; ++k)
            if (k < p.nd && g0 + i >= p.d[k] && F[g0 + i - p.d[k]] == c) mask[k] |= 1ull << i;
    }
#pragma unroll
    for (int k = 0; k < PE_MAXD; ++k) {
        const unsigned long long z = ~mask[k];
        m.head[k][t] = (unsigned short)(z ? __ffsll((long long)z) - 1 : PE_CH);
    }
    __syncthreads();
    int run[PE_MAXD];
#pragma unroll
    for (int k = 0; k < PE_MAXD; ++k) {
        int r = 0;
        for (int u = t + 1; u < PE_NT && r < PE_MAXLEN; ++u) {
            const int h = m.head[k][u];
            r += h;
            if (h < PE_CH) break;
        }
        run[k] = min(r, PE_MAXLEN);
    }
    // ---- best token per position and, for every entry position of the chunk, where the walk leaves the chunk
    const int cend = q0 + cn;
    for (int i = cn - 1; i >= 0; --i) {
        int L = 0, di = 0;
#pragma unroll
        for (int k = 0; k < PE_MAXD; ++k) {
            run[k] = ((mask[k] >> i) & 1ull) ? min(run[k] + 1, PE_MAXLEN) : 0;
            if (run[k] > L) { L = run[k]; di = k; }                // strictly longer: the first in list order among equals
        }
        const int q = q0 + i;
        const bool match = L >= 3;
        best[q] = match ? (unsigned short)(PE_IS_MATCH | (L << 3) | di) : (unsigned short)F[g0 + i];
        const int nq = q + (match ? L : 1);
        ex[q] = (unsigned short)(nq >= cend ? nq : ex[nq]);
    }
    __syncthreads();
    if (t == 0) {
        int pos = 0;
        while (pos < len) {
            m.entry[pos >> 6] = (unsigned short)pos;
            pos = ex[pos];
        }
    }
    __syncthreads();
    const int e = m.entry[t];
    for (int i = t; i < PE_SEG / 2; i += PE_NT) bitbuf[i] = 0u;        // the exit positions are not needed any more
    // ---- histograms
    if (e != 0xFFFF) {
        for (int q = e; q < cend;) {
            const int v = best[q];
            if (v & PE_IS_MATCH) {
                const int L = (v >> 3) & 0x1FF;
                int k, eb, ev;
                length_code(L, k, eb, ev);
                atomicAdd(&m.lit_cnt[257 + k], 1);
                atomicAdd(&m.dist_cnt[dc.k[v & 7]], 1);
                q += L;
            } else {
                atomicAdd(&m.lit_cnt[v], 1);
                ++q;
            }
        }
    }
    if (t == 0) atomicAdd(&m.lit_cnt[256], 1);
    __syncthreads();
    // ---- codes.  The literal/length alphabet always has two counted symbols: end-of-block and a literal or a length.
    if (t < 32) m.dist_bld[t] = m.dist_cnt[t];
    __syncthreads();
    if (t == 0) two_symbols(m.dist_bld, 30);
    __syncthreads();
    rank_sort(m.lit_cnt, 286, m.lit_a, m.lit_sym);
    rank_sort(m.dist_bld, 30, m.dist_a, m.dist_sym);
    __syncthreads();
    if (t == 0) build_codes(m.lit_cnt, 286, 15, m.lit_a, m.lit_sym, m.num[0], m.lit_len, m.lit_code);
    if (t == 64) build_codes(m.dist_bld, 30, 15, m.dist_a, m.dist_sym, m.num[1], m.dist_len, m.dist_code);
    __syncthreads();
    // ---- bits of the three forms
    unsigned long long dyn = 0, fix = 0;
    for (int sy = t; sy < 286; sy += PE_NT) {
        const int c = m.lit_cnt[sy], xb = sy > 256 ? length_extra_bits(sy - 257) : 0;
        dyn += (unsigned)(c * (m.lit_len[sy] + xb));
        fix += (unsigned)(c * (fixed_lit_len(sy) + xb));
    }
    if (t < 30) {
        const int c = m.dist_cnt[t], xb = dist_extra_bits(t);
        dyn += (unsigned)(c * (m.dist_len[t] + xb));
        fix += (unsigned)(c * (5 + xb));
    }
    dyn = block_sum(dyn, m.red);
    fix = block_sum(fix, m.red);
    if (t == 0) {
        // the code-length code over the two length lists as one sequence
        int hlit = 286, hdist = 30;
        while (hlit > 257 && m.lit_len[hlit - 1] == 0) --hlit;
        while (hdist > 1 && m.dist_len[hdist - 1] == 0) --hdist;
        const int total = hlit + hdist;
        int ncl = 0;
        for (int i = 0; i < total;) {
            const int v = i < hlit ? m.lit_len[i] : m.dist_len[i - hlit];
            int r = 1;
            while (i + r < total && (i + r < hlit ? m.lit_len[i + r] : m.dist_len[i + r - hlit]) == v) ++r;
            int sym, extra = 0, adv = 1;
            if (v == 0 && r >= 3) {
                adv = min(r, 138);
                sym = adv <= 10 ? 17 : 18;
                extra = adv <= 10 ? adv - 3 : adv - 11;
            } else if (v != 0 && i > 0 && (i - 1 < hlit ? m.lit_len[i - 1] : m.dist_len[i - 1 - hlit]) == v && r >= 3) {
                adv = min(r, 6);
                sym = 16;
                extra = adv - 3;
            } else {
                sym = v;
            }
            m.cl_tok[ncl++] = (unsigned short)(sym | (extra << 5));
            ++m.cl_cnt[sym];
            i += adv;
        }
        two_symbols(m.cl_cnt, 19);
        int n = 0;                                              // 19 symbols: sorted by insertion
        for (int sy = 0; sy < 19; ++sy) {
            const int c = m.cl_cnt[sy];
            if (c == 0) continue;
            int j = n++;
            while (j > 0 && m.cl_a[j - 1] > c) {                // equal counts stay in symbol order
                m.cl_a[j] = m.cl_a[j - 1];
                m.cl_sym[j] = m.cl_sym[j - 1];
                --j;
            }
            m.cl_a[j] = c;
            m.cl_sym[j] = (unsigned short)sy;
        }
        build_codes(m.cl_cnt, 19, 7, m.cl_a, m.cl_sym, m.num[2], m.cl_len, m.cl_code);
        const unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && m.cl_len[order[hclen - 1]] == 0) --hclen;
        int hdr = 3 + 14 + 3 * hclen;
        for (int i = 0; i < ncl; ++i) {
            const int sym = m.cl_tok[i] & 31;
            hdr += m.cl_len[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        const long long stored = 40 + 8ll * len, fixed = 3 + (long long)fix, dynamic = hdr + (long long)dyn;
        int kind = 0;
        long long bits = stored;
        if (fixed < bits) { kind = 1; bits = fixed; }
        if (dynamic < bits) kind = 2;
        m.kind = kind;
        m.hdr_bits = kind == 2 ? hdr : 3;
        m.hlit = hlit; m.hdist = hdist; m.hclen = hclen; m.ncl = ncl;
    }
    __syncthreads();
    const int kind = m.kind;
    if (kind == 1) {            // the fixed code is canonical too: lengths in, codes out
        for (int sy = t; sy < 288; sy += PE_NT) {
            const int l = fixed_lit_len(sy);
            const unsigned c = sy < 144 ? 0x30u + sy : sy < 256 ? 0x190u + (sy - 144) : sy < 280 ? (unsigned)(sy - 256) : 0xC0u + (sy - 280);
            m.lit_len[sy] = (unsigned char)l;
            m.lit_code[sy] = (unsigned short)(__brev(c) >> (32 - l));
        }
        if (t < 32) {
            m.dist_len[t] = 5;
            m.dist_code[t] = (unsigned short)(__brev((unsigned)t) >> 27);
        }
        __syncthreads();
    }
    // ---- bytes
    if (kind == 0) {
        unsigned char* bb = reinterpret_cast<unsigned char*>(bitbuf);
        if (t == 0) {
            bb[0] = last ? 1 : 0;
            bb[1] = (unsigned char)(len & 255);
            bb[2] = (unsigned char)(len >> 8);
            bb[3] = (unsigned char)(~len & 255);
            bb[4] = (unsigned char)((~len >> 8) & 255);
            m.nbytes = 5 + len;
        }
        for (int q = t; q < len; q += PE_NT) bb[5 + q] = F[s0 + q];
    } else {
        int mybits = 0;
        if (e != 0xFFFF) {
            for (int q = e; q < cend;) {
                const int v = best[q];
                if (v & PE_IS_MATCH) {
                    const int L = (v >> 3) & 0x1FF;
                    int k, eb, ev;
                    length_code(L, k, eb, ev);
                    const int dk = dc.k[v & 7];
                    mybits += m.lit_len[257 + k] + eb + m.dist_len[dk] + dist_extra_bits(dk);
                    q += L;
                } else {
                    mybits += m.lit_len[v];
                    ++q;
                }
            }
        }
        int total;
        const int start = m.hdr_bits + block_excl_scan(mybits, m.scan, total);
        if (e != 0xFFFF) {
            Emit em;
            em.w = bitbuf; em.wi = start >> 5; em.n = start & 31; em.acc = 0; em.first = true;
            for (int q = e; q < cend;) {
                const int v = best[q];
                if (v & PE_IS_MATCH) {
                    const int L = (v >> 3) & 0x1FF;
                    int k, eb, ev;
                    length_code(L, k, eb, ev);
                    const int di = v & 7, dk = dc.k[di];
                    const int ll = m.lit_len[257 + k], dl = m.dist_len[dk];
                    em.put((unsigned)m.lit_code[257 + k] | ((unsigned)ev << ll), ll + eb);
                    em.put((unsigned)m.dist_code[dk] | ((unsigned)dc.ev[di] << dl), dl + dist_extra_bits(dk));
                    q += L;
                } else {
                    em.put(m.lit_code[v], m.lit_len[v]);
                    ++q;
                }
            }
            em.flush();
        }
        if (t == 0) {
            int pos = 0;
            put_at(bitbuf, pos, (last ? 1u : 0u) | ((unsigned)kind << 1), 3);
            if (kind == 2) {
                const unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                put_at(bitbuf, pos, (unsigned)(m.hlit - 257), 5);
                put_at(bitbuf, pos, (unsigned)(m.hdist - 1), 5);
                put_at(bitbuf, pos, (unsigned)(m.hclen - 4), 4);
                for (int i = 0; i < m.hclen; ++i) put_at(bitbuf, pos, m.cl_len[order[i]], 3);
                for (int i = 0; i < m.ncl; ++i) {
                    const int sym = m.cl_tok[i] & 31, extra = m.cl_tok[i] >> 5;
                    put_at(bitbuf, pos, m.cl_code[sym], m.cl_len[sym]);
                    put_at(bitbuf, pos, (unsigned)extra, sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
                }
            }
            pos = m.hdr_bits + total;
            put_at(bitbuf, pos, m.lit_code[256], m.lit_len[256]);
            if (!last) {
                pos += 3;                                       // an empty stored block: 000, zero padding, 00 00 FF FF
                pos = (pos + 7) & ~7;
                put_at(bitbuf, pos, 0xFFFF0000u, 32);
            }
            m.nbytes = (pos + 7) >> 3;
        }
    }
    const unsigned long long after = (unsigned long long)max(len - cend, 0);
    const unsigned long long asum_all = block_sum(asum, m.red);
    const unsigned long long bsum_all = block_sum(((unsigned long long)bsum + (unsigned long long)asum * after) % PE_ADLER, m.red);
    __syncthreads();                                            // the bit buffer and nbytes are complete
    const int nbytes = m.nbytes;
    const size_t at = (size_t)b * p.nseg + seg;
    unsigned* dst = reinterpret_cast<unsigned*>(s.slot + at * PE_SLOT);
    for (int i = t; i < (nbytes + 3) >> 2; i += PE_NT) dst[i] = bitbuf[i];
    if (t == 0) {
        s.segbytes[at] = nbytes;
        s.adler[at] = make_uint2((unsigned)(asum_all % PE_ADLER), (unsigned)(bsum_all % PE_ADLER));
    }
}

// grid (B)
__global__ __launch_bounds__(256) void png_place_kernel(PngScratch s, PngParams p, unsigned char* __restrict__ out, int* __restrict__ length,
                                                        int* __restrict__ status) {
    __shared__ int sm[4];
    const int b = blockIdx.x;
    const int* nb = s.segbytes + (size_t)b * p.nseg;
    int* off = s.segoff + (size_t)b * p.nseg;
    int carry = 2;
    for (int base = 0; base < p.nseg; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < p.nseg ? nb[i] : 0;
        int total;
        const int o = block_excl_scan(v, sm, total);
        if (i < p.nseg) off[i] = carry + o;
        carry += total;
    }
    if (threadIdx.x == 0) {
        unsigned char* o = out + (size_t)b * p.cap;
        o[0] = 0x78;
        o[1] = 0x01;
        const uint2* ad = s.adler + (size_t)b * p.nseg;
        unsigned a = 1, bb = 0;
        for (int i = 0; i < p.nseg; ++i) {
            const unsigned n = (unsigned)min(PE_SEG, p.n - i * PE_SEG);
            bb = (unsigned)(((unsigned long long)bb + (unsigned long long)n * a + ad[i].y) % PE_ADLER);
            a = (a + ad[i].x) % PE_ADLER;
        }
        o[carry] = (unsigned char)(bb >> 8);
        o[carry + 1] = (unsigned char)(bb & 255);
        o[carry + 2] = (unsigned char)(a >> 8);
        o[carry + 3] = (unsigned char)(a & 255);
        length[b] = carry + 4;
        status[2 * b] = 0;
        status[2 * b + 1] = carry + 4;
    }
}

// grid (nseg, B)
__global__ __launch_bounds__(256) void png_copy_kernel(PngScratch s, PngParams p, unsigned char* __restrict__ out) {
    const size_t at = (size_t)blockIdx.y * p.nseg + blockIdx.x;
    const int n = s.segbytes[at];
    const unsigned char* src = s.slot + at * PE_SLOT;
    unsigned char* dst = out + (size_t)blockIdx.y * p.cap + s.segoff[at];
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------------------------- host
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

struct PngSizes {
    int R, n, nseg;
    long long bound;
    size_t fstride, off_slot, off_bytes, off_off, off_adler, total;
};

bool png_sizes(int batch, int height, int width, int channels, PngSizes& z) {
    if (batch <= 0 || batch > 65535 || height <= 0 || width <= 0 || (channels != 1 && channels != 3)) return false;
    const long long R = 1 + (long long)width * channels;
    if (R * height > 0x7fffffffll) return false;                // H * R < 2^31
    z.R = (int)R;
    z.n = (int)(R * height);
    z.nseg = (int)((R * height + PE_SEG - 1) / PE_SEG);
    z.bound = 2 + (long long)z.n + 10ll * z.nseg + 4;
    z.fstride = up256((size_t)z.n);
    size_t o = (size_t)batch * z.fstride;
    z.off_slot = o;  o += up256((size_t)batch * z.nseg * PE_SLOT);
    z.off_bytes = o; o += up256((size_t)batch * z.nseg * sizeof(int));
    z.off_off = o;   o += up256((size_t)batch * z.nseg * sizeof(int));
    z.off_adler = o; o += up256((size_t)batch * z.nseg * sizeof(uint2));
    z.total = o;
    return true;
}

}  // namespace

extern "C" long long se_png_encode_scratch_bytes(int batch, int height, int width, int channels) {
    PngSizes z;
    if (!png_sizes(batch, height, width, channels, z)) return SE_ERR_BAD_ARG;
    return (long long)z.total;
}

extern "C" long long se_png_encode_bound(int height, int width, int channels) {
    PngSizes z;
    if (!png_sizes(1, height, width, channels, z)) return SE_ERR_BAD_ARG;
    return z.bound;
}

extern "C" int se_png_encode_u8(const unsigned char* frames, unsigned char* out, int* length, int* status, void* scratch,
                                long long scratch_bytes, int batch, int height, int width, int channels, long long capacity,
                                void* stream) {
    if (!frames || !out || !length || !status || !scratch) return SE_ERR_BAD_ARG;
    PngSizes z;
    if (!png_sizes(batch, height, width, channels, z)) return SE_ERR_BAD_ARG;
    if (scratch_bytes < (long long)z.total || !se_aligned({scratch}, 16) || !se_aligned({length, status}, 4)) return SE_ERR_BAD_ARG;
    if (capacity < z.bound || capacity > 0x7fffffffll) return SE_ERR_BAD_ARG;
    PngParams p;
    p.H = height; p.W = width; p.bpp = channels; p.R = z.R; p.n = z.n; p.nseg = z.nseg;
    p.fstride = (long long)z.fstride;
    p.cap = capacity;
    // the candidate distances: (1, bpp), duplicates removed, nothing beyond the window
    DistCodes dc;
    p.nd = 0;
    for (int k = 0; k < PE_MAXD; ++k) { p.d[k] = 0; dc.k[k] = 0; dc.ev[k] = 0; }
    const int cand[PE_MAXD] = {1, channels};
    for (int k = 0; k < PE_MAXD; ++k) {
        bool seen = cand[k] > 32768;
        for (int j = 0; j < p.nd; ++j) seen = seen || p.d[j] == cand[k];
        if (seen) continue;
        dist_code(cand[k], dc.k[p.nd], dc.ev[p.nd]);
        p.d[p.nd++] = cand[k];
    }
    char* base = static_cast<char*>(scratch);
    PngScratch s;
    s.f = reinterpret_cast<unsigned char*>(base);
    s.slot = reinterpret_cast<unsigned char*>(base + z.off_slot);
    s.segbytes = reinterpret_cast<int*>(base + z.off_bytes);
    s.segoff = reinterpret_cast<int*>(base + z.off_off);
    s.adler = reinterpret_cast<uint2*>(base + z.off_adler);
    constexpr int LDS = 4 * PE_SEG + (int)sizeof(Small);
    static_assert(LDS <= 160 * 1024, "one segment's state must fit the LDS of a CU");
    SE_ENSURE_LDS(png_deflate_kernel, LDS);
    hipStream_t st = se_stream(stream);
    hipLaunchKernelGGL(png_filter_kernel, dim3(height, batch), dim3(256), 0, st, frames, s, p);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(png_deflate_kernel, dim3(z.nseg, batch), dim3(PE_NT), LDS, st, s, p, dc);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(png_place_kernel, dim3(batch), dim3(256), 0, st, s, p, out, length, status);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(png_copy_kernel, dim3(z.nseg, batch), dim3(256), 0, st, s, p, out);
    SE_CHECK_LAUNCH();
    return 0;
}
