// PIZ-compressed OpenEXR depth maps decoded on the device (a batch of chunks from any number of files -> float32).
//
// Stands in for the host decoder sceneego_amd/exr.py (read_depth_exr) and follows the same specification, step for step:
// bitmap -> reverse LUT, canonical Huffman with the run-length symbol rlc = iM and an 8-bit repeat count, wav2Decode (wdec14 when
// max_value < 2^14, wdec16 otherwise, with the odd row / column left over at each level), LUT, HALF / FLOAT / UINT assembly.  The
// result is bit-identical to exr.py for every file exr.py decodes (NaN payloads included: HALF -> float32 is the bit rule of
// numpy's float16 cast).
//
//   se_exr_piz_huffman_kernel  one workgroup per chunk.  Lane 0 unpacks the 6-bit code-length table into (length, symbol) records;
//                              all lanes count lengths; lane 0 computes the canonical start codes and orders the records by
//                              (length, symbol); all lanes fill a 2^12-entry (symbol, length) fast table in LDS.  Codes longer than
//                              12 bits are found through per-length (start code, count, base) ranges: a canonical code is
//                              prefix-free, so the shortest matching length is the only one.  The decode itself is serial on lane 0
//                              with a 64-bit bit buffer (codes reach 58 bits) over the bitstream staged in LDS.  Only the words up to
//                              the end of the selected channel's plane are decoded; those of the selected plane go to scratch.
//   se_exr_piz_wavelet_kernel  one workgroup per (chunk, selected plane): wav2Decode level by level (every level's 2x2 blocks, odd
//                              column and odd row are disjoint, so a level is one parallel step), the LUT through a popcount prefix
//                              of the bitmap (the k-th set bit; no 64 K table), then the epilogue: float32 conversion, optional clamp
//                              (values above `clamp` set to it, NaN kept) and the nearest resize of prepare_depth
//                              (src = min(floor(dst * (H / H_out)), H - 1), float64 like numpy) into out[b][H_out][W_out].  The
//                              plane lives in LDS when it fits (64 KB), otherwise the same code runs on the chunk's scratch slice.
//                              Chunks stored uncompressed skip the Huffman and wavelet steps and go through the same epilogue.
//
// Bounds: every descriptor field is checked on the device against payload_bytes / scratch_bytes / the file's size before it is used
// (status SE_EXR_BAD_DESC otherwise), the table and bitstream reads stop at the chunk's Huffman bytes and its nBits, and the decode
// writes only words [0, plane words) of the chunk's scratch slice.
#include "common.h"

#define EXR_TB 12                 // fast-table bits
#define EXR_STAGE 40960           // bitstream bytes staged in LDS (a demo chunk holds ~1.4 KB)
#define EXR_PLANE_LDS 65536       // plane bytes kept in LDS by the wavelet kernel
#define EXR_THREADS 256

// status codes (status[2 * chunk] = code, status[2 * chunk + 1] = words decoded when the stream ended early)
#define SE_EXR_OK 0
#define SE_EXR_BAD_DESC 1         // a descriptor field out of range
#define SE_EXR_TABLE_END 2        // the code-length table runs past the Huffman bytes
#define SE_EXR_TABLE_SIZE 3       // more code lengths than the scratch slice holds
#define SE_EXR_NBITS 4            // nBits exceeds the bytes after the table
#define SE_EXR_NO_CODE 5          // no code matches the next bits
#define SE_EXR_STREAM_END 6       // stream ended after k of n symbols
#define SE_EXR_RUN_PAST_END 7     // a run goes past the end of the output

namespace {

struct ChunkDesc {                // int64[16] per chunk, see include/sceneego_hip.h
    long long block_off, block_len, file, row0, ny, stored, min_nz, max_nz, huf_off, huf_len, im, iM, nbits, scratch_off, cap, pad;
};
struct FileDesc {                 // int32[8] per file
    int W, H, ptype, pre, sel, tot, pad0, pad1;
};

__device__ __forceinline__ long long plane_words(const ChunkDesc& d, const FileDesc& f) { return (long long)f.sel * f.W * d.ny; }

// records + sorted records (uint32 each) after the plane words, 16-byte aligned
__device__ __forceinline__ long long words_bytes_aligned(long long words) { return (words * 2 + 15) & ~15ll; }

__device__ bool desc_ok(const ChunkDesc& d, const FileDesc* files, int n_files, long long payload_bytes, long long scratch_bytes) {
    if (d.file < 0 || d.file >= n_files) return false;
    const FileDesc f = files[d.file];
    if (f.W <= 0 || f.H <= 0 || f.ptype < 0 || f.ptype > 2 || f.sel != (f.ptype == 1 ? 1 : 2) || f.pre < 0 || f.tot < f.pre + f.sel)
        return false;
    if (d.row0 < 0 || d.ny < 1 || d.row0 + d.ny > f.H) return false;
    if (d.block_off < 0 || d.block_len < 0 || d.block_off > payload_bytes || d.block_len > payload_bytes - d.block_off) return false;
    if (d.stored) return d.block_len >= 2ll * f.tot * f.W * d.ny;
    if (d.min_nz <= d.max_nz && (d.min_nz < 0 || d.max_nz >= 8192 || 4 + (d.max_nz - d.min_nz + 1) > d.block_len)) return false;
    if (d.huf_off < 4 || d.huf_len < 0 || d.huf_off > d.block_len || d.huf_len > d.block_len - d.huf_off) return false;
    if (d.huf_len > 0) {
        if (d.huf_len < 20 || d.im < 0 || d.im > d.iM || d.iM > 65536 || d.nbits < 0 || d.nbits > 8 * (d.huf_len - 20)) return false;
        if (d.cap < 0 || d.cap > d.iM - d.im + 1) return false;
    }
    const long long need = words_bytes_aligned(plane_words(d, f)) + 8 * (d.huf_len > 0 ? d.cap : 0);
    return d.scratch_off >= 0 && (d.scratch_off & 15) == 0 && d.scratch_off <= scratch_bytes && need <= scratch_bytes - d.scratch_off;
}

__device__ __forceinline__ void wdec14(uint32_t l, uint32_t h, uint32_t& a, uint32_t& b) {
    const int ls = (short)l, hi = (short)h;
    const int ai = ls + (hi & 1) + (hi >> 1);
    a = (uint32_t)ai & 0xFFFFu;
    b = (uint32_t)(ai - hi) & 0xFFFFu;
}
__device__ __forceinline__ void wdec16(uint32_t l, uint32_t h, uint32_t& a, uint32_t& b) {
    const int m = (int)l, d = (int)h;
    const int bb = (m - (d >> 1)) & 0xFFFF;
    a = (uint32_t)(d + bb - (1 << 15)) & 0xFFFFu;
    b = (uint32_t)bb;
}

// numpy's float16 -> float32 bit rule (npy_halfbits_to_floatbits): NaN payloads are shifted, not quieted
__device__ __forceinline__ uint32_t half_bits_to_float_bits(uint32_t h) {
    const uint32_t sgn = (h & 0x8000u) << 16;
    uint32_t e = h & 0x7C00u, sig = h & 0x03FFu;
    if (e == 0) {
        if (sig == 0) return sgn;
        sig <<= 1;
        while ((sig & 0x0400u) == 0) { sig <<= 1; e++; }
        return sgn + ((uint32_t)(127 - 15 - e) << 23) + ((sig & 0x03FFu) << 13);
    }
    if (e == 0x7C00u) return sgn + 0x7F800000u + (sig << 13);
    return sgn + (((h & 0x7FFFu) + 0x1C000u) << 13);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EXR_THREADS) se_exr_piz_huffman_kernel(const uint8_t* __restrict__ payload, long long payload_bytes,
                                                                         const ChunkDesc* __restrict__ descs, const FileDesc* __restrict__ files,
                                                                         int n_files, uint8_t* __restrict__ scratch, long long scratch_bytes,
                                                                         int* __restrict__ status) {
    __shared__ uint32_t fast[1 << EXR_TB];
    __shared__ uint8_t stage[EXR_STAGE];
    __shared__ unsigned long long s_start[59];
    __shared__ int s_count[59], s_base[59], s_next[59];
    __shared__ int s_nrec, s_err;
    __shared__ long long s_stream_pos;

    const int chunk = blockIdx.x, tid = threadIdx.x;
    const ChunkDesc d = descs[chunk];
    if (!desc_ok(d, files, n_files, payload_bytes, scratch_bytes)) {
        if (tid == 0) { status[2 * chunk] = SE_EXR_BAD_DESC; status[2 * chunk + 1] = 0; }
        return;
    }
    const FileDesc f = files[d.file];
    const long long n_sel = plane_words(d, f);
    uint16_t* words = reinterpret_cast<uint16_t*>(scratch + d.scratch_off);
    if (d.stored) {                       // copied by the wavelet kernel's epilogue
        if (tid == 0) { status[2 * chunk] = SE_EXR_OK; status[2 * chunk + 1] = 0; }
        return;
    }
    if (d.huf_len == 0) {                 // an empty Huffman block decodes to zeros (exr.py)
        for (long long i = tid; i < n_sel; i += EXR_THREADS) words[i] = 0;
        if (tid == 0) { status[2 * chunk] = SE_EXR_OK; status[2 * chunk + 1] = 0; }
        return;
    }
    const uint8_t* huf = payload + d.block_off + d.huf_off;
    const long long huf_len = d.huf_len;
    uint32_t* recs = reinterpret_cast<uint32_t*>(scratch + d.scratch_off + words_bytes_aligned(n_sel));
    uint32_t* sorted = recs + d.cap;

    for (int i = tid; i < (1 << EXR_TB); i += EXR_THREADS) fast[i] = 0xFFFFFFFFu;
    if (tid < 59) s_count[tid] = 0;
    if (tid == 0) {
        // code-length table (exr.py _huf_unpack_enc_table): records (length << 17 | symbol) in symbol order
        unsigned long long c = 0;
        int lc = 0, err = 0, nrec = 0;
        long long pos = 20;
        long long i = d.im;
        while (i <= d.iM) {
            while (lc < 6 && pos < huf_len) { c = (c << 8) | huf[pos++]; lc += 8; }
            if (lc < 6) { err = SE_EXR_TABLE_END; break; }
            lc -= 6;
            const int l = (int)((c >> lc) & 63);
            if (l == 63) {
                while (lc < 8 && pos < huf_len) { c = (c << 8) | huf[pos++]; lc += 8; }
                if (lc < 8) { err = SE_EXR_TABLE_END; break; }
                lc -= 8;
                i += (long long)((c >> lc) & 255) + 6;            // SHORTEST_LONG_RUN
            } else if (l >= 59) {
                i += l - 59 + 2;
            } else {
                if (l > 0) {
                    if (nrec >= d.cap) { err = SE_EXR_TABLE_SIZE; break; }
                    recs[nrec++] = ((uint32_t)l << 17) | (uint32_t)i;
                }
                i++;
            }
        }
        s_err = err;
        s_nrec = nrec;
        s_stream_pos = pos;
    }
    __syncthreads();
    if (s_err) {
        if (tid == 0) { status[2 * chunk] = s_err; status[2 * chunk + 1] = 0; }
        return;
    }
    const int nrec = s_nrec;
    for (int k = tid; k < nrec; k += EXR_THREADS) atomicAdd(&s_count[recs[k] >> 17], 1);
    __syncthreads();
    if (tid == 0) {
        // canonical start codes (exr.py _huf_canonical_code_table), then a stable order by length
        unsigned long long c = 0;
        for (int l = 58; l > 0; --l) {
            const unsigned long long nc = (c + (unsigned long long)s_count[l]) >> 1;
            s_start[l] = c;
            c = nc;
        }
        int b = 0;
        for (int l = 0; l <= 58; ++l) { s_base[l] = b; s_next[l] = b; b += s_count[l]; }
        for (int k = 0; k < nrec; ++k) {
            const uint32_t r = recs[k];
            sorted[s_next[r >> 17]++] = r;
        }
    }
    __syncthreads();
    // fast table: every code of length <= EXR_TB owns 2^(EXR_TB - l) entries; atomicMin keeps the shortest code on an entry, which
    // is what the bit-serial decoder of exr.py finds first
    for (int k = tid; k < nrec; k += EXR_THREADS) {
        const uint32_t r = sorted[k];
        const int l = (int)(r >> 17);
        if (l > EXR_TB) continue;
        const unsigned long long code = s_start[l] + (unsigned long long)(k - s_base[l]);
        if (code >= (1ull << l)) continue;                        // never matches an l-bit string
        const int lo = (int)(code << (EXR_TB - l)), n = 1 << (EXR_TB - l);
        for (int e = 0; e < n; ++e) atomicMin(&fast[lo + e], r);
    }
    // bitstream: ceil(nBits / 8) bytes after the table, staged in LDS when it fits
    const long long stream_pos = s_stream_pos;
    const long long stream_avail = huf_len - stream_pos;
    const long long nbits = d.nbits;
    const long long stream_bytes = (nbits + 7) >> 3;
    const bool nbits_ok = stream_bytes <= stream_avail;
    const bool staged = nbits_ok && stream_bytes <= EXR_STAGE;
    if (staged)
        for (long long i = tid; i < stream_bytes; i += EXR_THREADS) stage[i] = huf[stream_pos + i];
    __syncthreads();
    if (tid != 0) return;
    if (!nbits_ok) { status[2 * chunk] = SE_EXR_NBITS; status[2 * chunk + 1] = 0; return; }

    const uint8_t* src = staged ? stage : huf + stream_pos;
    const long long word_start = (long long)f.pre * f.W * d.ny, n_out = word_start + n_sel;
    const uint32_t rlc = (uint32_t)d.iM;
    // c holds lc unread bits (low end); bp counts the bits consumed.  Fast codes come out of c; a long code (up to 58 bits, more
    // than c may hold right after a refill) is read straight from the bytes at bp and c is re-synchronised behind it.
    unsigned long long c = 0;
    int lc = 0;
    long long pos = 0, bp = 0, o = 0;
    uint32_t last = 0;
    int err = SE_EXR_OK;
    while (bp < nbits && o < n_out) {
        while (lc <= 56 && pos < stream_bytes) { c = (c << 8) | src[pos++]; lc += 8; }
        const uint32_t idx = (uint32_t)((lc >= EXR_TB ? (c >> (lc - EXR_TB)) : (c << (EXR_TB - lc))) & ((1u << EXR_TB) - 1));
        const uint32_t e = fast[idx];
        int l = 0;
        uint32_t sym = 0;
        if (e != 0xFFFFFFFFu) {
            l = (int)(e >> 17);
            sym = e & 0x1FFFFu;
            if (l > nbits - bp) { err = SE_EXR_STREAM_END; break; }
            lc -= l;                          // l <= bits left <= lc: the refill stops short of 57 bits only at the stream's end
            bp += l;
        } else {
            const long long byte = bp >> 3;
            const int sh = (int)(bp & 7);
            unsigned long long v = 0;
            for (int k = 0; k < 8; ++k) v = (v << 8) | (byte + k < stream_bytes ? src[byte + k] : 0u);
            if (sh) v = (v << sh) | ((byte + 8 < stream_bytes ? src[byte + 8] : 0u) >> (8 - sh));
            for (int t = EXR_TB + 1; t <= 58; ++t) {
                const int n = s_count[t];
                if (n == 0) continue;
                const unsigned long long code = v >> (64 - t);
                if (code >= s_start[t] && code - s_start[t] < (unsigned long long)n) {
                    l = t;
                    sym = sorted[s_base[t] + (int)(code - s_start[t])] & 0x1FFFFu;
                    break;
                }
            }
            if (l == 0) { err = nbits - bp < 58 ? SE_EXR_STREAM_END : SE_EXR_NO_CODE; break; }
            if (l > nbits - bp) { err = SE_EXR_STREAM_END; break; }
            bp += l;
            pos = bp >> 3;                    // byte pos < stream_bytes whenever bp is not byte-aligned (bp <= nbits)
            c = 0;
            lc = 0;
            if (bp & 7) { c = src[pos++]; lc = 8 - (int)(bp & 7); }
        }
        if (sym == rlc) {
            if (nbits - bp < 8) { err = SE_EXR_STREAM_END; break; }
            while (lc <= 56 && pos < stream_bytes) { c = (c << 8) | src[pos++]; lc += 8; }
            lc -= 8;
            bp += 8;
            const long long cs = (long long)((c >> lc) & 255);
            if (o + cs > n_out) { err = SE_EXR_RUN_PAST_END; break; }
            const long long a = o > word_start ? o : word_start, b = o + cs;
            for (long long q = a; q < b; ++q) words[q - word_start] = (uint16_t)last;
            o += cs;
        } else {
            last = sym;
            if (o >= word_start) words[o - word_start] = (uint16_t)sym;
            o++;
        }
    }
    if (err == SE_EXR_OK && o < n_out) err = SE_EXR_STREAM_END;
    status[2 * chunk] = err;
    status[2 * chunk + 1] = (int)(o < 0x7FFFFFFF ? o : 0x7FFFFFFF);
}

// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EXR_THREADS) se_exr_piz_wavelet_kernel(const uint8_t* __restrict__ payload, long long payload_bytes,
                                                                         const ChunkDesc* __restrict__ descs, const FileDesc* __restrict__ files,
                                                                         int n_files, uint8_t* __restrict__ scratch, long long scratch_bytes,
                                                                         const int* __restrict__ status, float* __restrict__ out,
                                                                         int out_h, int out_w, float clamp) {
    extern __shared__ uint32_t lds[];
    uint32_t* bm = lds;                    // bitmap as 2048 32-bit words
    uint32_t* pre = lds + 2048;            // set bits before each word
    uint16_t* plane_lds = reinterpret_cast<uint16_t*>(lds + 4096);
    __shared__ int s_part[EXR_THREADS];

    const int chunk = blockIdx.x, tid = threadIdx.x;
    if (status[2 * chunk] != SE_EXR_OK) return;
    const ChunkDesc d = descs[chunk];
    if (!desc_ok(d, files, n_files, payload_bytes, scratch_bytes)) return;      // status says so already
    const FileDesc f = files[d.file];
    const int W = f.W, H = f.H, ny = (int)d.ny, s = f.sel;
    const long long n_sel = plane_words(d, f);
    const uint8_t* block = payload + d.block_off;

    uint16_t* img = nullptr;
    if (!d.stored) {
        uint16_t* gwords = reinterpret_cast<uint16_t*>(scratch + d.scratch_off);
        const bool in_lds = n_sel * 2 <= EXR_PLANE_LDS;
        img = in_lds ? plane_lds : gwords;
        if (in_lds)
            for (long long i = tid; i < n_sel; i += EXR_THREADS) plane_lds[i] = gwords[i];
        // bitmap (bytes min_nz..max_nz; value 0 always present) and its popcount prefix
        for (int w = tid; w < 2048; w += EXR_THREADS) {
            uint32_t v = 0;
            for (int k = 0; k < 4; ++k) {
                const long long byte = 4ll * w + k;
                if (byte >= d.min_nz && byte <= d.max_nz) v |= (uint32_t)block[4 + byte - d.min_nz] << (8 * k);
            }
            if (w == 0) v |= 1u;
            bm[w] = v;
        }
        __syncthreads();
        int part = 0;
        for (int k = 0; k < 8; ++k) part += __popc(bm[tid * 8 + k]);
        s_part[tid] = part;
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int t = 0; t < EXR_THREADS; ++t) { const int v = s_part[t]; s_part[t] = acc; acc += v; }
        }
        __syncthreads();
        {
            int acc = s_part[tid];
            for (int k = 0; k < 8; ++k) { pre[tid * 8 + k] = acc; acc += __popc(bm[tid * 8 + k]); }
        }
        __syncthreads();
        const int max_value = (int)pre[2047] + __popc(bm[2047]) - 1;
        const bool w14 = max_value < (1 << 14);

        // wav2Decode on each 16-bit sub-image j (the two halves of a 32-bit channel are independent): element (y, x) at (y*W + x)*s + j
        int n = W < ny ? W : ny;
        int p = 1;
        while (p <= n) p <<= 1;
        p >>= 1;
        int p2 = p;
        p >>= 1;
        while (p >= 1) {
            const int nys = ny >= p2 ? (ny - p2) / p2 + 1 : 0, nxs = W >= p2 ? (W - p2) / p2 + 1 : 0;
            const int n2d = nys * nxs, ncol = (W & p) ? nys : 0, nrow = (ny & p) ? nxs : 0;
            const int per = n2d + ncol + nrow;
            for (int t = tid; t < per * s; t += EXR_THREADS) {
                const int j = t / per, u = t - j * per;
                auto at = [&](int y, int x) -> uint16_t& { return img[((long long)y * W + x) * s + j]; };
                uint32_t a, b;
                if (u < n2d) {
                    const int y = (u / nxs) * p2, x = (u % nxs) * p2;
                    uint32_t i00, i01, i10, i11;
                    if (w14) { wdec14(at(y, x), at(y + p, x), i00, i10); wdec14(at(y, x + p), at(y + p, x + p), i01, i11); }
                    else { wdec16(at(y, x), at(y + p, x), i00, i10); wdec16(at(y, x + p), at(y + p, x + p), i01, i11); }
                    if (w14) wdec14(i00, i01, a, b); else wdec16(i00, i01, a, b);
                    at(y, x) = (uint16_t)a; at(y, x + p) = (uint16_t)b;
                    if (w14) wdec14(i10, i11, a, b); else wdec16(i10, i11, a, b);
                    at(y + p, x) = (uint16_t)a; at(y + p, x + p) = (uint16_t)b;
                } else if (u < n2d + ncol) {             // odd column left over at this level
                    const int y = (u - n2d) * p2, x = nxs * p2;
                    if (w14) wdec14(at(y, x), at(y + p, x), a, b); else wdec16(at(y, x), at(y + p, x), a, b);
                    at(y, x) = (uint16_t)a; at(y + p, x) = (uint16_t)b;
                } else {                                   // odd row left over at this level
                    const int y = nys * p2, x = (u - n2d - ncol) * p2;
                    if (w14) wdec14(at(y, x), at(y, x + p), a, b); else wdec16(at(y, x), at(y, x + p), a, b);
                    at(y, x) = (uint16_t)a; at(y, x + p) = (uint16_t)b;
                }
            }
            __syncthreads();
            p2 = p;
            p >>= 1;
        }
        // reverse LUT: word v -> the v-th value present in the bitmap (0 beyond max_value)
        for (long long i = tid; i < n_sel; i += EXR_THREADS) {
            const int v = img[i];
            uint32_t r = 0;
            if (v <= max_value) {
                int lo = 0, hi = 2047;                    // largest word with pre[w] <= v
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if ((int)pre[mid] <= v) lo = mid; else hi = mid - 1;
                }
                uint32_t m = bm[lo];
                for (int k = v - (int)pre[lo]; k > 0; --k) m &= m - 1;
                r = 32u * lo + (uint32_t)(__ffs(m) - 1);
            }
            img[i] = (uint16_t)r;
        }
        __syncthreads();
    }

    // epilogue: output rows whose nearest source row lies in this chunk
    const double ry = (double)H / (double)out_h, rx = (double)W / (double)out_w;
    const long long row_words = (long long)f.tot * W;    // 16-bit words per scanline of a stored chunk
    float* ob = out + (long long)d.file * out_h * out_w;
    // src_row(y) is non-decreasing: start a little before the first output row of the chunk and stop behind its last
    long long y_first = (long long)floor((double)d.row0 / ry) - 2;
    for (long long y = y_first < 0 ? 0 : y_first; y < out_h; ++y) {
        long long sy = (long long)floor((double)y * ry);
        if (sy > H - 1) sy = H - 1;
        const long long r = sy - d.row0;
        if (r >= ny) break;
        if (r < 0) continue;
        for (int x = tid; x < out_w; x += EXR_THREADS) {
            long long sx = (long long)floor((double)x * rx);
            if (sx > W - 1) sx = W - 1;
            uint32_t w0, w1 = 0;
            if (d.stored) {
                const long long q = r * row_words + (long long)f.pre * W + sx * s;
                w0 = block[2 * q] | ((uint32_t)block[2 * q + 1] << 8);
                if (s == 2) w1 = block[2 * q + 2] | ((uint32_t)block[2 * q + 3] << 8);
            } else {
                const long long q = (r * W + sx) * s;
                w0 = img[q];
                if (s == 2) w1 = img[q + 1];
            }
            float v;
            if (f.ptype == 1) v = __uint_as_float(half_bits_to_float_bits(w0));
            else if (f.ptype == 2) v = __uint_as_float((w1 << 16) | w0);
            else v = __uint2float_rn((w1 << 16) | w0);
            if (clamp > 0.f && v > clamp) v = clamp;
            ob[(long long)y * out_w + x] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
extern "C" long long se_exr_piz_scratch_bytes(long long* chunk_desc, int n_chunks, const int* channel_desc, int n_files) {
    if (n_chunks < 0 || n_files < 0 || (n_chunks > 0 && (!chunk_desc || !channel_desc))) return SE_ERR_BAD_ARG;
    long long total = 0;
    for (int i = 0; i < n_chunks; ++i) {
        long long* d = chunk_desc + 16ll * i;
        const long long file = d[2], ny = d[4], huf_len = d[9], im = d[10], iM = d[11];
        if (file < 0 || file >= n_files || ny < 1 || ny > (1 << 20)) return SE_ERR_BAD_ARG;
        const int* fd = channel_desc + 8ll * file;
        const long long W = fd[0], sel = fd[4];
        if (W <= 0 || W > (1 << 24) || sel < 1 || sel > 2) return SE_ERR_BAD_ARG;
        long long cap = 0;
        if (!d[5] && huf_len > 0) {
            if (huf_len < 20 || im < 0 || im > iM || iM > 65536) return SE_ERR_BAD_ARG;
            cap = (8 * (huf_len - 20)) / 6 + 1;                  // a length field takes at least 6 bits
            if (cap > iM - im + 1) cap = iM - im + 1;
        }
        d[13] = total;
        d[14] = cap;
        total += ((sel * W * ny * 2 + 15) & ~15ll) + ((8 * cap + 15) & ~15ll);      // every slice starts 16-byte aligned
    }
    return total;
}

extern "C" int se_exr_piz_decode_f32(const void* payload, long long payload_bytes, const long long* chunk_desc, int n_chunks,
                                     const int* channel_desc, int n_files, float* out, int out_h, int out_w, float clamp,
                                     void* scratch, long long scratch_bytes, int* status, void* stream) {
    if (n_chunks < 0 || n_files < 0 || out_h <= 0 || out_w <= 0 || payload_bytes < 0 || scratch_bytes < 0) return SE_ERR_BAD_ARG;
    if (n_chunks == 0) return 0;
    if (!payload || !chunk_desc || !channel_desc || !out || !status || n_files == 0 || (scratch_bytes > 0 && !scratch))
        return SE_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(chunk_desc) & 7) || (reinterpret_cast<uintptr_t>(channel_desc) & 3) ||
        (reinterpret_cast<uintptr_t>(scratch) & 15))
        return SE_ERR_BAD_ARG;
    const hipStream_t s = se_stream(stream);
    const auto* descs = reinterpret_cast<const ChunkDesc*>(chunk_desc);
    const auto* files = reinterpret_cast<const FileDesc*>(channel_desc);
    const auto* pl = static_cast<const uint8_t*>(payload);
    auto* sc = static_cast<uint8_t*>(scratch);
    hipLaunchKernelGGL(se_exr_piz_huffman_kernel, dim3(n_chunks), dim3(EXR_THREADS), 0, s, pl, payload_bytes, descs, files, n_files,
                       sc, scratch_bytes, status);
    SE_CHECK_LAUNCH();
    const int lds = 4096 * 4 + EXR_PLANE_LDS;
    SE_ENSURE_LDS(se_exr_piz_wavelet_kernel, lds);
    hipLaunchKernelGGL(se_exr_piz_wavelet_kernel, dim3(n_chunks), dim3(EXR_THREADS), lds, s, pl, payload_bytes, descs, files, n_files,
                       sc, scratch_bytes, status, out, out_h, out_w, clamp);
    SE_CHECK_LAUNCH();
    return 0;
}
