// ZIP / ZIPS-compressed and uncompressed OpenEXR depth maps decoded on the device (a batch of chunks from any number of files ->
// float32).  The companion of exr_piz.hip: same channel_desc, same epilogue, status codes that do not collide with its 2-7.
//
// Stands in for the host decoder sceneego_amd/exr.py (read_depth_exr: zlib.decompress, then _zip_decompress's predictor and
// de-interleave) and follows RFC 1950 / 1951 with zlib's acceptance rules:
//   zlib header   CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0, FDICT = 0 (zlib.decompress has no dictionary).
//   blocks        stored (LEN == ~NLEN, any length, empty included), fixed and dynamic Huffman, any number of them; BTYPE 3 is bad.
//   code lengths  HLIT <= 286, HDIST <= 30; a repeat code 16 needs a previous length and no repeat runs past HLIT + HDIST.  As in
//                 zlib's inflate_table: over-subscribed sets are bad; incomplete sets are bad except a literal/length or distance
//                 code whose only code has length 1, or an empty distance code; the literal/length code must hold end-of-block.
//                 The code-length code must be complete (zlib accepts an empty one, whose stream then fails on its missing
//                 end-of-block: the same verdict).
//   symbols       literal/length 286 / 287 and distance 30 / 31 are invalid, as is a bit pattern no code of an incomplete set
//                 has; a distance further back than the chunk's output so far is invalid.
//   trailer       Adler-32 of the output, big-endian, after the final block; bytes after it are ignored.
// One deliberate difference from exr.py: a stream that inflates to anything but the chunk's bytes_per_line * rows bytes is a bad
// stream (SE_ZIP_SIZE).  exr.py would de-interleave the longer or shorter buffer and read whatever lands in the chunk's rows.
//
//   se_exr_zip_inflate_kernel  one wavefront per chunk.  Symbols are decoded wave-uniformly (every lane runs the same decode; the
//                              bit buffer refills from a 2 KB window of the block that all lanes stage in LDS).  Huffman tables are
//                              built per block in LDS: a 2^9-entry fast table indexed by the next (bit-reversed) bits and, for
//                              longer codes or none, the canonical count / symbol walk.  Output goes to a 32 KB LDS ring (the
//                              deflate window); a match of any distance is one lane-parallel step per 64 bytes
//                              (out[p + k] = out[p - d + (k mod d)]).  The ring is streamed to the chunk's scratch slice with
//                              16-byte stores, which also accumulate the Adler-32 sums; nothing written to global memory is read
//                              back in this kernel.
//   se_exr_zip_recon_kernel    one workgroup per chunk: the predictor t[i] = (t[i - 1] + raw[i] - 128) mod 256 as a prefix sum over
//                              the whole slice (in place), then the epilogue of se_exr_piz_wavelet_kernel: the selected channel's
//                              bytes, de-interleaved on the fly (byte q of the line data is t[q / 2] for even q, t[half + q / 2]
//                              for odd q), float32 conversion, optional clamp and prepare_depth's nearest resize into
//                              out[b][H_out][W_out].  Stored chunks (block bytes == bytes_per_line * rows, and every NONE chunk)
//                              skip the inflate and the predictor and read their rows straight from the block.
//
// Bounds: every descriptor field is checked on the device against payload_bytes / scratch_bytes / the file's size before it is used
// (status SE_EXR_BAD_DESC otherwise).  The bit reader reads only bytes [0, block bytes) of the chunk's block; running out of bits is
// SE_ZIP_TRUNCATED, never a read past the block.  Output positions are checked against bytes_per_line * rows before every write, so
// the inflate writes only bytes [0, bytes_per_line * rows) of the chunk's scratch slice; the recon kernel reads and writes only
// those bytes and the chunk's rows of `out`, and only for a chunk whose status is 0.
#include "common.h"

#define ZIP_THREADS 64            // inflate: one wavefront per chunk
#define ZIP_RECON_THREADS 256
#define ZIP_FB 9                  // fast-table bits
#define ZIP_RING 32768            // deflate window (LDS ring of the output)
#define ZIP_FLUSH 16384           // stream the ring out once this many bytes are pending
#define ZIP_STAGE 2048            // block bytes staged in LDS for the bit reader
#define ZIP_ADLER_MOD 65521ull

// status codes (status[2 * chunk] = code, status[2 * chunk + 1] = bytes of output when the stream stopped); 1 is exr_piz.hip's
// SE_EXR_BAD_DESC, 2-7 its own stream errors
#define SE_ZIP_OK 0
#define SE_ZIP_BAD_DESC 1         // a descriptor field out of range (== SE_EXR_BAD_DESC)
#define SE_ZIP_BAD_HEADER 8       // zlib header: CM != 8, CINFO > 7, FCHECK or FDICT
#define SE_ZIP_BAD_BTYPE 9        // block type 3
#define SE_ZIP_BAD_STORED 10      // stored block with LEN != ~NLEN
#define SE_ZIP_BAD_LENGTHS 11     // code-length set over-subscribed / incomplete / without end-of-block / HLIT > 286 / HDIST > 30
#define SE_ZIP_BAD_SYMBOL 12      // invalid literal/length or distance symbol, or a bad repeat of code lengths
#define SE_ZIP_TOO_FAR 13         // distance further back than the output so far
#define SE_ZIP_TRUNCATED 14       // the block ended before the final block and trailer
#define SE_ZIP_SIZE 15            // decompressed size != bytes_per_line * rows
#define SE_ZIP_ADLER 16           // Adler-32 mismatch

namespace {

struct ChunkDesc {                // int64[16] per chunk, see include/sceneego_hip.h
    long long block_off, block_len, file, row0, ny, stored, c6, c7, c8, c9, c10, c11, c12, scratch_off, cap, pad;
};
struct FileDesc {                 // int32[8] per file (the PIZ channel_desc)
    int W, H, ptype, pre, sel, tot, pad0, pad1;
};
struct Huff {
    uint32_t fast[1 << ZIP_FB];   // (length << 16 | symbol) of the code the next ZIP_FB bits start with; 0: longer code or none
    uint16_t count[16];           // codes per length
    uint16_t sym[288];            // symbols ordered by (length, symbol)
};

__constant__ uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131,
                                      163, 195, 227, 258};
__constant__ uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                       2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// bytes of line data of a chunk (bytes_per_line * rows)
__device__ __forceinline__ long long raw_bytes(const ChunkDesc& d, const FileDesc& f) { return 2ll * f.tot * f.W * d.ny; }

__device__ bool desc_ok(const ChunkDesc& d, const FileDesc* files, int n_files, long long payload_bytes, long long scratch_bytes) {
    if (d.file < 0 || d.file >= n_files) return false;
    const FileDesc f = files[d.file];
    if (f.W <= 0 || f.H <= 0 || f.ptype < 0 || f.ptype > 2 || f.sel != (f.ptype == 1 ? 1 : 2) || f.pre < 0 || f.tot < f.pre + f.sel)
        return false;
    if (d.row0 < 0 || d.ny < 1 || d.row0 + d.ny > f.H) return false;
    if (d.block_off < 0 || d.block_len < 0 || d.block_off > payload_bytes || d.block_len > payload_bytes - d.block_off) return false;
    const long long n = raw_bytes(d, f);
    if (n > 0x7FFFFFFFll) return false;
    if (d.stored) return d.block_len >= n;
    return d.cap >= n && d.scratch_off >= 0 && (d.scratch_off & 15) == 0 && d.scratch_off <= scratch_bytes &&
           d.cap <= scratch_bytes - d.scratch_off;
}

// numpy's float16 -> float32 bit rule (npy_halfbits_to_floatbits), as in exr_piz.hip
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

// Canonical Huffman table of lens[0, n) with zlib's acceptance (inftrees.c; kind 0 code-length code, 1 literal/length, 2 distance).
// Run by the whole wave; returns 0 or SE_ZIP_BAD_LENGTHS (wave-uniform).  tmp: int[50] of LDS.
__device__ int huff_build(const uint8_t* lens, int n, Huff& h, int kind, int* tmp) {
    int* s_first = tmp;           // [16] first canonical code of each length
    int* s_base = tmp + 16;       // [16] index of its first symbol in h.sym
    int* s_next = tmp + 32;       // [16]
    const int lane = threadIdx.x;
    if (lane == 0) {
        for (int l = 0; l < 16; ++l) h.count[l] = 0;
        for (int s = 0; s < n; ++s) h.count[lens[s]]++;
        int maxl = 0;
        for (int l = 15; l >= 1; --l)
            if (h.count[l]) { maxl = l; break; }
        int left = 1, err = 0;
        for (int l = 1; l <= 15; ++l) {
            left = 2 * left - h.count[l];
            if (left < 0) { err = 1; break; }                   // over-subscribed
        }
        if (!err && left > 0) {                                 // incomplete
            if (kind == 0) err = 1;
            else if (kind == 1 && maxl != 1) err = 1;
            else if (kind == 2 && maxl > 1) err = 1;
        }
        int b = 0, code = 0;
        for (int l = 1; l <= 15; ++l) {
            if (l > 1) code = (code + h.count[l - 1]) << 1;
            s_first[l] = code;
            s_base[l] = b;
            s_next[l] = b;
            b += h.count[l];
        }
        for (int s = 0; s < n; ++s)
            if (lens[s]) h.sym[s_next[lens[s]]++] = (uint16_t)s;
        tmp[48] = err;
        tmp[49] = b;
    }
    __syncthreads();
    const int err = tmp[48], nsym = tmp[49];
    if (err) return SE_ZIP_BAD_LENGTHS;
    for (int i = lane; i < (1 << ZIP_FB); i += ZIP_THREADS) h.fast[i] = 0;
    __syncthreads();
    for (int k = lane; k < nsym; k += ZIP_THREADS) {
        const int s = h.sym[k], l = lens[s];
        if (l > ZIP_FB) continue;
        const uint32_t code = (uint32_t)(s_first[l] + (k - s_base[l]));
        const uint32_t rev = __brev(code) >> (32 - l);            // deflate sends Huffman codes most significant bit first
        for (uint32_t e = rev; e < (1u << ZIP_FB); e += 1u << l) h.fast[e] = ((uint32_t)l << 16) | (uint32_t)s;
    }
    __syncthreads();
    return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ZIP_THREADS) se_exr_zip_inflate_kernel(const uint8_t* __restrict__ payload, long long payload_bytes,
                                                                         const ChunkDesc* __restrict__ descs, const FileDesc* __restrict__ files,
                                                                         int n_files, uint8_t* __restrict__ scratch, long long scratch_bytes,
                                                                         int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[ZIP_RING];
    __shared__ __attribute__((aligned(16))) uint8_t stage[ZIP_STAGE];
    __shared__ Huff s_lit, s_dist;
    __shared__ uint8_t s_lens[320 + 19];                        // literal/length + distance lengths, then the 19 code-length lengths
    __shared__ int s_tmp[64];
    __shared__ unsigned long long s_adler[2][ZIP_THREADS];

    const int chunk = blockIdx.x, lane = threadIdx.x;
    const ChunkDesc d = descs[chunk];
    if (!desc_ok(d, files, n_files, payload_bytes, scratch_bytes)) {
        if (lane == 0) { status[2 * chunk] = SE_ZIP_BAD_DESC; status[2 * chunk + 1] = 0; }
        return;
    }
    if (d.stored) {                                             // read from the block by the recon kernel
        if (lane == 0) { status[2 * chunk] = SE_ZIP_OK; status[2 * chunk + 1] = 0; }
        return;
    }
    const FileDesc f = files[d.file];
    const long long n_out = raw_bytes(d, f);
    const uint8_t* src = payload + d.block_off;
    const long long blen = d.block_len;
    uint8_t* dst = scratch + d.scratch_off;

    // ---- bit reader over src[0, blen): bytes [in_lo, in_hi) staged in LDS; every call is wave-uniform ----
    unsigned long long bitbuf = 0;
    int bitcnt = 0;
    long long pos = 0, in_lo = 0, in_hi = 0;
    auto restage = [&](long long at) {
        __syncthreads();                                        // every lane is done with the old window
        const long long hi = blen - at < ZIP_STAGE ? blen : at + ZIP_STAGE;
        for (long long i = at + lane; i < hi; i += ZIP_THREADS) stage[i - at] = src[i];
        in_lo = at;
        in_hi = hi;
        __syncthreads();
    };
    auto refill = [&]() {
        if (bitcnt > 32 || pos >= blen) return;
        if (pos + 4 > in_hi) restage(pos);
        if (pos + 4 <= in_hi) {
            const uint8_t* q = stage + (pos - in_lo);
            const uint32_t w = q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
            bitbuf |= (unsigned long long)w << bitcnt;
            bitcnt += 32;
            pos += 4;
        } else {                                                // the block's last 1-3 bytes
            while (pos < in_hi) { bitbuf |= (unsigned long long)stage[pos - in_lo] << bitcnt; bitcnt += 8; pos++; }
        }
    };
    // n <= 16 bits; false when the block has fewer left
    auto getbits = [&](int n, uint32_t& v) -> bool {
        refill();
        if (n > bitcnt) return false;
        v = (uint32_t)(bitbuf & ((1ull << n) - 1));
        bitbuf >>= n;
        bitcnt -= n;
        return true;
    };
    auto decode = [&](const Huff& h, int& sym) -> int {
        refill();
        const uint32_t e = h.fast[bitbuf & ((1u << ZIP_FB) - 1)];
        if (e) {
            // a prefix code: a code found on the real bits (zero-filled past the end) of at most its length is the code
            const int l = (int)(e >> 16);
            if (l > bitcnt) return SE_ZIP_TRUNCATED;
            bitbuf >>= l;
            bitcnt -= l;
            sym = (int)(e & 0xFFFFu);
            return SE_ZIP_OK;
        }
        int code = 0, first = 0, index = 0;                     // canonical walk, one bit at a time
        for (int l = 1; l <= 15; ++l) {
            if (l > bitcnt) return SE_ZIP_TRUNCATED;
            code |= (int)((bitbuf >> (l - 1)) & 1);
            const int cnt = h.count[l];
            if (code - cnt < first) {
                sym = h.sym[index + (code - first)];
                bitbuf >>= l;
                bitcnt -= l;
                return SE_ZIP_OK;
            }
            index += cnt;
            first = (first + cnt) << 1;
            code <<= 1;
        }
        return SE_ZIP_BAD_SYMBOL;                               // a pattern no code of an incomplete set has
    };

    // ---- output: ring[p % ZIP_RING] holds byte p; bytes [0, flushed) are in dst ----
    long long p = 0, flushed = 0;
    unsigned long long a0 = 0, a1 = 0;                          // this lane's sums of byte and of position * byte, mod 65521
    auto flush = [&](long long upto) {                          // dst[flushed, upto) <- ring; flushed is 16-aligned
        __syncthreads();                                        // literals written by lane 0, match / stored bytes by all lanes
        const long long full = upto & ~15ll;
        for (long long q = flushed + 16ll * lane; q < full; q += 16ll * ZIP_THREADS) {
            const uint4 w = *reinterpret_cast<const uint4*>(ring + (q & (ZIP_RING - 1)));
            *reinterpret_cast<uint4*>(dst + q) = w;
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
            for (int k = 0; k < 16; ++k) {
                const uint32_t b = (ws[k >> 2] >> (8 * (k & 3))) & 255u;
                a0 += b;
                a1 += (unsigned long long)(q + k) * b;
            }
        }
        for (long long q = (full > flushed ? full : flushed) + lane; q < upto; q += ZIP_THREADS) {
            const uint32_t b = ring[q & (ZIP_RING - 1)];
            dst[q] = (uint8_t)b;
            a0 += b;
            a1 += (unsigned long long)q * b;
        }
        a0 %= ZIP_ADLER_MOD;                                    // < 2^47 added per flush (positions < 2^31)
        a1 %= ZIP_ADLER_MOD;
        flushed = upto;
        __syncthreads();
    };
    auto maybe_flush = [&]() {
        if (p - flushed >= ZIP_FLUSH) flush(p & ~15ll);
    };

    int err = SE_ZIP_OK;
    uint32_t v = 0;
    // ---- zlib header ----
    {
        uint32_t cmf = 0, flg = 0;
        if (!getbits(8, cmf) || !getbits(8, flg)) { err = SE_ZIP_TRUNCATED; goto done; }
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) { err = SE_ZIP_BAD_HEADER; goto done; }
    }
    // ---- blocks ----
    for (;;) {
        uint32_t bfinal = 0, btype = 0;
        if (!getbits(1, bfinal) || !getbits(2, btype)) { err = SE_ZIP_TRUNCATED; goto done; }
        if (btype == 3) { err = SE_ZIP_BAD_BTYPE; goto done; }
        if (btype == 0) {
            // stored: drop to the byte boundary, then LEN, NLEN and LEN bytes straight from the block
            bitbuf >>= bitcnt & 7;
            bitcnt -= bitcnt & 7;
            long long at = pos - bitcnt / 8;                    // the next unread byte
            bitbuf = 0;
            bitcnt = 0;
            if (blen - at < 4) { err = SE_ZIP_TRUNCATED; goto done; }
            const uint32_t len = src[at] | ((uint32_t)src[at + 1] << 8), nlen = src[at + 2] | ((uint32_t)src[at + 3] << 8);
            at += 4;
            if (len != (~nlen & 0xFFFFu)) { err = SE_ZIP_BAD_STORED; goto done; }
            if (blen - at < (long long)len) { err = SE_ZIP_TRUNCATED; goto done; }
            if (p + len > n_out) { err = SE_ZIP_SIZE; goto done; }
            for (uint32_t k = 0; k < len; k += 256) {           // <= 256 bytes between flush checks: the ring never overruns
                const uint32_t m = len - k < 256 ? len - k : 256;
                for (uint32_t j = lane; j < m; j += ZIP_THREADS) ring[(p + j) & (ZIP_RING - 1)] = src[at + k + j];
                p += m;
                maybe_flush();
            }
            pos = at + len;
            in_lo = in_hi = 0;                                  // restage at the next refill
            if (bfinal) break;
            continue;
        }
        if (btype == 1) {                                       // fixed codes; distance codes 30 / 31 exist and are invalid
            __syncthreads();
            for (int s = lane; s < 320; s += ZIP_THREADS) s_lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
            __syncthreads();
            huff_build(s_lens, 288, s_lit, 1, s_tmp);           // both complete
            huff_build(s_lens + 288, 32, s_dist, 2, s_tmp);
        } else {                                                // dynamic codes
            uint32_t hlit = 0, hdist = 0, hclen = 0;
            if (!getbits(5, hlit) || !getbits(5, hdist) || !getbits(4, hclen)) { err = SE_ZIP_TRUNCATED; goto done; }
            const int nlen = (int)hlit + 257, ndist = (int)hdist + 1, ncl = (int)hclen + 4;
            if (nlen > 286 || ndist > 30) { err = SE_ZIP_BAD_LENGTHS; goto done; }
            uint8_t* cl = s_lens + 320;
            __syncthreads();
            if (lane < 19) cl[lane] = 0;
            __syncthreads();
            for (int i = 0; i < ncl; ++i) {
                if (!getbits(3, v)) { err = SE_ZIP_TRUNCATED; goto done; }
                if (lane == 0) cl[kClOrder[i]] = (uint8_t)v;
            }
            __syncthreads();
            if ((err = huff_build(cl, 19, s_dist, 0, s_tmp))) goto done;
            // nlen literal/length then ndist distance lengths, one array (a repeat may cross from one into the other)
            int have = 0, prev = 0;
            while (have < nlen + ndist) {
                int sym = 0;
                if ((err = decode(s_dist, sym))) goto done;
                sym = __builtin_amdgcn_readfirstlane(sym);
                if (sym < 16) {
                    if (lane == 0) s_lens[have] = (uint8_t)sym;
                    prev = sym;
                    have++;
                    continue;
                }
                int rep;
                if (sym == 16) {
                    if (have == 0) { err = SE_ZIP_BAD_SYMBOL; goto done; }
                    if (!getbits(2, v)) { err = SE_ZIP_TRUNCATED; goto done; }
                    rep = 3 + (int)v;
                } else if (sym == 17) {
                    if (!getbits(3, v)) { err = SE_ZIP_TRUNCATED; goto done; }
                    rep = 3 + (int)v;
                    prev = 0;
                } else {
                    if (!getbits(7, v)) { err = SE_ZIP_TRUNCATED; goto done; }
                    rep = 11 + (int)v;
                    prev = 0;
                }
                if (have + rep > nlen + ndist) { err = SE_ZIP_BAD_SYMBOL; goto done; }
                for (int j = lane; j < rep; j += ZIP_THREADS) s_lens[have + j] = (uint8_t)prev;
                have += rep;
            }
            __syncthreads();
            if (s_lens[256] == 0) { err = SE_ZIP_BAD_LENGTHS; goto done; }        // no end-of-block code
            if ((err = huff_build(s_lens, nlen, s_lit, 1, s_tmp))) goto done;
            if ((err = huff_build(s_lens + nlen, ndist, s_dist, 2, s_tmp))) goto done;
        }
        // ---- the codes of a Huffman block ----
        for (;;) {
            int sym = 0;
            if ((err = decode(s_lit, sym))) goto done;
            sym = __builtin_amdgcn_readfirstlane(sym);
            if (sym < 256) {
                if (p >= n_out) { err = SE_ZIP_SIZE; goto done; }
                if (lane == 0) ring[p & (ZIP_RING - 1)] = (uint8_t)sym;
                p++;
                maybe_flush();
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) { err = SE_ZIP_BAD_SYMBOL; goto done; }                  // 286, 287
            if (!getbits(kLenExtra[sym], v)) { err = SE_ZIP_TRUNCATED; goto done; }
            const int len = kLenBase[sym] + (int)v;
            int dsym = 0;
            if ((err = decode(s_dist, dsym))) goto done;
            dsym = __builtin_amdgcn_readfirstlane(dsym);
            if (dsym >= 30) { err = SE_ZIP_BAD_SYMBOL; goto done; }                 // 30, 31
            if (!getbits(kDistExtra[dsym], v)) { err = SE_ZIP_TRUNCATED; goto done; }
            const int dist = kDistBase[dsym] + (int)v;
            if (dist > p) { err = SE_ZIP_TOO_FAR; goto done; }
            if (p + len > n_out) { err = SE_ZIP_SIZE; goto done; }
            // every source byte precedes p, and with dist <= ZIP_RING no source slot is one an earlier step of this match wrote
            // (slot of p + j' == slot of p - dist + (j mod dist) needs j' >= j); within a step all lanes read before any writes
            __syncthreads();
            for (int k = 0; k < len; k += ZIP_THREADS) {
                const int j = k + lane;
                uint8_t b = 0;
                if (j < len) b = ring[(p - dist + (j % dist)) & (ZIP_RING - 1)];
                __syncthreads();
                if (j < len) ring[(p + j) & (ZIP_RING - 1)] = b;
            }
            p += len;
            maybe_flush();
        }
        if (bfinal) break;
    }
    // ---- trailer: Adler-32, big-endian, at the next byte boundary ----
    {
        bitbuf >>= bitcnt & 7;
        bitcnt -= bitcnt & 7;
        uint32_t adler = 0;
        for (int k = 0; k < 4; ++k) {
            if (!getbits(8, v)) { err = SE_ZIP_TRUNCATED; goto done; }
            adler = (adler << 8) | v;
        }
        if (p != n_out) { err = SE_ZIP_SIZE; goto done; }
        flush(p);
        s_adler[0][lane] = a0;
        s_adler[1][lane] = a1;
        __syncthreads();
        if (lane == 0) {
            unsigned long long s0 = 0, s1 = 0;
            for (int t = 0; t < ZIP_THREADS; ++t) { s0 += s_adler[0][t]; s1 += s_adler[1][t]; }
            // A = 1 + sum b_i, B = n + sum (n - i) b_i = n + n * sum b_i - sum i * b_i (i from 0), both mod 65521
            const unsigned long long m = ZIP_ADLER_MOD, nm = (unsigned long long)p % m;
            s0 %= m;
            s1 %= m;
            const uint32_t A = (uint32_t)((1 + s0) % m), B = (uint32_t)((nm + nm * s0 + m - s1) % m);
            s_tmp[62] = ((B << 16) | A) == adler ? SE_ZIP_OK : SE_ZIP_ADLER;
        }
        __syncthreads();
        err = s_tmp[62];
    }
done:
    if (lane == 0) {
        status[2 * chunk] = err;
        status[2 * chunk + 1] = (int)p;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ZIP_RECON_THREADS) se_exr_zip_recon_kernel(const uint8_t* __restrict__ payload, long long payload_bytes,
                                                                             const ChunkDesc* __restrict__ descs, const FileDesc* __restrict__ files,
                                                                             int n_files, uint8_t* __restrict__ scratch, long long scratch_bytes,
                                                                             const int* __restrict__ status, float* __restrict__ out,
                                                                             int out_h, int out_w, float clamp) {
    __shared__ uint32_t s_part[ZIP_RECON_THREADS];
    const int chunk = blockIdx.x, tid = threadIdx.x;
    if (status[2 * chunk] != SE_ZIP_OK) return;
    const ChunkDesc d = descs[chunk];
    if (!desc_ok(d, files, n_files, payload_bytes, scratch_bytes)) return;      // status says so already
    const FileDesc f = files[d.file];
    const int W = f.W, H = f.H, ny = (int)d.ny, s = f.sel;
    const long long n = raw_bytes(d, f);
    const uint8_t* block = payload + d.block_off;
    uint8_t* t = scratch + d.scratch_off;

    if (!d.stored) {
        // predictor: t[0] = raw[0], t[i] = t[i - 1] + raw[i] - 128 (mod 256); each thread a contiguous segment, in place
        const long long seg = (n + ZIP_RECON_THREADS - 1) / ZIP_RECON_THREADS;
        const long long a = tid * seg < n ? tid * seg : n, b = a + seg < n ? a + seg : n;
        uint32_t sum = 0;
        for (long long i = a; i < b; ++i) sum += t[i] + (i ? 128u : 0u);                // raw - 128 == raw + 128 (mod 256)
        s_part[tid] = sum & 255u;
        __syncthreads();
        if (tid == 0) {
            uint32_t acc = 0;
            for (int k = 0; k < ZIP_RECON_THREADS; ++k) { const uint32_t x = s_part[k]; s_part[k] = acc; acc = (acc + x) & 255u; }
        }
        __syncthreads();
        uint32_t run = s_part[tid];
        for (long long i = a; i < b; ++i) {
            run = (run + t[i] + (i ? 128u : 0u)) & 255u;
            t[i] = (uint8_t)run;
        }
        __syncthreads();
    }
    const long long half = (n + 1) >> 1;
    auto byte_at = [&](long long q) -> uint32_t {                // byte q of the chunk's line data
        if (d.stored) return block[q];
        return (q & 1) ? t[half + (q >> 1)] : t[q >> 1];
    };

    // epilogue (se_exr_piz_wavelet_kernel's): output rows whose nearest source row lies in this chunk
    const double ry = (double)H / (double)out_h, rx = (double)W / (double)out_w;
    const long long bpl = 2ll * f.tot * W;
    float* ob = out + (long long)d.file * out_h * out_w;
    long long y_first = (long long)floor((double)d.row0 / ry) - 2;
    for (long long y = y_first < 0 ? 0 : y_first; y < out_h; ++y) {
        long long sy = (long long)floor((double)y * ry);
        if (sy > H - 1) sy = H - 1;
        const long long r = sy - d.row0;
        if (r >= ny) break;
        if (r < 0) continue;
        for (int x = tid; x < out_w; x += ZIP_RECON_THREADS) {
            long long sx = (long long)floor((double)x * rx);
            if (sx > W - 1) sx = W - 1;
            const long long q = r * bpl + 2ll * f.pre * W + 2ll * s * sx;
            const uint32_t w0 = byte_at(q) | (byte_at(q + 1) << 8);
            const uint32_t w1 = s == 2 ? byte_at(q + 2) | (byte_at(q + 3) << 8) : 0u;
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
extern "C" long long se_exr_zip_scratch_bytes(long long* chunk_desc, int n_chunks, const int* channel_desc, int n_files) {
    if (n_chunks < 0 || n_files < 0 || (n_chunks > 0 && (!chunk_desc || !channel_desc))) return SE_ERR_BAD_ARG;
    long long total = 0;
    for (int i = 0; i < n_chunks; ++i) {
        long long* d = chunk_desc + 16ll * i;
        const long long file = d[2], ny = d[4];
        if (file < 0 || file >= n_files || ny < 1 || ny > (1 << 20)) return SE_ERR_BAD_ARG;
        const int* fd = channel_desc + 8ll * file;
        const long long W = fd[0], tot = fd[5];
        if (W <= 0 || W > (1 << 24) || tot < 1 || tot > (1 << 16)) return SE_ERR_BAD_ARG;
        const long long cap = d[5] ? 0 : 2 * tot * W * ny;      // bytes_per_line * rows; stored chunks need none
        if (cap > 0x7FFFFFFFll) return SE_ERR_BAD_ARG;
        d[13] = total;
        d[14] = cap;
        total += (cap + 15) & ~15ll;                            // every slice starts 16-byte aligned
    }
    return total;
}

extern "C" int se_exr_zip_decode_f32(const void* payload, long long payload_bytes, const long long* chunk_desc, int n_chunks,
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
    hipLaunchKernelGGL(se_exr_zip_inflate_kernel, dim3(n_chunks), dim3(ZIP_THREADS), 0, s, pl, payload_bytes, descs, files, n_files,
                       sc, scratch_bytes, status);
    SE_CHECK_LAUNCH();
    hipLaunchKernelGGL(se_exr_zip_recon_kernel, dim3(n_chunks), dim3(ZIP_RECON_THREADS), 0, s, pl, payload_bytes, descs, files,
                       n_files, sc, scratch_bytes, status, out, out_h, out_w, clamp);
    SE_CHECK_LAUNCH();
    return 0;
}
