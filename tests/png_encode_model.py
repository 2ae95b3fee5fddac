"""Numpy model of the device PNG encoder (csrc/png_enc.hip), integer arithmetic only.  The kernel equals it byte for
byte.  Every rule that decides a byte is stated here once:

filter    per row the five PNG filters (above row 0 and left of column 0: zero); the row takes the filter with the smallest sum of
          min(v, 256 - v) over its filtered bytes, ties to the lowest filter number.  F = H rows of [type][W * bpp bytes].
segments  F in pieces of SEG bytes, one deflate block each.
parse     greedy over the ordered candidate distances D = distances(W, bpp): at p the run length L_d of F[p + i] == F[p + i - d]
          (p - d >= 0), capped at 258 and at the segment's end; the largest L_d, the first in list order among equals; >= 3: a
          (length, distance) token, else the literal.
codes     counts (end of block: 1); an alphabet with fewer than two counted symbols gets symbols 0 / 1 counted once where unused;
          the counted symbols sorted by (count, symbol); minimum-redundancy depths (Moffat / Katajainen in place on the sorted
          counts); depths above the limit folded into it and the Kraft sum repaired as miniz does (take one code off the limit,
          split the deepest shorter code, until the sum is exact); the lengths go out shortest first to the END of the sorted list
          (largest count, then largest symbol); canonical codes as RFC 1951 3.2.2.
lengths   the literal/length lengths 0..HLIT-1 and distance lengths 0..HDIST-1 as ONE sequence; at entry i with value v and run r
          of equal entries from i: v == 0 and r >= 3: code 17 (r <= 10) or 18 with min(r, 138); v != 0, entry i-1 equal v and
          r >= 3: code 16 with min(r, 6); else the entry itself.  The 19-symbol alphabet is limited to 7 bits by the same rule.
block     exact bits of the stored (40 + 8 n: header, padding, LEN / NLEN, bytes), fixed and dynamic forms; the smallest, ties
          stored, then fixed, then dynamic.
layout    every segment starts on a byte; a Huffman block that is not the last is followed by an empty stored block (000, zero
          padding, 00 00 FF FF); the last block has BFINAL = 1 and zero padding.  zlib: 78 01, segments, Adler-32 big-endian.
"""
import struct
import zlib

import numpy as np

SEG = 16384             # PE_SEG of csrc/png_enc.hip
MAX_MATCH, MIN_MATCH, WINDOW = 258, 3, 32768
SIGNATURE = b"\x89PNG\r\n\x1a\n"

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LIT = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8
FIXED_DIST = (5,) * 30


def distances(width, bpp):
    """The ordered candidate list D of a frame: the byte before and the pixel before.  Every further candidate tried (2 bpp, 3 bpp,
    R, R - bpp, R + bpp, 2 R) made the files larger: the greedy parse takes the longest match whatever its distance costs."""
    out = []
    for d in (1, bpp):
        if d not in out and d <= WINDOW:
            out.append(d)
    return tuple(out)


def zlib_bound(n, seg=SEG):
    """Bytes no zlib stream of this encoder exceeds for n filtered bytes: every segment stored plus its worst Huffman overhead."""
    return 2 + sum(min(seg, n - s) + 10 for s in range(0, n, seg)) + 4


# ------------------------------------------------------------------------------------------------------------------------- filter
def filter_candidates(img):
    """int64 [5, H, W*bpp]: the five filtered versions of every row (values 0..255)."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    cur = img.reshape(h, w * bpp).astype(np.int64)
    a = np.zeros_like(cur)
    a[:, bpp:] = cur[:, :-bpp] if w > 1 else 0
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    c = np.zeros_like(cur)
    c[1:, bpp:] = cur[:-1, :-bpp] if w > 1 else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([cur, (cur - a) & 255, (cur - b) & 255, (cur - ((a + b) >> 1)) & 255, (cur - paeth) & 255])


def filter_stream(img):
    """(F uint8 [H * (1 + W*bpp)], filter type per row)."""
    cand = filter_candidates(img)
    cost = np.minimum(cand, 256 - cand).sum(axis=2)                  # [5, H]
    types = np.argmin(cost, axis=0)                                  # the first among equals
    h = cand.shape[1]
    rows = cand[types, np.arange(h)]
    return np.concatenate([types[:, None], rows], axis=1).astype(np.uint8).reshape(-1), types


# -------------------------------------------------------------------------------------------------------------------------- parse
def parse(f, s0, s1, dists):
    """Tokens of the segment F[s0:s1]: an int (literal) or (length, distance)."""
    m = s1 - s0
    pos = np.arange(s0, s1)
    runs = []
    for d in dists:
        eq = np.zeros(m, dtype=bool)
        ok = pos >= d
        eq[ok] = f[pos[ok]] == f[pos[ok] - d]
        stops = np.append(np.flatnonzero(~eq), m)                     # the first unequal position at or after each position
        runs.append(np.minimum(stops[np.searchsorted(stops, np.arange(m))] - np.arange(m), MAX_MATCH))
    runs = np.stack(runs)
    best, which = runs.max(axis=0), runs.argmax(axis=0)
    tokens, p = [], 0
    while p < m:
        if best[p] >= MIN_MATCH:
            tokens.append((int(best[p]), int(dists[which[p]])))
            p += int(best[p])
        else:
            tokens.append(int(f[s0 + p]))
            p += 1
    return tokens


def length_symbol(n):
    """(symbol 257..285, extra bits, extra value)."""
    k = max(i for i, b in enumerate(LEN_BASE) if b <= n)
    return 257 + k, LEN_EXTRA[k], n - LEN_BASE[k]


def distance_symbol(d):
    k = max(i for i, b in enumerate(DIST_BASE) if b <= d)
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


def histograms(tokens):
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            lit[length_symbol(t[0])[0]] += 1
            dist[distance_symbol(t[1])[0]] += 1
        else:
            lit[t] += 1
    return lit, dist


# -------------------------------------------------------------------------------------------------------------------------- codes
def code_lengths(counts, limit):
    """Length-limited code lengths of an alphabet (see the module text); a list as long as ``counts``."""
    counts = list(counts)
    for s in (0, 1):
        if sum(1 for c in counts if c) < 2 and counts[s] == 0:
            counts[s] = 1
    order = sorted((c, s) for s, c in enumerate(counts) if c)
    n = len(order)
    a = [c for c, _ in order]
    # Moffat / Katajainen, in place: a[] ends as the depth of every sorted symbol
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or a[root] < a[leaf]:
            a[nxt] = a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] = a[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] += a[leaf]
            leaf += 1
    a[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    avbl, used, depth, root, nxt = 1, 0, 0, n - 2, n - 1
    while avbl > 0:
        while root >= 0 and a[root] == depth:
            used += 1
            root -= 1
        while avbl > used:
            a[nxt] = depth
            nxt -= 1
            avbl -= 1
        avbl, depth, used = 2 * used, depth + 1, 0
    # fold into the limit, repair the Kraft sum
    num = [0] * (limit + 1)
    for d in a:
        num[min(d, limit)] += 1
    total = sum(num[i] << (limit - i) for i in range(1, limit + 1))
    while total != 1 << limit:
        num[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
    lengths, j = [0] * len(counts), n
    for i in range(1, limit + 1):
        for _ in range(num[i]):
            j -= 1
            lengths[order[j][1]] = i
    return lengths


def canonical_codes(lengths):
    """Per symbol the code with its bits reversed (deflate sends a code from its most significant bit)."""
    top = max(lengths)
    count = [0] * (top + 2)
    for n in lengths:
        if n:
            count[n] += 1
    nxt, code = [0] * (top + 2), 0
    for n in range(1, top + 1):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = []
    for n in lengths:
        if n:
            out.append(int(format(nxt[n], f"0{n}b")[::-1], 2))
            nxt[n] += 1
        else:
            out.append(0)
    return out


def length_tokens(seq):
    """The run-length form of a sequence of code lengths: (symbol 0..18, extra value)."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            k = min(r, 138)
            out.append((17, k - 3) if k <= 10 else (18, k - 11))
            i += k
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3:
            k = min(r, 6)
            out.append((16, k - 3))
            i += k
        else:
            out.append((v, 0))
            i += 1
    return out


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        assert self.n % 8 == 0
        return self.acc.to_bytes(self.n // 8, "little")


def dynamic_plan(lit, dist):
    """Everything the dynamic form needs: (lit lengths, dist lengths, hlit, hdist, length tokens, cl lengths, hclen, header bits)."""
    ll, dl = code_lengths(lit, 15), code_lengths(dist, 15)
    hlit = max(257, 1 + max(s for s, n in enumerate(ll) if n))
    hdist = 1 + max(s for s, n in enumerate(dl) if n)
    toks = length_tokens(ll[:hlit] + dl[:hdist])
    clc = [0] * 19
    for s, _ in toks:
        clc[s] += 1
    cl = code_lengths(clc, 7)
    hclen = max(4, 1 + max(i for i, s in enumerate(CL_ORDER) if cl[s]))
    bits = 3 + 14 + 3 * hclen + sum(cl[s] + CL_EXTRA.get(s, 0) for s, _ in toks)
    return ll, dl, hlit, hdist, toks, cl, hclen, bits


def token_bits(lit, dist, ll, dl):
    """Bits of the tokens and the end-of-block code under the lengths ll / dl, from the histograms alone."""
    n = sum(c * ll[s] for s, c in enumerate(lit)) + sum(c * dl[s] for s, c in enumerate(dist))
    n += sum(lit[257 + k] * LEN_EXTRA[k] for k in range(29)) + sum(dist[k] * DIST_EXTRA[k] for k in range(30))
    return n


def block_bit_counts(tokens, nbytes):
    """(stored, fixed, dynamic) bits of a segment, by arithmetic on its histograms: what the choice is made from."""
    lit, dist = histograms(tokens)
    plan = dynamic_plan(lit, dist)
    return 40 + 8 * nbytes, 3 + token_bits(lit, dist, FIXED_LIT, FIXED_DIST), plan[7] + token_bits(lit, dist, plan[0], plan[1])


def choose_block(counts):
    return min(range(3), key=lambda k: (counts[k], k))          # 0 stored, 1 fixed, 2 dynamic


def write_block(out, raw, tokens, kind, last):
    """One deflate block of the given kind (0 stored, 1 fixed, 2 dynamic) appended to the bit writer ``out``."""
    out.put(1 if last else 0, 1)
    out.put(kind, 2)
    if kind == 0:
        out.align()
        out.put(len(raw), 16)
        out.put(len(raw) ^ 0xFFFF, 16)
        for v in raw:
            out.put(int(v), 8)
        return
    if kind == 1:
        ll, dl = list(FIXED_LIT), list(FIXED_DIST)
    else:
        ll, dl, hlit, hdist, toks, cl, hclen, _ = dynamic_plan(*histograms(tokens))
        out.put(hlit - 257, 5)
        out.put(hdist - 1, 5)
        out.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            out.put(cl[s], 3)
        clcode = canonical_codes(cl)
        for s, extra in toks:
            out.put(clcode[s], cl[s])
            if s >= 16:
                out.put(extra, CL_EXTRA[s])
    lc, dc = canonical_codes(ll), canonical_codes(dl)
    for t in tokens:
        if isinstance(t, tuple):
            s, eb, ev = length_symbol(t[0])
            out.put(lc[s], ll[s])
            out.put(ev, eb)
            s, eb, ev = distance_symbol(t[1])
            out.put(dc[s], dl[s])
            out.put(ev, eb)
        else:
            out.put(lc[t], ll[t])
    out.put(lc[256], ll[256])


def encode_segment(f, s0, s1, dists, last, force=None):
    """(bytes of the segment, info): the chosen (or forced) block and what follows it up to the next byte boundary."""
    tokens = parse(f, s0, s1, dists)
    counts = block_bit_counts(tokens, s1 - s0)
    kind = choose_block(counts) if force is None else force
    out = Bits()
    write_block(out, f[s0:s1], tokens, kind, last)
    block_bits = out.n
    if not last and kind != 0:
        out.put(0, 3)
        out.align()
        out.put(0xFFFF0000, 32)
    out.align()
    return out.bytes(), {"kind": kind, "counts": counts, "block_bits": block_bits, "tokens": tokens}


def adler32_segments(f, seg=SEG):
    """Adler-32 from per-segment (a, b, n) partials combined in order, as the pack kernel does."""
    a_all, b_all = 1, 0
    for s0 in range(0, len(f), seg):
        piece = f[s0:s0 + seg].astype(np.int64)
        n = len(piece)
        a = int(piece.sum()) % 65521
        b = int((piece * (n - np.arange(n))).sum()) % 65521
        b_all = (b_all + n * a_all + b) % 65521
        a_all = (a_all + a) % 65521
    return (b_all << 16) | a_all


def zlib_stream(f, dists, seg=SEG, info=None):
    out = bytearray(b"\x78\x01")
    for s0 in range(0, len(f), seg):
        s1 = min(s0 + seg, len(f))
        data, i = encode_segment(f, s0, s1, dists, s1 == len(f))
        out += data
        if info is not None:
            info.append(i)
    return bytes(out) + struct.pack(">I", adler32_segments(f, seg))


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_container(height, width, channels, idat):
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2 if channels == 3 else 0, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def encode(img, seg=SEG, dists=None, info=None):
    """uint8 [H,W,3] or [H,W] -> the PNG file."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3))
    h, w = img.shape[:2]
    bpp = 1 if img.ndim == 2 else 3
    f, _ = filter_stream(img)
    d = distances(w, bpp) if dists is None else dists
    return png_container(h, w, bpp, zlib_stream(f, d, seg, info))


def idat_of(data):
    """The IDAT payload of a file with the layout png_container writes."""
    assert data[:8] == SIGNATURE
    pos, out = 8, b""
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body), kind
        if kind == b"IDAT":
            out += body
        pos += 12 + n
    return out
