"""Test-side ZIP / ZIPS / NONE OpenEXR files whose deflate streams come from ``zlib.compressobj`` with chosen levels, strategies, window
sizes and flushes, for the device inflate (csrc/exr_zip.hip).

``write_zip_exr(channels, compression, ...)`` -> file bytes (``channels`` as in exr_piz_writer.write_exr); ``stream(data, chunk)``
makes each chunk's zlib stream from its predicted bytes, ``override={chunk: bytes}`` puts given bytes in a chunk verbatim.
``make_cases()`` -> {name: (file bytes, channels, what it covers, info)}; ``info`` lists each chunk's block types (``block_types``, a
small RFC 1951 walker), zlib CINFO and whether it is stored.  ``reencode(path, compression)`` writes a depth map again."""
from __future__ import annotations

import struct
import zlib

import numpy as np

import exr_piz_writer as W
from sceneego_amd import exr

_COMP = {"none": 0, "zips": 2, "zip": 3}
_LINES = {0: 1, 2: 1, 3: 16}


def predict(raw: bytes) -> bytes:
    """The inverse of exr.py's ``_zip_decompress``: the two halves interleaved, then byte differences + 128."""
    t = np.frombuffer(raw, dtype=np.uint8)
    inter = np.concatenate([t[0::2], t[1::2]]).astype(np.int32)
    d = inter.copy()
    d[1:] = (inter[1:] - inter[:-1] + 128) & 0xFF
    return d.astype(np.uint8).tobytes()


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush=None, pieces=1) -> bytes:
    """zlib stream of ``data``; with ``flush`` (Z_SYNC_FLUSH / Z_FULL_FLUSH) after each of ``pieces`` - 1 pieces."""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    step = max(1, -(-len(data) // pieces))
    out = []
    for i in range(0, len(data), step):
        out.append(co.compress(data[i:i + step]))
        if flush is not None and i + step < len(data):
            out.append(co.flush(flush))
    out.append(co.flush())
    return b"".join(out)


def with_cinfo(stream: bytes, cinfo: int) -> bytes:
    """The same stream with another CINFO in its header (FCHECK recomputed); only for streams with no distance beyond 2^(cinfo+8)."""
    cmf = (cinfo << 4) | 8
    flg = stream[1] & 0xE0
    flg |= (31 - ((cmf << 8) | flg) % 31) % 31
    return bytes([cmf, flg]) + stream[2:]


def write_zip_exr(channels: dict, compression: str = "zip", window=(0, 0), stream=None, store_chunks=(), override=None) -> bytes:
    chans = sorted((n, pt, np.asarray(a)) for n, (pt, a) in channels.items())
    H, Wd = chans[0][2].shape
    xmin, ymin = window
    comp = _COMP[compression]
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", pt, 0, 1, 1) for n, pt, _ in chans) + b"\0"
    hdr = b"\x76\x2f\x31\x01" + struct.pack("<I", 2)
    hdr += W._attr("channels", "chlist", chlist)
    hdr += W._attr("compression", "compression", bytes([comp]))
    hdr += W._attr("dataWindow", "box2i", struct.pack("<iiii", xmin, ymin, xmin + Wd - 1, ymin + H - 1))
    hdr += W._attr("displayWindow", "box2i", struct.pack("<iiii", xmin, ymin, xmin + Wd - 1, ymin + H - 1))
    hdr += W._attr("lineOrder", "lineOrder", b"\0")
    hdr += W._attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    hdr += W._attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0))
    hdr += W._attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    lpc = _LINES[comp]
    n_chunks = (H + lpc - 1) // lpc
    make = stream or (lambda data, i: deflate(data))
    blocks = []
    for i in range(n_chunks):
        y0 = i * lpc
        ny = min(lpc, H - y0)
        raw = W._raw_lines(chans, y0, ny)
        if override and i in override:
            data = override[i]
        elif comp == 0 or i in store_chunks:
            data = raw
        else:
            data = make(predict(raw), i)
            assert len(data) != len(raw), "a stream as long as the scanlines reads as a stored chunk"
        blocks.append(struct.pack("<ii", ymin + y0, len(data)) + data)
    pos = len(hdr) + 8 * n_chunks
    offsets = []
    for b in blocks:
        offsets.append(pos)
        pos += len(b)
    return hdr + struct.pack(f"<{n_chunks}Q", *offsets) + b"".join(blocks)


def chunks(buf: bytes):
    """[(y0, block bytes)] of a scanline file, in offset-table order."""
    hdr = exr._parse_header(buf)
    H = hdr["window"][3] - hdr["window"][1] + 1
    lpc = exr._LINES_PER_CHUNK[hdr["compression"]]
    n = (H + lpc - 1) // lpc
    out = []
    for off in struct.unpack_from(f"<{n}Q", buf, hdr["data_start"]):
        y0, size = struct.unpack_from("<ii", buf, off)
        out.append((y0, buf[off + 8:off + 8 + size]))
    return out


def reencode(path_or_bytes, compression: str, **kw) -> bytes:
    buf = path_or_bytes if isinstance(path_or_bytes, bytes) else open(path_or_bytes, "rb").read()
    hdr = exr._parse_header(buf)
    planes = exr.read_exr_buffer(buf)
    chans = {c[0]: (c[1], planes[c[0]]) for c in hdr["channels"]}
    return write_zip_exr(chans, compression, window=hdr["window"][:2], **kw)


# ------------------------------------------------------------------------------------------------
# RFC 1951 block walker (block types only; the stream is trusted)
# ------------------------------------------------------------------------------------------------
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in range(2)]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class _Bits:
    def __init__(self, data, pos):
        self.d, self.p, self.buf, self.cnt = data, pos, 0, 0

    def get(self, n):
        while self.cnt < n:
            self.buf |= self.d[self.p] << self.cnt
            self.p += 1
            self.cnt += 8
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v


def _table(lens):
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    offs = [0] * 16
    for l in range(1, 16):
        offs[l] = offs[l - 1] + count[l - 1]
    sym = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            sym[offs[l]] = s
            offs[l] += 1
    return count, sym


def _decode(br, table):
    count, sym = table
    code = first = index = 0
    for l in range(1, 16):
        code |= br.get(1)
        c = count[l]
        if code - c < first:
            return sym[index + code - first]
        index += c
        first = (first + c) << 1
        code <<= 1
    raise ValueError("bad code")


def block_types(stream: bytes):
    """Types (0 stored, 1 fixed, 2 dynamic) of the deflate blocks of a zlib stream, in order; stored ones as (0, LEN)."""
    br = _Bits(stream, 2)
    types = []
    while True:
        final, t = br.get(1), br.get(2)
        if t == 0:
            br.buf = br.cnt = 0                       # get() reads whole bytes: dropping the rest aligns to a byte
            n = stream[br.p] | stream[br.p + 1] << 8
            types.append((0, n))
            br.p += 4 + n
        else:
            types.append(t)
            if t == 1:
                lit, dist = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30)
            else:
                nlen, nd, ncl = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                cl = [0] * 19
                for i in range(ncl):
                    cl[_ORDER[i]] = br.get(3)
                h, lens = _table(cl), []
                while len(lens) < nlen + nd:
                    s = _decode(br, h)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + br.get(2))
                    elif s == 17:
                        lens += [0] * (3 + br.get(3))
                    else:
                        lens += [0] * (11 + br.get(7))
                lit, dist = _table(lens[:nlen]), _table(lens[nlen:])
            while True:
                s = _decode(br, lit)
                if s == 256:
                    break
                if s > 256:
                    br.get(_LEXT[s - 257])
                    br.get(_DEXT[_decode(br, dist)])
        if final:
            return types


# ------------------------------------------------------------------------------------------------
# the cases the tests decode
# ------------------------------------------------------------------------------------------------
def _odd():
    d = W._smooth(77, 333, 1)
    d[5, 7], d[6, 8], d[70, 300], d[40, 3] = np.nan, np.inf, 12.5, -np.inf
    d[50:77, 10:320] = 11.0
    return d


def make_cases():
    c = {}
    odd = {"Y": (1, _odd())}
    c["zip_odd_window"] = (odd, dict(compression="zip", window=(5, -3)), "ZIP 333x77 at (5, -3), 13-row last chunk, NaN / inf")
    c["zips_odd_window"] = (odd, dict(compression="zips", window=(5, -3)), "ZIPS, the same data: 77 one-line chunks")
    c["none_odd_window"] = (odd, dict(compression="none", window=(5, -3)), "NONE, the same data")
    sm = {"Y": (1, W._smooth(40, 96, 2))}
    for level in (0, 1, 9):
        c[f"zip_level{level}"] = (sm, dict(stream=lambda d, i, lv=level: deflate(d, level=lv)), f"zlib level {level}")
    c["zip_level0_sync"] = (sm, dict(stream=lambda d, i: deflate(d, level=0, flush=zlib.Z_SYNC_FLUSH, pieces=4)),
                            "level 0 with sync flushes: several stored blocks per chunk, empty ones among them")
    for name, st in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE),
                     ("filtered", zlib.Z_FILTERED)):
        c[f"zip_{name}"] = (sm, dict(stream=lambda d, i, s=st: deflate(d, level=6, strategy=s)), f"strategy Z_{name.upper()}")
    # chunk i: CINFO i + 1 (wbits 9-15); the last chunk CINFO 0 on a Huffman-only stream (no distances)
    wb = {"Y": (1, W._smooth(125, 80, 3))}
    c["zip_cinfo"] = (wb, dict(stream=lambda d, i: deflate(d, level=9, wbits=9 + i) if i < 7 else
                               with_cinfo(deflate(d, level=9, strategy=zlib.Z_HUFFMAN_ONLY, wbits=9), 0)),
                      "every CINFO 0-7, one per chunk")
    c["zip_sync_flush"] = (sm, dict(stream=lambda d, i: deflate(d, flush=zlib.Z_SYNC_FLUSH, pieces=5)),
                           "sync flushes: several Huffman blocks and empty stored blocks per chunk")
    c["zip_full_flush"] = (sm, dict(stream=lambda d, i: deflate(d, level=9, flush=zlib.Z_FULL_FLUSH, pieces=3)),
                           "full flushes")
    c["zip_stored_chunk"] = (sm, dict(store_chunks=(1,)), "chunk 1 stored uncompressed")
    one = {"Y": (1, W._smooth(37, 1, 4))}
    c["zip_1px"] = (one, dict(compression="zip"), "1 pixel wide, ZIP")
    c["zips_1px"] = (one, dict(compression="zips"), "1 pixel wide, ZIPS")
    yy, xx = np.mgrid[0:35, 0:70]
    u = (3_000_000_000 + 977 * xx + 31 * yy).astype(np.uint32)
    multi = {"A": (1, W._smooth(35, 70, 5)), "B": (2, W._smooth(35, 70, 6) * 3.0), "G": (0, u), "R": (1, W._smooth(35, 70, 7))}
    multi["B"][1][3, 4], multi["B"][1][9, 9] = np.nan, -np.inf
    c["zip_multi_float"] = (multi, dict(compression="zip"), "HALF A, FLOAT B (picked), UINT G, HALF R")
    c["zips_uint"] = ({"Y": (0, u), "Z": (2, W._smooth(35, 70, 8))}, dict(compression="zips"), "UINT Y picked, ZIPS")
    c["none_multi"] = (multi, dict(compression="none"), "NONE, several channels")
    wide = {k: (2, W._smooth(20, 1280, 10 + i) + i) for i, k in enumerate("ABGR")}
    c["zip_wide_rgba"] = (wide, dict(compression="zip"), "RGBA FLOAT 1280 wide: 327 680-byte chunks, beyond LDS")
    c["zip_wide_level0"] = (wide, dict(stream=lambda d, i: deflate(d, level=0)), "the same, level 0: many stored blocks")
    out = {}
    for name, (chans, kw, what) in c.items():
        buf = write_zip_exr(chans, **kw)
        comp = exr._parse_header(buf)["compression"]
        bpl = sum(exr._PIXEL_SIZE[pt] for pt, _ in chans.values()) * next(iter(chans.values()))[1].shape[1]
        info = []
        H = next(iter(chans.values()))[1].shape[0]
        for y0, blk in chunks(buf):
            ny = min(_LINES[comp], H - (y0 - kw.get("window", (0, 0))[1]))
            stored = comp == 0 or len(blk) == bpl * ny
            info.append(dict(stored=stored, cinfo=None if stored else blk[0] >> 4, size=len(blk)))
        out[name] = (buf, chans, what, info)
    return out
