"""Test-side OpenEXR writer: single-part scanline files with PIZ, ZIP or NONE compression, from the published specification
(ImfPizCompressor: bitmap -> forward LUT -> wav2Encode with wenc14 / wenc16 -> canonical Huffman with the run-length symbol;
ImfHuf: hufPackEncTable / hufEncode).  It exists to give the decoders ground they have never seen: odd sizes, non-zero data
windows, several channels, FLOAT / UINT halves, stored chunks, long runs, wdec16 data and 58-bit codes.

``write_exr(channels, ...)`` -> file bytes.  ``channels``: {name: (pixel type, [H, W] array)}, pixel type 0 UINT, 1 HALF, 2 FLOAT.
``lengths="skew"`` replaces the Huffman code lengths by a Kraft-complete comb (1, 2, ..., 57, 58, 58, split further when the
alphabet is larger), so the least frequent symbols get 58-bit codes.  ``STATS["max_len"]`` is the longest code the last
``write_exr`` call emitted into a bitstream.
"""
from __future__ import annotations

import heapq
import struct
import zlib

import numpy as np

HUF_ENCSIZE = 65537
SHORT_ZEROCODE_RUN = 59
LONG_ZEROCODE_RUN = 63
SHORTEST_LONG_RUN = 2 + LONG_ZEROCODE_RUN - SHORT_ZEROCODE_RUN
LONGEST_LONG_RUN = 255 + SHORTEST_LONG_RUN
BITMAP_SIZE = 8192
_PIXEL_SIZE = {0: 4, 1: 2, 2: 4}
_COMP = {"none": 0, "zip": 3, "piz": 4}
_LINES = {0: 1, 3: 16, 4: 32}
STATS = {"max_len": 0, "stored": 0, "w16": 0, "max_run": 0}


# ------------------------------------------------------------------------------------------------
# wavelet (ImfWav wav2Encode)
# ------------------------------------------------------------------------------------------------
def _wenc14(a, b):
    as_ = a.astype(np.uint16).view(np.int16).astype(np.int32)
    bs = b.astype(np.uint16).view(np.int16).astype(np.int32)
    ms = (as_ + bs) >> 1
    ds = as_ - bs
    return (ms & 0xFFFF).astype(np.uint16), (ds & 0xFFFF).astype(np.uint16)


def _wenc16(a, b):
    ao = (a.astype(np.int32) + (1 << 15)) & 0xFFFF
    bi = b.astype(np.int32)
    m = (ao + bi) >> 1
    d = ao - bi
    m = np.where(d < 0, (m + (1 << 15)) & 0xFFFF, m)
    return m.astype(np.uint16), (d & 0xFFFF).astype(np.uint16)


def wav2_encode(img: np.ndarray, mx: int) -> None:
    ny, nx = img.shape
    wenc = _wenc14 if mx < (1 << 14) else _wenc16
    n = min(nx, ny)
    p, p2 = 1, 2
    while p2 <= n:
        ys = np.arange(0, ny - p2 + 1, p2)
        xs = np.arange(0, nx - p2 + 1, p2)
        if len(ys) and len(xs):
            Y, X = np.meshgrid(ys, xs, indexing="ij")
            i00, i01 = wenc(img[Y, X], img[Y, X + p])
            i10, i11 = wenc(img[Y + p, X], img[Y + p, X + p])
            img[Y, X], img[Y + p, X] = wenc(i00, i10)
            img[Y, X + p], img[Y + p, X + p] = wenc(i01, i11)
        if nx & p and len(ys):
            x = len(xs) * p2
            img[ys, x], img[ys + p, x] = wenc(img[ys, x], img[ys + p, x])
        if ny & p and len(xs):
            y = len(ys) * p2
            img[y, xs], img[y, xs + p] = wenc(img[y, xs], img[y, xs + p])
        p = p2
        p2 <<= 1


# ------------------------------------------------------------------------------------------------
# Huffman (ImfHuf)
# ------------------------------------------------------------------------------------------------
def _huffman_lengths(freq: dict) -> dict:
    if len(freq) == 1:
        return {next(iter(freq)): 1}
    heap = [(f, s, [s]) for s, f in freq.items()]
    heapq.heapify(heap)
    length = dict.fromkeys(freq, 0)
    while len(heap) > 1:
        f1, k1, m1 = heapq.heappop(heap)
        f2, k2, m2 = heapq.heappop(heap)
        for s in m1 + m2:
            length[s] += 1
        heapq.heappush(heap, (f1 + f2, min(k1, k2), m1 + m2))
    return length


def _skew_lengths(freq: dict) -> dict:
    """Kraft-complete comb with a 58-bit bottom: depths 1..57 once, 58 twice; split the deepest leaf above 58 while symbols remain."""
    cnt = [0] * 59
    for d in range(1, 58):
        cnt[d] = 1
    cnt[58] = 2
    total = 59
    while total < len(freq):
        d = max(i for i in range(58) if cnt[i] > 0)
        cnt[d] -= 1
        cnt[d + 1] += 2
        total += 1
    while total > len(freq):               # fewer symbols than leaves: merge the two deepest into their parent
        d = max(i for i in range(59) if cnt[i] > 0)
        if cnt[d] < 2:
            raise ValueError("alphabet too small for a skewed code")
        cnt[d] -= 2
        cnt[d - 1] += 1
        total -= 1
    depths = [d for d in range(59) for _ in range(cnt[d])]
    order = sorted(freq, key=lambda s: (-freq[s], s))
    return dict(zip(order, depths))


def _canonical(lengths: dict) -> dict:
    n = [0] * 59
    for l in lengths.values():
        n[l] += 1
    c, start = 0, [0] * 59
    for i in range(58, 0, -1):
        nc = (c + n[i]) >> 1
        start[i] = c
        c = nc
    codes = {}
    for s in sorted(lengths):
        l = lengths[s]
        codes[s] = (start[l], l)
        start[l] += 1
    return codes


def _pack_table(lengths: dict, im: int, iM: int) -> bytes:
    bits = []
    i = im
    while i <= iM:
        l = lengths.get(i, 0)
        if l == 0:
            zerun = 1
            while i < iM and zerun < LONGEST_LONG_RUN and lengths.get(i + 1, 0) == 0:
                i += 1
                zerun += 1
            if zerun >= 2:
                if zerun >= SHORTEST_LONG_RUN:
                    bits.append(format(LONG_ZEROCODE_RUN, "06b") + format(zerun - SHORTEST_LONG_RUN, "08b"))
                else:
                    bits.append(format(SHORT_ZEROCODE_RUN + zerun - 2, "06b"))
                i += 1
                continue
        bits.append(format(l, "06b"))
        i += 1
    return _bits_to_bytes("".join(bits))


def _bits_to_bytes(s: str) -> bytes:
    if not s:
        return b""
    pad = (-len(s)) % 8
    return int(s + "0" * pad, 2).to_bytes((len(s) + pad) // 8, "big")


def huf_compress(words: np.ndarray, lengths_mode: str = "huffman") -> bytes:
    words = [int(w) for w in words]
    freq = {}
    for w in words:
        freq[w] = freq.get(w, 0) + 1
    im, iM = min(freq), max(freq)
    rlc = iM + 1
    freq[rlc] = 1
    iM = rlc
    lengths = (_skew_lengths if lengths_mode == "skew" else _huffman_lengths)(freq)
    codes = _canonical(lengths)
    fmt = {s: format(c, f"0{l}b") for s, (c, l) in codes.items()}
    out, used = [], 0

    def send(s, run):
        nonlocal used
        l, lr = lengths[s], lengths[rlc]
        if l + lr + 8 < l * run:
            out.append(fmt[s] + fmt[rlc] + format(run, "08b"))
            used = max(used, l, lr)
        else:
            out.append(fmt[s] * (run + 1))
            used = max(used, l)

    run = 1
    for a, b in zip(words, words[1:]):
        run = run + 1 if a == b else 1
        STATS["max_run"] = max(STATS["max_run"], run)
    s, cs = words[0], 0
    for w in words[1:]:
        if w == s and cs < 255:
            cs += 1
        else:
            send(s, cs)
            cs = 0
        s = w
    send(s, cs)
    stream = "".join(out)
    STATS["max_len"] = max(STATS["max_len"], used)
    table = _pack_table(lengths, im, iM)
    return struct.pack("<IIIII", im, iM, len(table), len(stream), 0) + table + _bits_to_bytes(stream)


# ------------------------------------------------------------------------------------------------
# chunks
# ------------------------------------------------------------------------------------------------
def _words(ptype: int, rows: np.ndarray) -> np.ndarray:
    """[ny, W] pixels -> [ny, W * words per pixel] little-endian 16-bit words."""
    if ptype == 1:
        return np.ascontiguousarray(rows.astype(np.float16)).view(np.uint16)
    dt = np.uint32 if ptype == 0 else np.float32
    return np.ascontiguousarray(rows.astype(dt)).view(np.uint32).view(np.uint16).reshape(rows.shape[0], -1)


def _raw_lines(chans, y0, ny) -> bytes:
    out = bytearray()
    for r in range(ny):
        for _, ptype, arr in chans:
            out += _words(ptype, arr[y0 + r:y0 + r + 1]).astype("<u2").tobytes()
    return bytes(out)


def _piz_block(chans, y0, ny, lengths_mode) -> bytes:
    planes = [(_PIXEL_SIZE[pt] // 2, _words(pt, arr[y0:y0 + ny])) for _, pt, arr in chans]
    allw = np.concatenate([p.reshape(-1) for _, p in planes])
    bitmap = np.zeros(BITMAP_SIZE * 8, dtype=bool)
    bitmap[allw] = True
    bitmap[0] = False                                  # zero is implied
    bm = np.packbits(bitmap, bitorder="little")
    nz = np.nonzero(bm)[0]
    min_nz, max_nz = (int(nz[0]), int(nz[-1])) if len(nz) else (BITMAP_SIZE - 1, 0)
    bitmap[0] = True
    present = np.nonzero(bitmap)[0]
    fwd = np.zeros(65536, dtype=np.uint16)
    fwd[present] = np.arange(len(present), dtype=np.uint16)
    mx = len(present) - 1
    if mx >= (1 << 14):
        STATS["w16"] += 1
    coded = []
    for s, p in planes:
        p = fwd[p]
        if s == 1:
            wav2_encode(p, mx)
        else:
            for j in range(s):
                sub = np.ascontiguousarray(p[:, j::s])
                wav2_encode(sub, mx)
                p[:, j::s] = sub
        coded.append(p.reshape(-1))
    huf = huf_compress(np.concatenate(coded), lengths_mode)
    head = struct.pack("<HH", min_nz, max_nz)
    if min_nz <= max_nz:
        head += bm[min_nz:max_nz + 1].tobytes()
    return head + struct.pack("<i", len(huf)) + huf


def _zip_block(raw: bytes) -> bytes:
    t = np.frombuffer(raw, dtype=np.uint8)
    inter = np.concatenate([t[0::2], t[1::2]]).astype(np.int32)
    d = inter.copy()
    d[1:] = (inter[1:] - inter[:-1] + 128) & 0xFF
    return zlib.compress(d.astype(np.uint8).tobytes())


def _attr(name, typ, data):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(data)) + data


def write_exr(channels: dict, compression: str = "piz", window=(0, 0), lengths: str = "huffman", store_chunks=(),
              store_larger=True) -> bytes:
    """channels {name: (pixel type, [H, W] array)} -> OpenEXR file bytes.  ``store_chunks``: chunk indices written uncompressed;
    ``store_larger=False`` keeps a compressed block even where it is larger than the raw lines (never of the same size: a reader
    takes that for a stored chunk)."""
    STATS.update(max_len=0, stored=0, w16=0, max_run=0)
    chans = sorted((n, pt, np.asarray(a)) for n, (pt, a) in channels.items())
    H, W = chans[0][2].shape
    xmin, ymin = window
    comp = _COMP[compression]
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", pt, 0, 1, 1) for n, pt, _ in chans) + b"\0"
    hdr = b"\x76\x2f\x31\x01" + struct.pack("<I", 2)
    hdr += _attr("channels", "chlist", chlist)
    hdr += _attr("compression", "compression", bytes([comp]))
    hdr += _attr("dataWindow", "box2i", struct.pack("<iiii", xmin, ymin, xmin + W - 1, ymin + H - 1))
    hdr += _attr("displayWindow", "box2i", struct.pack("<iiii", xmin, ymin, xmin + W - 1, ymin + H - 1))
    hdr += _attr("lineOrder", "lineOrder", b"\0")
    hdr += _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    hdr += _attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0))
    hdr += _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    lpc = _LINES[comp]
    n_chunks = (H + lpc - 1) // lpc
    blocks = []
    for i in range(n_chunks):
        y0 = i * lpc
        ny = min(lpc, H - y0)
        raw = _raw_lines(chans, y0, ny)
        if comp == 0:
            data = raw
        elif comp == 3:
            data = _zip_block(raw)
        else:
            data = _piz_block(chans, y0, ny, lengths)
        if comp and not store_larger and i not in store_chunks:
            assert len(data) != len(raw)
        if i in store_chunks or (store_larger and len(data) >= len(raw)):
            data = raw
            STATS["stored"] += 1
        blocks.append(struct.pack("<ii", ymin + y0, len(data)) + data)
    pos = len(hdr) + 8 * n_chunks
    offsets = []
    for b in blocks:
        offsets.append(pos)
        pos += len(b)
    return hdr + struct.pack(f"<{n_chunks}Q", *offsets) + b"".join(blocks)


# ------------------------------------------------------------------------------------------------
# the cases the tests decode
# ------------------------------------------------------------------------------------------------
def _smooth(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = 1.5 + 0.011 * xx + 0.017 * yy + 0.05 * np.sin(xx / 7.0) + rng.normal(0, 0.002, (h, w))
    return (np.round(d * 1024) / 1024).astype(np.float32)


def make_cases():
    """{name: (file bytes, {channel: (pixel type, array)}, what it covers)}; every array holds what the file stores."""
    c = {}
    d = _smooth(77, 333, 1)
    d[5, 7], d[6, 8], d[70, 300], d[40, 3] = np.nan, np.inf, 12.5, -np.inf
    d[50:77, 10:320] = 11.0                                        # above 10 m; constant block
    c["odd_window"] = ({"Y": (1, d)}, dict(window=(5, -3)), "333x77, data window at (5, -3), 13-row last chunk, NaN / inf / >10 m")
    bits = (np.arange(64 * 640, dtype=np.int64) * 7 % 65536).astype(np.uint16).reshape(64, 640)
    c["w16"] = ({"Y": (1, bits.view(np.float16))}, {}, "max_value >= 2^14: wdec16")
    bgr = {k: (1, _smooth(40, 200, i) + i) for i, k in enumerate("BGR")}
    bgr["Z"] = (2, _smooth(40, 200, 9) * 3.0)
    c["bgr_z"] = (bgr, {}, "BGR HALF + FLOAT Z: B is picked")
    z = _smooth(70, 96, 4) * 2.0
    z[3, 3], z[60, 90] = np.nan, np.inf
    c["float_z"] = ({"Z": (2, z)}, {}, "FLOAT-only Z: two 16-bit halves transformed independently")
    c["stored"] = ({"Y": (1, _smooth(64, 128, 5))}, dict(store_chunks=(1,)), "chunk 1 stored uncompressed")
    r = _smooth(64, 640, 6)
    r[:32] = 4.0
    c["runs"] = ({"Y": (1, r)}, {}, "a constant chunk: runs over 255 split into 8-bit counts")
    sk = np.random.default_rng(7).uniform(1.0, 9.0, (32, 64)).astype(np.float32)
    c["skew58"] = ({"Y": (1, sk)}, dict(lengths="skew", store_larger=False), "a skewed length set with 58-bit codes")
    c["a_y"] = ({"A": (1, _smooth(33, 50, 8)), "Y": (1, _smooth(33, 50, 9) + 2)}, {}, "Y after A: the plane after another")
    yy, xx = np.mgrid[0:35, 0:70]
    u = (3_000_000_000 + 977 * xx + 31 * yy).astype(np.uint32)       # above 2^24: rounded to float32
    u[:, :20] = 123456789
    c["uint"] = ({"Y": (0, u)}, dict(store_larger=False), "UINT channel, rounded to float32")
    out = {}
    for name, (chans, kw, what) in c.items():
        out[name] = (write_exr(chans, **kw), chans, what, dict(STATS))
    return out


def expected_planes(chans):
    """What a decoder must return for each channel: HALF through float16, FLOAT as is, UINT rounded to float32."""
    e = {}
    for name, (pt, a) in chans.items():
        if pt == 1:
            e[name] = np.asarray(a).astype(np.float16).astype(np.float32)
        elif pt == 2:
            e[name] = np.asarray(a, dtype=np.float32)
        else:
            e[name] = np.asarray(a).astype(np.uint32).astype(np.float32)
    return e
