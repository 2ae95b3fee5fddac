"""A numpy restatement of csrc/jpeg_enc.hip that produces whole files: libjpeg's integer colour conversion (jccolor.c), h2v2
downsampling (jcsample.c), edge handling (jcprepct.c / jccoefct.c), ISLOW forward DCT (jfdctint.c), quantiser (jcdctmgr.c), quality
scaling (jcparam.c) and sequential Huffman coding with the Annex K.3 tables (jchuff.c), plus the file layout of
``sceneego_amd.jpeg_encode``.  Written independently of the package's encoder: only the zigzag order and the Annex K.3 Huffman
tables are taken from ``sceneego_amd.jpeg_device``.  Meant for small images (pure Python per coefficient in the entropy coder).

Edges, as libjpeg has them (``ceil`` throughout):
  * every component's plane is filled by replicating the last column / row of its own samples out to whole 8x8 blocks; the
    4:2:0 chroma planes replicate the last full-resolution column and row pair *before* the 2x2 average (so an odd width averages
    the last column with itself) and the last *downsampled* row below that;
  * a 4:2:0 MCU holds 2x2 luma blocks; a luma block that lies wholly outside ceil(W/8) x ceil(H/8) blocks is a dummy block: all
    AC coefficients zero and the DC of the block before it in the MCU (right edge: its left neighbour; bottom edge: the last
    block of the MCU's upper row).
"""
from __future__ import annotations

import struct

import numpy as np

from sceneego_amd.jpeg_device import _STD_HUFF, ZIGZAG

# Annex K.1 / K.2, natural order
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
                     51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121,
                     120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99,
                       99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64)


def quant_tables(quality):
    """(luma, chroma) int64 [64] natural order: jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA, STD_CHROMA))


def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(rgb):
    """uint8 [H,W,3] R, G, B -> int64 Y, Cb, Cr planes (jccolor.c rgb_ycc_convert)."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + 32768) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, h, w):
    """Replicate the last row / column of ``plane`` out to [h, w]."""
    return np.pad(plane, ((0, h - plane.shape[0]), (0, w - plane.shape[1])), mode="edge")


def h2v2(plane):
    """jcsample.c h2v2_downsample of a plane with even height and width: bias 1, 2, 1, 2 ... along a row."""
    s = plane[0::2, 0::2] + plane[0::2, 1::2] + plane[1::2, 0::2] + plane[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias[None, :]) >> 2


C = {"0_298631336": 2446, "0_390180644": 3196, "0_541196100": 4433, "0_765366865": 6270, "0_899976223": 7373, "1_175875602": 9633,
     "1_501321110": 12299, "1_847759065": 15137, "1_961570560": 16069, "2_053119869": 16819, "2_562915447": 20995,
     "3_072711026": 25172}


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """One pass of jfdctint.c on d [..., 8] (last axis), int64."""
    tmp0, tmp7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    tmp1, tmp6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    tmp2, tmp5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    tmp3, tmp4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    out = [None] * 8
    if first:
        out[0], out[4] = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
        n = 11
    else:
        out[0], out[4] = _descale(tmp10 + tmp11, 2), _descale(tmp10 - tmp11, 2)
        n = 15
    z1 = (tmp12 + tmp13) * C["0_541196100"]
    out[2] = _descale(z1 + tmp13 * C["0_765366865"], n)
    out[6] = _descale(z1 + tmp12 * (-C["1_847759065"]), n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * C["1_175875602"]
    tmp4, tmp5, tmp6, tmp7 = tmp4 * C["0_298631336"], tmp5 * C["2_053119869"], tmp6 * C["3_072711026"], tmp7 * C["1_501321110"]
    z1, z2 = z1 * (-C["0_899976223"]), z2 * (-C["2_562915447"])
    z3, z4 = z3 * (-C["1_961570560"]) + z5, z4 * (-C["0_390180644"]) + z5
    out[7], out[5], out[3], out[1] = (_descale(tmp4 + z1 + z3, n), _descale(tmp5 + z2 + z4, n), _descale(tmp6 + z2 + z3, n),
                                      _descale(tmp7 + z1 + z4, n))
    return np.stack(out, axis=-1)


def fdct_quant(blocks, q):
    """int64 [n, 8, 8] samples (0..255), q int64 [64] natural -> quantised coefficients int64 [n, 64] natural order."""
    d = blocks.astype(np.int64) - 128
    d = _fdct_1d(d, True)                                        # rows
    d = np.swapaxes(_fdct_1d(np.swapaxes(d, 1, 2), False), 1, 2)  # columns
    c = d.reshape(-1, 64)
    div = 8 * q[None, :]
    mag = (np.abs(c) + (div >> 1)) // div
    return np.where(c < 0, -mag, mag)


def _blocks(plane, by, bx):
    return plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8]


def coefficients(rgb, quality, subsampling):
    """Quantised coefficients of one frame in MCU (scan) order: (int64 [n_blocks, 64] natural order with absolute DC, component of
    every block of an MCU, mcus_x, mcus_y)."""
    H, W = rgb.shape[:2]
    ql, qc = quant_tables(quality)
    y, cb, cr = rgb_to_ycc(rgb)
    if subsampling == "444":
        mx, my = -(-W // 8), -(-H // 8)
        pl = [_pad(p, 8 * my, 8 * mx) for p in (y, cb, cr)]
        comp = [0, 1, 2]
        rows = []
        for m in range(mx * my):
            for c in range(3):
                rows.append(_blocks(pl[c], m // mx, m % mx))
        blocks = np.stack(rows)
        q = [ql, qc, qc]
        coef = np.concatenate([fdct_quant(blocks[i::3], q[i])[:, None] for i in range(3)], axis=1).reshape(-1, 64)
        return coef, comp, mx, my
    if subsampling != "420":
        raise ValueError(subsampling)
    mx, my = -(-W // 16), -(-H // 16)
    wb, hb = -(-W // 8), -(-H // 8)                    # real luma blocks
    yp = _pad(y, 8 * hb, 8 * wb)
    hc, wc = -(-H // 2), -(-W // 2)
    chroma = []
    for p in (cb, cr):
        full = _pad(p, 2 * hc, 16 * mx)                # the last column out to the MCU grid, the last row to an even count
        chroma.append(_pad(h2v2(full), 8 * my, 8 * mx))    # the last downsampled row below
    out = np.zeros((mx * my * 6, 64), dtype=np.int64)
    for m in range(mx * my):
        r, c = m // mx, m % mx
        for k in range(4):
            by, bx = 2 * r + (k >> 1), 2 * c + (k & 1)
            if by < hb and bx < wb:
                out[6 * m + k] = fdct_quant(_blocks(yp, by, bx)[None], ql)[0]
            else:
                out[6 * m + k, 0] = out[6 * m + k - 1, 0]      # dummy block
        out[6 * m + 4] = fdct_quant(_blocks(chroma[0], r, c)[None], qc)[0]
        out[6 * m + 5] = fdct_quant(_blocks(chroma[1], r, c)[None], qc)[0]
    return out, [0, 0, 0, 0, 1, 2], mx, my


def _enc_table(key):
    """(code, length) per symbol of an Annex K.3 table (jpeg_make_c_derived_tbl)."""
    bits, vals = _STD_HUFF[key]
    code, p, tab = 0, 0, {}
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            tab[vals[p]] = (code, ln)
            code += 1
            p += 1
        code <<= 1
    return tab


ENC = {k: _enc_table(k) for k in _STD_HUFF}


class Stats:
    """What a scan exercised (filled by ``entropy_code``)."""

    def __init__(self):
        self.zrl = self.no_eob = self.stuffed = self.pad_bits = 0
        self.max_ac_cat = self.max_dc_cat = 0
        self.blocks = 0


def _emit_block(bits, coef_zz, diff, comp, st):
    dc, ac = ENC[(0, 1 if comp else 0)], ENC[(1, 1 if comp else 0)]

    def put(v, n):
        bits.append((v, n))

    def cat_bits(v):
        a = abs(v)
        n = a.bit_length()
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    n, x = cat_bits(diff)
    st.max_dc_cat = max(st.max_dc_cat, n)
    put(*dc[n])
    if n:
        put(x, n)
    run = 0
    for k in range(1, 64):
        v = int(coef_zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            put(*ac[0xF0])
            st.zrl += 1
            run -= 16
        n, x = cat_bits(v)
        st.max_ac_cat = max(st.max_ac_cat, n)
        put(*ac[(run << 4) | n])
        put(x, n)
        run = 0
    if run > 0:
        put(*ac[0])
    else:
        st.no_eob += 1
    st.blocks += 1


def entropy_code(coef, comp, mcus_x, mcus_y, restart_rows, stats=None):
    """Scan bytes (stuffed, RSTm markers and padding included) of coefficient rows in MCU order."""
    st = stats if stats is not None else Stats()
    bpm = len(comp)
    per = restart_rows * mcus_x if restart_rows else mcus_x * mcus_y
    out = bytearray()
    n_mcu = mcus_x * mcus_y
    for seg, m0 in enumerate(range(0, n_mcu, per)):
        if seg:
            out += bytes([0xFF, 0xD0 + ((seg - 1) & 7)])
        last = [0, 0, 0]
        bits = []
        for m in range(m0, min(m0 + per, n_mcu)):
            for k in range(bpm):
                row = coef[m * bpm + k]
                c = comp[k]
                _emit_block(bits, row[ZIGZAG], int(row[0]) - last[c], c, st)
                last[c] = int(row[0])
        acc = nacc = 0
        for v, n in bits:
            acc = (acc << n) | v
            nacc += n
        if nacc & 7:
            pad = 8 - (nacc & 7)
            st.pad_bits += pad
            acc = (acc << pad) | ((1 << pad) - 1)
            nacc += pad
        raw = acc.to_bytes(nacc // 8, "big")
        st.stuffed += raw.count(b"\xff")
        out += raw.replace(b"\xff", b"\xff\x00")
    return bytes(out)


def headers(H, W, ql, qc, subsampling, restart_mcus):
    """SOI .. SOS header of a file, as ``sceneego_amd.jpeg_encode`` (and libjpeg with default settings) lay it out."""
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for i, q in enumerate((ql, qc)):
        out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(int(v) for v in np.asarray(q)[ZIGZAG])
    hv = 0x22 if subsampling == "420" else 0x11
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, H, W, 3) + bytes([1, hv, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls, t in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = _STD_HUFF[(cls, t)]
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), (cls << 4) | t) + bytes(bits) + bytes(vals)
    if restart_mcus:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart_mcus)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return bytes(out)


def encode(rgb, quality=90, subsampling="444", restart_rows=0, stats=None):
    """One complete baseline JPEG file of uint8 [H,W,3] (R, G, B)."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    ql, qc = quant_tables(quality)
    coef, comp, mx, my = coefficients(rgb, quality, subsampling)
    scan = entropy_code(coef, comp, mx, my, restart_rows, stats)
    return headers(H, W, ql, qc, subsampling, restart_rows * mx if restart_rows else 0) + scan + b"\xff\xd9"


def scan_of(jpeg_bytes):
    """The bytes after the SOS header up to (not including) EOI."""
    i = jpeg_bytes.index(b"\xff\xda")
    (n,) = struct.unpack_from(">H", jpeg_bytes, i + 2)
    assert jpeg_bytes[-2:] == b"\xff\xd9"
    return jpeg_bytes[i + 2 + n:-2]


def dqt_of(jpeg_bytes):
    """{table id: bytes in file (zigzag) order} of an 8-bit-table file."""
    out, pos = {}, 2
    while jpeg_bytes[pos + 1] != 0xDA:
        (n,) = struct.unpack_from(">H", jpeg_bytes, pos + 2)
        if jpeg_bytes[pos + 1] == 0xDB:
            body = jpeg_bytes[pos + 4:pos + 2 + n]
            for q in range(0, len(body), 65):
                out[body[q] & 15] = bytes(body[q + 1:q + 65])
        pos += 2 + n
    return out
