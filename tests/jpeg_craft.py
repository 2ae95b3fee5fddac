"""A test-side writer of sequential (SOF0 / SOF1) JPEG files from quantised coefficients, for the decoder tests: pure Python / numpy, no
PIL.  It writes what an ordinary encoder never does: any Huffman table set (ids 0..3, long codes, a table defined twice), 8- or 16-bit
quantisation tables with ids 0..3, any frame / scan component list, any restart interval, fill bytes, either kind of padding bits,
and raw blocks whose symbols are emitted without any consistency check (runs past coefficient 63, DC sums that leave 16 bits).

Only the zigzag order and the Annex K.3 tables are taken from ``sceneego_amd.jpeg_device``; nothing here shares code with the decoder
or with ``tests/jpeg_model.py``.
"""
from __future__ import annotations

import struct

import numpy as np

from sceneego_amd.jpeg_device import _STD_HUFF, ZIGZAG

ZRL = "ZRL"        # raw symbol 0xF0: sixteen zeros
EOB = "EOB"        # raw symbol 0x00: end of block

AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]     # the 162 symbols of a baseline AC table


def std_table(cls, tid):
    bits, vals = _STD_HUFF[(cls, tid)]
    return list(bits), bytes(vals)


def canonical_table(symbols, minlen=1, spread=False):
    """(bits[1..16], vals) of a valid canonical Huffman table for ``symbols`` in which every code is at least ``minlen`` bits long
    and the all-ones code of the longest length stays unused (libjpeg and ``HuffTable`` refuse a table that uses it: a complete
    table of 16 symbols therefore needs 5-bit codes).  ``spread``: share the symbols out over the lengths minlen..16 instead of
    giving them all the shortest length that holds them."""
    symbols = list(symbols)
    n = len(symbols)
    if not 0 < n <= 256 or len(set(symbols)) != n:
        raise ValueError("canonical_table: 1..256 distinct symbols")
    bits = [0] * 16
    if spread:
        lens = list(range(minlen, 17))
        per = n // len(lens)
        for ln in lens[:-1]:
            bits[ln - 1] = min(per, (1 << ln) // 4)           # at most a quarter of the code space per length: never oversubscribed
        bits[15] = n - sum(bits)
    else:
        ln = max(minlen, n.bit_length())                      # n <= 2^ln - 1
        if ln > 16:
            raise ValueError("canonical_table: too many symbols")
        bits[ln - 1] = n
    code = 0
    for ln in range(1, 17):                                   # the check of jpeg_make_d_derived_tbl
        code += bits[ln - 1]
        if code >= (1 << ln):
            raise ValueError(f"canonical_table: oversubscribed at length {ln}")
        code <<= 1
    return bits, bytes(symbols)


def code_table(bits, vals):
    """{symbol: (code, length)} of a (bits, vals) table (jpeg_make_c_derived_tbl)."""
    code, p, tab = 0, 0, {}
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            tab[vals[p]] = (code, ln)
            code += 1
            p += 1
        code <<= 1
    return tab


def _cat_bits(v):
    n = abs(int(v)).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def com(text):
    return b"\xff\xfe" + struct.pack(">H", len(text) + 2) + bytes(text)


def appn(n, body):
    return bytes([0xFF, 0xE0 + n]) + struct.pack(">H", len(body) + 2) + bytes(body)


class Raw:
    """One block given as symbols: a DC difference, then ``(run, value)`` pairs, ``ZRL`` and ``EOB``; written as they stand."""

    def __init__(self, dc_diff, symbols):
        self.dc_diff, self.symbols = int(dc_diff), list(symbols)


def _emit_block(put, dc, ac, diff, symbols):
    n, x = _cat_bits(diff)
    put(*dc[n])
    if n:
        put(x, n)
    for s in symbols:
        if s is ZRL or s == ZRL:
            put(*ac[0xF0])
        elif s is EOB or s == EOB:
            put(*ac[0x00])
        else:
            run, v = s
            n, x = _cat_bits(v)
            if not (0 <= run <= 15 and 1 <= n <= 15):
                raise ValueError(f"raw symbol {s}")
            put(*ac[(run << 4) | n])
            put(x, n)


def block_symbols(coef_zz):
    """The (run, value) / ZRL / EOB symbols of one block's AC coefficients in zigzag order, as jchuff.c codes them."""
    out, run = [], 0
    for k in range(1, 64):
        v = int(coef_zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(ZRL)
            run -= 16
        out.append((run, v))
        run = 0
    if run:
        out.append(EOB)
    return out


def write_jpeg(H, W, comps, coefs, quant, *, scan=None, dht=None, sof=0xC0, restart=0, jfif=True, adobe=None, extra=b"", pad_ones=True,
               rst_fill=0, raw=None, eoi=True, info=None):
    """One sequential JPEG file.

    comps    frame components [(id, h, v, quantisation table id)]; one component is written as libjpeg reads it (one 8x8 block per MCU)
    coefs    per component int [block rows, block cols, 64], natural order, absolute DC; the block grid is the padded MCU grid
             (MCU rows * v, MCUs per row * h)
    quant    {id: (int [64] natural order, 16-bit?)} in the order they are written
    scan     [(frame index, DC table id, AC table id)]; default: every component in frame order, tables 0 for the first, 1 for the others
    dht      [((class, id), (bits, vals))] written in this order, a later entry redefining an earlier one (the encoder uses the last);
             default: the Annex K.3 tables the scan names
    sof      0xC0 or 0xC1           restart  DRI value (0: no DRI)
    jfif     write a JFIF APP0      adobe    transform byte of an Adobe APP14 (None: no APP14)
    extra    bytes written before the first DQT (COM / APPn segments, 0xFF fill bytes before the next marker)
    pad_ones pad every segment's last byte with 1 bits (else 0 bits)
    rst_fill 0xFF fill bytes before every RSTn
    raw      {(frame index, block row, block col): Raw}: these blocks are written from their symbols; the DC predictor follows
             every difference as an exact integer, and an ordinary block's difference is its DC minus the predictor modulo 2^16
    info     a dict that receives ``segments``: [(first byte, end byte)] of every entropy-coded segment in the file
    """
    nf = len(comps)
    raw = raw or {}
    if scan is None:
        scan = [(i, min(i, 1), min(i, 1)) for i in range(nf)]
    if dht is None:
        dht = []
        for _, td, ta in scan:
            for key in ((0, td), (1, ta)):
                if key not in [k for k, _ in dht]:
                    dht.append((key, std_table(*key)))
    enc = {key: code_table(bits, vals) for key, (bits, vals) in dht}        # the last definition wins
    for key in _STD_HUFF:
        enc.setdefault(key, code_table(*std_table(*key)))
    if nf == 1:
        hs, vs = [1], [1]
    else:
        hs, vs = [c[1] for c in comps], [c[2] for c in comps]
    hmax, vmax = max(hs), max(vs)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    for i, c in enumerate(coefs):
        if tuple(np.shape(c)) != (my * vs[i], mx * hs[i], 64):
            raise ValueError(f"component {i}: coefficients {np.shape(c)}, expected {(my * vs[i], mx * hs[i], 64)}")
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += appn(0, struct.pack(">5sBBBHHBB", b"JFIF\0", 1, 1, 0, 1, 1, 0, 0))
    if adobe is not None:
        out += appn(14, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe))
    out += extra
    for tq, (vals, wide) in quant.items():
        zz = np.asarray(vals, dtype=np.int64)[ZIGZAG]
        body = bytes([(0x10 if wide else 0) | tq]) + (zz.astype(">u2").tobytes() if wide else bytes(int(v) for v in zz))
        out += b"\xff\xdb" + struct.pack(">H", len(body) + 2) + body
    out += bytes([0xFF, sof]) + struct.pack(">HBHHB", 8 + 3 * nf, 8, H, W, nf)
    for cid, h, v, tq in comps:
        out += bytes([cid, (h << 4) | v, tq])
    for (cls, tid), (bits, vals) in dht:
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), (cls << 4) | tid) + bytes(bits) + bytes(vals)
    if restart:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart)
    out += b"\xff\xda" + struct.pack(">HB", 6 + 2 * len(scan), len(scan))
    for fi, td, ta in scan:
        out += bytes([comps[fi][0], (td << 4) | ta])
    out += bytes([0, 63, 0])
    n_mcu = mx * my
    per = restart if restart else n_mcu
    segments = []
    for seg, m0 in enumerate(range(0, n_mcu, per)):
        if seg:
            out += b"\xff" * rst_fill + bytes([0xFF, 0xD0 + ((seg - 1) & 7)])
        pred = [0] * nf
        acc = nacc = 0

        def put(v, n):
            nonlocal acc, nacc
            acc = (acc << n) | v
            nacc += n

        for m in range(m0, min(m0 + per, n_mcu)):
            r, c = m // mx, m % mx
            for fi, td, ta in scan:
                for yy in range(vs[fi]):
                    for xx in range(hs[fi]):
                        by, bx = r * vs[fi] + yy, c * hs[fi] + xx
                        blk = raw.get((fi, by, bx))
                        if blk is not None:
                            diff, syms = blk.dc_diff, blk.symbols
                        else:
                            row = np.asarray(coefs[fi][by][bx])
                            # the decoder stores (short)(predictor + difference): the difference is taken modulo 2^16, so a
                            # block after raw differences that carried the predictor away still decodes to its own DC
                            diff = (int(row[0]) - pred[fi] + 32768) % 65536 - 32768
                            syms = block_symbols(row[ZIGZAG])
                        pred[fi] += diff
                        _emit_block(put, enc[(0, td)], enc[(1, ta)], diff, syms)
        if nacc & 7:
            pad = 8 - (nacc & 7)
            acc = (acc << pad) | (((1 << pad) - 1) if pad_ones else 0)
            nacc += pad
        a = len(out)
        out += acc.to_bytes(nacc // 8, "big").replace(b"\xff", b"\xff\x00")
        segments.append((a, len(out)))
    if eoi:
        out += b"\xff\xd9"
    if info is not None:
        info["segments"] = segments
    return bytes(out)
