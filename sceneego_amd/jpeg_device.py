"""Batched baseline JPEG decode on the device: any number of same-sized files -> uint8 [B, H, W, 3] in B, G, R order on a HIP device.

The host part parses the markers (SOI, APPn / COM, DQT, SOF, DHT, DRI, SOS, RSTn, EOI), builds every Huffman table's decode tables
(a 9-bit lookahead table plus maxcode / valoffset per code length), splits the entropy-coded data at its RSTn markers into
segments, strips the 0x00 after every 0xFF with bytes-level operations, validates everything before anything is launched, packs the
descriptors, tables and unstuffed segments into one pinned buffer, copies it to the device in one transfer on the current stream and
launches ``se_jpeg_decode_bgr_u8`` (``csrc/jpeg.hip``: parallel Huffman decode by self-synchronisation, DC prediction, ISLOW IDCT,
fancy upsampling and YCbCr -> BGR).  The result is bit-identical to ``preprocess.load_image_bgr`` (PIL on libjpeg-turbo with its
defaults).  The kernels follow libjpeg's C code; PIL runs libjpeg-turbo's SIMD IDCT, and the two agree on *plain* blocks only: every
dequantised coefficient and every pass-1 workspace value fits int16, every pass-2 value after its descale lies in [-512, 511]
(``tests/jpeg_model.py`` ``plain_blocks`` has the argument; files of any ordinary encoder are far inside).  The IDCT kernel reports
any other block as status 4, and a file whose decode reports any status (a block that is not plain, no matching code, a stream that
ends early: damage libjpeg only warns about) is decoded again by PIL on the host and copied into its slot, so the result equals
``load_image_bgr``'s there too; ``DecodeStatus.redecoded`` lists those slots.  Only when PIL refuses the file as well does the
status raise.

The device path takes baseline or extended sequential (SOF0 / SOF1) Huffman-coded 8-bit files with one scan holding every component:
gray, or three components libjpeg's colour-space guess treats as YCbCr, sampled 4:4:4, 4:2:2 (h2v1) or 4:2:0 (h2v2); any size, any
restart interval, 8- or 16-bit quantisation tables.  Every other file (progressive, arithmetic, lossless, 12-bit, CMYK / YCCK, Adobe
RGB, multi-scan, a scan that lists the components in another order than the frame, entropy-coded data with no marker after it, other
sampling layouts, and files of other formats) is decoded by PIL on the host and uploaded, so every file ``load_image_bgr`` accepts is
accepted here, in the same output order, and a file PIL refuses raises ``HostDecodeError`` (a ``ValueError`` and an ``OSError``)
that names the file and carries PIL's message.  As in libjpeg-turbo, a scan that references Huffman table 0 or 1 without a DHT for it
uses the standard tables of the JPEG specification (Annex K.3).
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib

LANE_BITS = 128          # bits of entropy-coded data per lane of the self-synchronising decode (JPEG_LANE_BITS in csrc/jpeg.hip)
LOOKAHEAD = 9            # lookahead bits of the Huffman decode tables
_IMG = 64                # int32 columns per image (include/sceneego_hip.h)
_SEG = 8                 # int64 columns per segment
_TABLE_BYTES = 1536      # bytes per Huffman table record: uint16 lut[512], int32 maxcode[18], int32 valoff[18], uint8 vals[256]
_STATUS = {
    1: "descriptor out of range",
    2: "no code matches at bit {v}",
    3: "stream ended after {v} of {n} blocks",
    4: "block {v} of {n} is outside the plain-block domain of the IDCT",
}

# Annex K.3 tables (libjpeg-turbo's std_huff_tables): (bits[1..16], values)
_STD_HUFF = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], bytes(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], bytes(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a4344"
        "45464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4"
        "b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344"
        "45464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3"
        "b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
}

# zigzag index -> natural index (jpeg_natural_order, without the trailing guard entries)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int64)
_SOF_SEQ = (0xC0, 0xC1)
_SOF_OTHER = (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF)


def _name(src, i):
    return src if isinstance(src, str) else f"<bytes #{i}>"


class HostDecodeError(ValueError, OSError):
    """PIL refused a file the host decodes: both what this module raises for a bad file and what ``load_image_bgr`` raises."""


class HuffTable:
    """libjpeg's jpeg_make_d_derived_tbl, plus a LOOKAHEAD-bit table: ``lut[peek]`` = length << 8 | symbol (0: longer code)."""

    def __init__(self, bits, vals, is_dc, where):
        bits = [int(b) for b in bits]
        n = sum(bits)
        if n > 256 or n > len(vals):
            raise ValueError(f"{where}: {n} Huffman codes")
        self.bits, self.vals = bits, bytes(vals[:n])
        maxcode = np.full(18, -1, dtype=np.int64)
        valoff = np.zeros(18, dtype=np.int64)
        lut = np.zeros(1 << LOOKAHEAD, dtype=np.int64)
        code = p = 0
        for ln in range(1, 17):
            if bits[ln - 1]:
                valoff[ln] = p - code
                for _ in range(bits[ln - 1]):
                    if ln <= LOOKAHEAD:
                        lo = code << (LOOKAHEAD - ln)
                        lut[lo:lo + (1 << (LOOKAHEAD - ln))] = (ln << 8) | self.vals[p]
                    p += 1
                    code += 1
                maxcode[ln] = code - 1
            if code >= (1 << ln):
                raise ValueError(f"{where}: oversubscribed code-length table (length {ln})")
            code <<= 1
        maxcode[17] = 0xFFFFF
        if is_dc and any(v > 15 for v in self.vals):
            raise ValueError(f"{where}: DC symbol > 15")
        self.maxcode, self.valoff, self.lut = maxcode, valoff, lut

    def record(self):
        r = np.zeros(_TABLE_BYTES, dtype=np.uint8)
        r[:1024] = self.lut.astype("<u2").view(np.uint8)
        r[1024:1096] = self.maxcode.astype("<i4").view(np.uint8)
        r[1096:1168] = self.valoff.astype("<i4").view(np.uint8)
        r[1168:1168 + len(self.vals)] = np.frombuffer(self.vals, dtype=np.uint8)
        return r


class JpegFile:
    """Parsed markers of one file.  ``device`` tells whether the device path takes it (else ``why`` says why not); for a device
    file: ``W, H``, ``comps`` (frame order: id, h, v, quant id), ``scan`` (frame indices in scan order with DC / AC table ids),
    ``mcus_x, mcus_y``, ``blocks_per_mcu``, ``restart``, ``quant`` (natural order), ``huff`` and ``segments`` (first MCU, MCU
    count, unstuffed bytes)."""

    def __init__(self, src, index=0):
        self.name = _name(src, index)
        if isinstance(src, (bytes, bytearray, memoryview)):
            self.buf = bytes(src)
        else:
            with open(src, "rb") as f:
                self.buf = f.read()
        self.device, self.why = False, ""
        try:
            self._parse()
        except (struct.error, IndexError) as e:
            raise ValueError(f"{self.name}: truncated header ({e!r})") from None

    def _err(self, msg):
        raise ValueError(f"{self.name}: {msg}")

    def _fallback(self, why):
        self.device, self.why = False, why

    def _parse(self):
        buf = self.buf
        if buf[:2] != b"\xff\xd8":                   # not a JPEG (PNG, ...): PIL on the host, as load_image_bgr
            return self._fallback("no SOI marker")
        quant, huff = {}, {}
        self.restart = 0
        jfif = False
        adobe = None
        sof = None
        pos = 2
        while True:
            if pos + 4 > len(buf):
                self._err("truncated header (no SOS)")
            if buf[pos] != 0xFF:
                self._err(f"expected a marker at byte {pos}")
            while buf[pos + 1] == 0xFF:
                pos += 1
            m = buf[pos + 1]
            if m == 0xD9:
                self._err("EOI before SOS")
            if 0xD0 <= m <= 0xD7 or m == 0x01:
                pos += 2
                continue
            (seglen,) = struct.unpack_from(">H", buf, pos + 2)
            if seglen < 2 or pos + 2 + seglen > len(buf):
                self._err(f"truncated header (marker 0x{m:02X} of {seglen} bytes at byte {pos})")
            body = buf[pos + 4:pos + 2 + seglen]
            pos += 2 + seglen
            if m == 0xE0 and body[:5] == b"JFIF\0":
                jfif = True
            elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
                adobe = body[11]
            elif m == 0xDB:
                q = 0
                while q < len(body):
                    pq, tq = body[q] >> 4, body[q] & 15
                    n = 128 if pq else 64
                    if tq > 3 or pq > 1 or q + 1 + n > len(body):
                        self._err(f"bad DQT (table {tq}, precision {pq})")
                    zz = np.frombuffer(body, dtype=">u2" if pq else np.uint8, count=64, offset=q + 1).astype(np.int64)
                    nat = np.zeros(64, dtype=np.int64)
                    nat[ZIGZAG] = zz
                    quant[tq] = nat
                    q += 1 + n
            elif m == 0xC4:
                q = 0
                while q < len(body):
                    if q + 17 > len(body):
                        self._err("truncated DHT")
                    tc, th = body[q] >> 4, body[q] & 15
                    bits = list(body[q + 1:q + 17])
                    n = sum(bits)
                    if tc > 1 or th > 3 or q + 17 + n > len(body):
                        self._err(f"bad DHT (class {tc}, table {th})")
                    huff[(tc, th)] = (bits, body[q + 17:q + 17 + n])
                    q += 17 + n
            elif m == 0xDD:
                if len(body) < 2:
                    self._err("truncated DRI")
                (self.restart,) = struct.unpack_from(">H", body, 0)
            elif m in _SOF_SEQ or m in _SOF_OTHER:
                if sof is not None:
                    self._err("two SOF markers")
                sof = (m, body)
                if m in _SOF_OTHER:
                    return self._fallback(f"SOF 0x{m:02X}")
                if len(body) < 6:
                    self._err("truncated SOF")
                prec, H, W, nf = struct.unpack_from(">BHHB", body, 0)
                if len(body) < 6 + 3 * nf:
                    self._err("truncated SOF")
                if W == 0 or H == 0:
                    self._err(f"zero width or height ({W}x{H})")
                if prec != 8:
                    return self._fallback(f"{prec}-bit samples")
                self.W, self.H = W, H
                self.comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)]
            elif m == 0xDA:
                if sof is None:
                    self._err("SOS before SOF")
                self._sos(body, pos, quant, huff, jfif, adobe)
                return
            # other markers (APPn, COM, DNL, ...) are skipped

    def _sos(self, body, data_start, quant, huff, jfif, adobe):
        comps = self.comps
        nf = len(comps)
        if nf == 3:
            ids = [c[0] for c in comps]
            if jfif:
                rgb = False
            elif adobe is not None:
                rgb = adobe == 0
            else:
                rgb = ids == [82, 71, 66]
            if rgb:
                return self._fallback("RGB colour space")
            h0, v0 = comps[0][1], comps[0][2]
            if (h0, v0) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                return self._fallback(f"sampling {[(c[1], c[2]) for c in comps]}")
        elif nf != 1:
            return self._fallback(f"{nf} components")
        if any(c[1] < 1 or c[2] < 1 or c[1] > 4 or c[2] > 4 for c in comps):
            self._err(f"bad sampling factors {[(c[1], c[2]) for c in comps]}")
        if len(body) < 1:
            self._err("truncated SOS")
        ns = body[0]
        if len(body) < 4 + 2 * ns:
            self._err("truncated SOS")
        scan = []
        for i in range(ns):
            cid, t = body[1 + 2 * i], body[2 + 2 * i]
            idx = [k for k, c in enumerate(comps) if c[0] == cid]
            if not idx:
                self._err(f"scan component {cid} not in the frame")
            scan.append((idx[0], t >> 4, t & 15))
        ss, se, a = body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns]
        if ns != nf or len({s[0] for s in scan}) != nf:
            return self._fallback("multi-scan")
        if [s[0] for s in scan] != sorted(s[0] for s in scan):      # libjpeg takes the scan's components in frame order only
            return self._fallback("scan order differs from the frame's")
        if ss != 0 or se != 63 or a != 0:
            self._err(f"sequential scan with Ss={ss} Se={se} Ah/Al=0x{a:02X}")
        for fi, _, _ in scan:
            tq = comps[fi][3]
            if tq not in quant:
                self._err(f"quantisation table {tq} referenced but not defined")
        tables = {}
        for fi, td, ta in scan:
            for cls, t in ((0, td), (1, ta)):
                if (cls, t) in tables:
                    continue
                if t > 3:
                    self._err(f"Huffman table {t} out of range")
                if (cls, t) in huff:
                    bits, vals = huff[(cls, t)]
                elif t < 2:
                    bits, vals = _STD_HUFF[(cls, t)]
                else:
                    self._err(f"{'AC' if cls else 'DC'} Huffman table {t} referenced but not defined")
                tables[(cls, t)] = HuffTable(bits, vals, cls == 0, f"{self.name}: {'AC' if cls else 'DC'} Huffman table {t}")
        self.scan, self.huff = scan, tables
        self.quant = {fi: quant[comps[fi][3]] for fi, _, _ in scan}
        if nf == 1:
            self.hmax = self.vmax = 1
            self.mcus_x, self.mcus_y = -(-self.W // 8), -(-self.H // 8)
            self.block_comp = [0]
        else:
            self.hmax, self.vmax = max(c[1] for c in comps), max(c[2] for c in comps)
            self.mcus_x, self.mcus_y = -(-self.W // (8 * self.hmax)), -(-self.H // (8 * self.vmax))
            self.block_comp = [fi for fi, _, _ in scan for _ in range(comps[fi][1] * comps[fi][2])]
        self.blocks_per_mcu = len(self.block_comp)
        if self._segments(data_start):
            self.device = True

    def comp_hv(self, fi):
        return (1, 1) if len(self.comps) == 1 else (self.comps[fi][1], self.comps[fi][2])

    def _segments(self, start):
        buf = self.buf
        arr = np.frombuffer(buf, dtype=np.uint8)
        ff = np.flatnonzero(arr[start:len(buf) - 1] == 0xFF) + start
        nxt = arr[ff + 1]
        mk = ff[(nxt != 0x00) & (nxt != 0xFF)]
        kinds = arr[mk + 1]
        is_rst = (kinds >= 0xD0) & (kinds <= 0xD7)
        stop = np.flatnonzero(~is_rst)
        if not len(stop):                             # PIL calls such a file truncated, whether or not every block is there
            self._fallback("entropy-coded stream ended without a marker")
            return False
        end = int(mk[stop[0]])
        if kinds[stop[0]] == 0xDA:
            self._fallback("multi-scan")
            return False
        rst = mk[is_rst & (mk < end)]
        n_mcu = self.mcus_x * self.mcus_y
        if len(rst) and not self.restart:
            self._err("RST marker without a restart interval")
        expect = (kinds[is_rst & (mk < end)].astype(np.int64) - 0xD0)
        if len(rst) and not np.array_equal(expect, np.arange(len(rst)) % 8):
            bad = int(np.flatnonzero(expect != np.arange(len(rst)) % 8)[0])
            self._err(f"RST markers out of sequence (RST{int(expect[bad])} where RST{bad % 8} belongs, byte {int(rst[bad])})")
        per = self.restart if self.restart else n_mcu
        n_seg = -(-n_mcu // per)
        bounds = [start] + [int(r) + 2 for r in rst]
        ends = [int(r) for r in rst] + [end]
        if len(bounds) > n_seg:
            self._err(f"{len(bounds)} restart segments, more than the {n_seg} a restart interval of {per} MCUs implies")
        if len(bounds) < n_seg:
            self._err(f"entropy-coded data ends after {len(bounds)} of {n_seg} restart segments")
        self.segments = []
        for i, (a, b) in enumerate(zip(bounds, ends)):
            raw = buf[a:b].rstrip(b"\xff")
            self.segments.append((i * per, min(per, n_mcu - i * per), raw.replace(b"\xff\x00", b"\xff")))
        return True

    def host_decode(self):
        import io

        from PIL import Image
        with Image.open(io.BytesIO(self.buf)) as im:
            rgb = np.asarray(im.convert("RGB"))
        return np.ascontiguousarray(rgb[:, :, ::-1])


def parse(sources):
    """Parsed ``JpegFile`` of every source (paths or bytes), same size checked; raises ``ValueError`` naming the file."""
    files = []
    for i, s in enumerate(sources):
        f = s if isinstance(s, JpegFile) else JpegFile(s, i)
        files.append(f)
    shapes = {}
    for f in files:
        if f.device:
            shapes.setdefault((f.H, f.W), f.name)
        else:
            try:
                img = f.host_decode()
            except Exception as e:                    # PIL's UnidentifiedImageError, OSError, SyntaxError, ...
                raise HostDecodeError(f"{f.name}: {f.why}: {e}") from e
            f.host_image = img
            shapes.setdefault(img.shape[:2], f.name)
    if len(shapes) > 1:
        raise ValueError(f"decode_jpeg_batch: files of different sizes {sorted(shapes)} (e.g. {list(shapes.values())})")
    return files


class Packed:
    """Descriptors, tables and unstuffed segments of the device files of a batch, laid out for one pinned upload."""

    def __init__(self, files):
        dev = [(b, f) for b, f in enumerate(files) if f.device]
        self.dev = dev
        n_img = len(dev)
        n_seg = sum(len(f.segments) for _, f in dev)
        img = np.zeros((max(n_img, 1), _IMG), dtype=np.int32)
        seg = np.zeros((max(n_seg, 1), _SEG), dtype=np.int64)
        tables = np.zeros((max(n_img, 1) * 8, _TABLE_BYTES), dtype=np.uint8)
        quant = np.zeros((max(n_img, 1) * 4, 64), dtype=np.int32)
        seg_names = []
        data_len = 0
        r = 0
        for i, (b, f) in enumerate(dev):
            nf = len(f.comps)
            d = img[i]
            d[0:11] = [f.W, f.H, nf, f.mcus_x, f.mcus_y, f.blocks_per_mcu, r, len(f.segments), b, f.hmax, f.vmax]
            k0 = 0
            slot = {}
            for j, (fi, td, ta) in enumerate(f.scan):
                h, v = f.comp_hv(fi)
                d[12 + fi], d[15 + fi], d[18 + fi] = h, v, fi
                for cls, t in ((0, td), (1, ta)):
                    if (cls, t) not in slot:
                        slot[(cls, t)] = 4 * cls + t
                        tables[8 * i + 4 * cls + t] = f.huff[(cls, t)].record()
                d[21 + fi], d[24 + fi] = td, 4 + ta
                d[27 + fi], d[30 + fi] = 8 * h * f.mcus_x, 8 * v * f.mcus_y
                d[33 + fi] = k0
                k0 += h * v
                # libjpeg multiplies by the quantisation value cast to its 16-bit ISLOW_MULT_TYPE
                quant[4 * i + fi] = f.quant[fi].astype(np.uint16).view(np.int16).astype(np.int32)
            for k, fi in enumerate(f.block_comp):
                d[40 + k] = fi
            d[50] = f.restart
            for si, (m0, mc, data) in enumerate(f.segments):
                seg[r, 0:5] = [data_len, len(data), i, m0, mc]
                seg_names.append((f.name, si, mc * f.blocks_per_mcu, len(f.segments), b))
                data_len += ((len(data) + 3) & ~3) + 8
                r += 1
        self.img, self.seg, self.tables, self.quant = img, seg, tables, quant
        self.n_img, self.n_seg, self.seg_names, self.data_len = n_img, n_seg, seg_names, data_len

    def fill(self, host, base):
        """Writes descriptors, tables, quantisation and segment bytes into ``host`` (uint8) from ``base``; returns offsets."""
        offs = {}
        pos = base
        for key, arr in (("img", self.img), ("seg", self.seg), ("tables", self.tables), ("quant", self.quant)):
            raw = arr.view(np.uint8).reshape(-1)
            offs[key] = pos
            host[pos:pos + raw.size] = raw
            pos = (pos + raw.size + 15) & ~15
        offs["data"] = pos
        p = pos
        for _, f in self.dev:
            for _, _, data in f.segments:
                n = len(data)
                host[p:p + n] = np.frombuffer(data, dtype=np.uint8)
                pad = ((n + 3) & ~3) + 8
                host[p + n:p + pad] = 0
                p += pad
        offs["end"] = (p + 15) & ~15
        return offs

    def size(self):
        s = 0
        for arr in (self.img, self.seg, self.tables, self.quant):
            s = (s + arr.nbytes + 15) & ~15
        return (s + self.data_len + 15) & ~15


class DecodeStatus:
    """Per-segment status of a decode whose check was deferred (``check=False``): ``status`` is the device int32 [segments, 2]
    vector.  ``check()`` reads it back; every file with a non-zero status is decoded by PIL on the host and copied into its slot of
    the output (on the current stream), and ``redecoded`` lists those slots.  Where PIL refuses the file too, ``check()`` raises
    ``ValueError`` naming the file, its first bad segment and the status, chained from PIL's error; status 1 (a descriptor out of
    range, which no file can cause) raises at once."""

    def __init__(self, status, seg_names, files, out):
        self.status = status
        self._segs = seg_names                       # (file name, segment index, blocks, segments of the file, output slot)
        self._files, self._out = files, out
        self.redecoded = []

    def check(self):
        if self.status.numel() == 0:
            return
        st = self.status.cpu().numpy()
        done = set(self.redecoded)
        for i in np.nonzero(st[:, 0])[0]:
            i = int(i)
            name, si, n, ns, slot = self._segs[i]
            if slot in done:
                continue
            done.add(slot)
            msg = _STATUS.get(int(st[i, 0]), f"status {int(st[i, 0])}").format(v=int(st[i, 1]), n=n)
            where = f"restart segment {si}: " if ns > 1 else ""
            if int(st[i, 0]) == 1:                    # not the file's fault: the descriptors this module packed are wrong
                raise ValueError(f"{name}: {where}{msg}")
            try:
                img = self._files[slot].host_decode()
                if tuple(img.shape) != tuple(self._out.shape[1:]):
                    raise RuntimeError(f"PIL decodes it as {img.shape}")
            except Exception as e:
                raise ValueError(f"{name}: {where}{msg}") from e
            self._out[slot].copy_(torch.from_numpy(img))
            self.redecoded.append(slot)


def decode_jpeg_batch(sources, device, out=None, check=True, rounds=None):
    """JPEG files (paths, bytes or parsed ``JpegFile``) of one size -> uint8 [B, H, W, 3], B, G, R order, on ``device``.

    Bit-identical to ``preprocess.load_image_bgr``.  ``out``: a caller's contiguous uint8 [B, H, W, 3] tensor.  ``check``: read
    the per-segment status back, decode every file that reports one with PIL on the host into its slot, and raise ``ValueError``
    naming the file where PIL refuses it too; ``False`` returns ``(tensor, DecodeStatus)`` and leaves that to ``DecodeStatus.check()``.
    ``rounds``: inter-workgroup synchronisation launches (default: the library's); 0 sends every unsynchronised workgroup
    through the sequential repair kernel.  Everything runs on ``device``'s current stream."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HipExtensionError(f"decode_jpeg_batch needs a HIP device (got {device})")
    sources = list(sources)
    if not sources:
        raise ValueError("decode_jpeg_batch: no sources")
    files = parse(sources)
    f0 = files[0]
    H, W = (f0.H, f0.W) if f0.device else f0.host_image.shape[:2]
    B = len(files)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((B, H, W, 3), device=device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != (B, H, W, 3) or out.device != device:
        raise ValueError(f"out must be a contiguous uint8 [{B}, {H}, {W}, 3] tensor on {device}")
    pk = Packed(files)
    status = torch.zeros((pk.n_seg, 2), device=device, dtype=torch.int32)
    with torch.cuda.device(device):
        if pk.n_img:
            layout = np.zeros(8, dtype=np.int64)
            scratch_bytes = _lib.jpeg_scratch_bytes(pk.img[:pk.n_img], pk.seg[:pk.n_seg], layout)
            total = pk.size()
            pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            offs = pk.fill(pinned.numpy(), 0)
            dev = torch.empty(total, dtype=torch.uint8, device=device)
            dev.copy_(pinned, non_blocking=True)
            scratch = torch.empty(max(scratch_bytes, 16), dtype=torch.uint8, device=device)
            base = dev.data_ptr()
            _lib.jpeg_decode(base + offs["data"], offs["end"] - offs["data"], base + offs["img"], pk.n_img, base + offs["seg"],
                             pk.n_seg, base + offs["tables"], base + offs["quant"], layout, out, scratch, status,
                             -1 if rounds is None else int(rounds))
        for b, f in enumerate(files):
            if not f.device:
                out[b].copy_(torch.from_numpy(f.host_image))
    st = DecodeStatus(status, pk.seg_names, files, out)
    if not check:
        return out, st
    st.check()
    return out
