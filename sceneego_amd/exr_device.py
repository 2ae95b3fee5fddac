"""Batched OpenEXR depth decode on the device: the chunks of any number of scanline files (PIZ, ZIP, ZIPS, NONE, mixed) -> float32
[B, H, W] on a HIP device.

The host part parses the header (``exr._parse_header``), the offset table and each chunk's fields (PIZ: bitmap range and Huffman
header; ZIP / ZIPS: the 2-byte zlib header), picks the channel ``read_depth_exr`` picks (Y, B, Z, R, else the first name),
validates every offset and size before anything is launched, packs the descriptors and the file bytes of the whole batch into one
pinned buffer, copies it to the device in one transfer on the current stream and launches ``se_exr_piz_decode_f32``
(``csrc/exr_piz.hip``: Huffman, wavelet, LUT) for the PIZ chunks and ``se_exr_zip_decode_f32`` (``csrc/exr_zip.hip``: inflate,
predictor, de-interleave) for the ZIP / ZIPS / NONE chunks, both with the same conversion, optional clamp and nearest resize.  The
result is bit-identical to ``exr.read_depth_exr`` (with ``out_hw`` / ``clamp``: to ``preprocess.prepare_depth(read_depth_exr(p))``,
what the reference's ``TestDataset.__getitem__`` computes); no file is decoded on the host.  One difference: a zlib stream that
inflates to more or fewer bytes than its chunk's scanlines is reported as a bad chunk, where ``exr.py`` would read the misplaced
bytes.  Files ``exr.py`` cannot read raise what it raises (RLE chunks that are not stored, B44 / DWA, tiled, multi-part,
sub-sampled).
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib, exr
from .preprocess import DEPTH_CLAMP

_NONE, _RLE, _PIZ = 0, 1, 4
_DESC = 16                  # int64 columns per chunk (include/sceneego_hip.h)
_CHAN = 8                   # int32 columns per file
_STATUS = {                 # PIZ codes 1-7 (csrc/exr_piz.hip), ZIP codes 8-16 (csrc/exr_zip.hip); {k}: the status value
    1: "descriptor out of range",
    2: "code-length table runs past the Huffman data",
    3: "code-length table larger than its scratch",
    4: "nBits runs past the Huffman data",
    5: "no code matches",
    6: "stream ended after {k} of {n} symbols",
    7: "run past end of output",
    8: "bad zlib header",
    9: "deflate block type 3",
    10: "stored block LEN does not match NLEN",
    11: "bad Huffman code-length set",
    12: "invalid deflate symbol or code-length repeat",
    13: "distance too far back",
    14: "zlib stream ended before its final block and Adler-32 ({k} of {n} bytes)",
    15: "zlib stream does not inflate to the chunk's {n} bytes",
    16: "Adler-32 mismatch",
}


def _name(src, i):
    return src if isinstance(src, str) else f"<bytes #{i}>"


def _pick_channel(channels):
    names = [c[0] for c in channels]
    for pref in ("Y", "B", "Z", "R"):
        if pref in names:
            return names.index(pref)
    return names.index(sorted(names)[0])


class _File:
    """Parsed and validated header / offset table / chunk fields of one file."""

    def __init__(self, src, index):
        self.name = _name(src, index)
        if isinstance(src, (bytes, bytearray, memoryview)):
            self.buf = bytes(src)
        else:
            with open(src, "rb") as f:
                self.buf = f.read()
        try:
            hdr = exr._parse_header(self.buf)
        except (struct.error, IndexError, KeyError, UnicodeDecodeError) as e:
            raise ValueError(f"{self.name}: malformed OpenEXR header ({e!r})") from None
        xmin, ymin, xmax, ymax = hdr["window"]
        self.W, self.H = xmax - xmin + 1, ymax - ymin + 1
        if self.W <= 0 or self.H <= 0:
            raise ValueError(f"{self.name}: empty data window {hdr['window']}")
        self.hdr = hdr
        comp = hdr["compression"]
        if comp not in exr._LINES_PER_CHUNK:                # what exr.read_exr_buffer raises
            raise NotImplementedError(f"EXR compression {comp} is not supported (NONE, ZIPS, ZIP, PIZ are)")
        self.piz = comp == _PIZ
        self.rows = []                                     # chunk descriptors (without file base / file index)
        self._parse(comp)

    def _parse(self, comp):
        hdr, buf, name = self.hdr, self.buf, self.name
        channels = hdr["channels"]
        if any(c[2] != 1 or c[3] != 1 for c in channels):
            raise NotImplementedError("sub-sampled EXR channels are not supported")
        if any(c[1] not in exr._PIXEL_SIZE for c in channels):
            raise ValueError(f"{name}: unknown pixel type in {channels}")
        sizes = [exr._PIXEL_SIZE[c[1]] // 2 for c in channels]
        k = _pick_channel(channels)
        self.chan = (self.W, self.H, channels[k][1], sum(sizes[:k]), sizes[k], sum(sizes), 0, 0)
        lines = exr._LINES_PER_CHUNK[comp]
        ymin, ymax = hdr["window"][1], hdr["window"][3]
        n_chunks = (self.H + lines - 1) // lines
        table_end = hdr["data_start"] + 8 * n_chunks
        if table_end > len(buf):
            raise ValueError(f"{name}: offset table of {n_chunks} chunks runs past the end of the file ({len(buf)} bytes)")
        offsets = np.frombuffer(buf, dtype="<u8", count=n_chunks, offset=hdr["data_start"]).tolist()
        bytes_per_line = 2 * sum(sizes) * self.W
        for i, off in enumerate(offsets):
            where = f"{name}: chunk {i}"
            if off < table_end or off + 8 > len(buf):
                raise ValueError(f"{where}: offset {off} outside the file's chunk data [{table_end}, {len(buf)})")
            y0, size = struct.unpack_from("<ii", buf, off)
            if size < 0 or off + 8 + size > len(buf):
                raise ValueError(f"{where}: {size} bytes at offset {off} run past the end of the file ({len(buf)} bytes)")
            if y0 != ymin + i * lines:
                raise ValueError(f"{where}: first row {y0}, expected {ymin + i * lines}")
            ny = min(lines, ymax - y0 + 1)
            row = [off + 8, size, 0, y0 - ymin, ny, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
            if size == bytes_per_line * ny or comp == _NONE:  # stored uncompressed
                if size < bytes_per_line * ny:
                    raise ValueError(f"{where}: {size} bytes hold less than its {bytes_per_line * ny} bytes of scanlines")
                row[5] = 1
            elif comp == _RLE:
                raise NotImplementedError("RLE")
            elif comp == _PIZ:
                self._piz_fields(row, where)
            else:                                          # ZIPS / ZIP: one zlib stream; its deflate data is checked on the device
                if size < 2:
                    raise ValueError(f"{where}: {size} bytes cannot hold a zlib stream")
                cmf, flg = buf[off + 8], buf[off + 9]
                if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or flg & 32:
                    raise ValueError(f"{where}: bad zlib header {cmf:02x} {flg:02x} (CM 8, CINFO <= 7, FCHECK, no FDICT)")
            self.rows.append(row)

    def _piz_fields(self, row, where):
        buf, off, size = self.buf, row[0] - 8, row[1]
        if size < 8:
            raise ValueError(f"{where}: {size} bytes cannot hold a PIZ block")
        min_nz, max_nz = struct.unpack_from("<HH", buf, off + 8)
        p = 4
        if min_nz <= max_nz:
            if max_nz >= exr.BITMAP_SIZE:
                raise ValueError(f"{where}: bitmap range [{min_nz}, {max_nz}] past {exr.BITMAP_SIZE} bytes")
            p += max_nz - min_nz + 1
        if p + 4 > size:
            raise ValueError(f"{where}: bitmap runs past the chunk's {size} bytes")
        (length,) = struct.unpack_from("<i", buf, off + 8 + p)
        p += 4
        if length < 0 or p + length > size:
            raise ValueError(f"{where}: Huffman data of {length} bytes runs past the chunk's {size} bytes")
        im = iM = nbits = 0
        if length > 0:
            if length < 20:
                raise ValueError(f"{where}: Huffman data of {length} bytes is shorter than its 20-byte header")
            im, iM, _table_len, nbits = struct.unpack_from("<IIII", buf, off + 8 + p)
            if not im <= iM <= exr.HUF_ENCSIZE - 1:
                raise ValueError(f"{where}: symbol range im={im} iM={iM} outside [0, {exr.HUF_ENCSIZE - 1}]")
            if nbits > 8 * (length - 20):
                raise ValueError(f"{where}: nBits {nbits} exceeds the {length - 20} bytes of table and bitstream")
        row[6:13] = [min_nz, max_nz, p, length, im, iM, nbits]


class DecodeStatus:
    """The per-chunk status of a decode whose check was deferred (``check=False``): ``status`` is the device int32 [chunks, 2]
    vector (the PIZ chunks of the batch first, then the ZIP / ZIPS / NONE chunks, each in file order), ``bad()`` lists the bad
    chunks and ``check()`` raises ``ValueError`` naming the first bad file and chunk."""

    def __init__(self, status, chunks):
        self.status = status
        self._chunks = chunks                             # (file name, chunk index, words / bytes the decode needs)

    def bad(self):
        """[(file name, chunk index, status code, message)] of every bad chunk, in status-vector order (reads the status back)."""
        if self.status.numel() == 0:
            return []
        st = self.status.cpu().numpy()
        out = []
        for i in np.nonzero(st[:, 0])[0].tolist():
            name, ci, n = self._chunks[i]
            code = int(st[i, 0])
            out.append((name, ci, code, _STATUS.get(code, f"status {code}").format(k=int(st[i, 1]), n=n)))
        return out

    def check(self):
        bad = self.bad()
        if bad:
            name, ci, _, msg = bad[0]
            raise ValueError(f"{name}: chunk {ci}: {msg}")


def decode_depth_exr_batch(sources, device, out=None, out_hw=None, clamp=DEPTH_CLAMP, check=True):
    """Depth maps of ``sources`` (paths or file bytes) -> float32 [B, H, W] on ``device`` (the channel ``read_depth_exr`` picks).

    out_hw: (H_out, W_out) nearest resize with ``prepare_depth``'s index rule; required when the files differ in size.
    clamp:  values above it are set to it (NaN kept), ``None`` or 0 for none.  ``out``: a caller's float32 [B, H_out, W_out] tensor.
    check:  read the per-chunk status back and raise ``ValueError`` on a malformed chunk; ``False`` returns ``(tensor, DecodeStatus)``.
    Everything runs on ``device``'s current stream."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HipExtensionError(f"decode_depth_exr_batch needs a HIP device (got {device})")
    files = [_File(s, i) for i, s in enumerate(sources)]
    if not files:
        raise ValueError("decode_depth_exr_batch: no sources")
    if out_hw is None:
        shapes = {(f.H, f.W) for f in files}
        if len(shapes) != 1:
            raise ValueError(f"decode_depth_exr_batch: files of different sizes {sorted(shapes)} need a common out_hw")
        out_hw = shapes.pop()
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if oh <= 0 or ow <= 0:
        raise ValueError(f"decode_depth_exr_batch: bad out_hw {out_hw}")
    clampv = float(clamp) if clamp else 0.0
    B = len(files)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if out is None:
        out = torch.empty((B, oh, ow), device=device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, oh, ow) or out.device != device:
        raise ValueError(f"out must be a contiguous float32 [{B}, {oh}, {ow}] tensor on {device}")

    # descriptors and file bytes -> one pinned buffer:
    # [PIZ chunk rows int64][ZIP / ZIPS / NONE chunk rows int64][file rows int32][file bytes, 16-byte aligned each]
    n_piz = sum(len(f.rows) for f in files if f.piz)
    n_zip = sum(len(f.rows) for f in files if not f.piz)
    n_chunks = n_piz + n_zip
    chan = np.array([f.chan for f in files], dtype=np.int32).reshape(B, _CHAN)
    desc = np.zeros((n_chunks, _DESC), dtype=np.int64)
    names = [None] * n_chunks
    head = ((n_chunks * _DESC * 8 + B * _CHAN * 4) + 15) & ~15
    pos, r_piz, r_zip = head, 0, n_piz
    for b, f in enumerate(files):
        for ci, row in enumerate(f.rows):
            if f.piz:
                r, need = r_piz, (f.chan[3] + f.chan[4]) * f.W * row[4]        # words decoded up to the end of the plane
                r_piz += 1
            else:
                r, need = r_zip, 2 * f.chan[5] * f.W * row[4]                   # bytes of scanlines
                r_zip += 1
            desc[r] = row
            desc[r, 0] += pos - head
            desc[r, 2] = b
            names[r] = (f.name, ci, need)
        f.base = pos
        pos += (len(f.buf) + 15) & ~15
    status = torch.empty((n_chunks, 2), device=device, dtype=torch.int32)
    with torch.cuda.device(device):
        if n_chunks:
            desc_piz, desc_zip = desc[:n_piz], desc[n_piz:]     # views: the scratch layouts are written into desc
            piz_scratch = _lib.exr_piz_scratch_bytes(desc_piz, chan) if n_piz else 0
            zip_scratch = _lib.exr_zip_scratch_bytes(desc_zip, chan) if n_zip else 0
            pinned = torch.empty(pos, dtype=torch.uint8, pin_memory=True)
            host = pinned.numpy()
            host[:n_chunks * _DESC * 8] = desc.view(np.uint8).reshape(-1)
            host[n_chunks * _DESC * 8:n_chunks * _DESC * 8 + B * _CHAN * 4] = chan.view(np.uint8).reshape(-1)
            for f in files:
                host[f.base:f.base + len(f.buf)] = np.frombuffer(f.buf, dtype=np.uint8)
            dev = torch.empty(pos, dtype=torch.uint8, device=device)
            dev.copy_(pinned, non_blocking=True)
            base = dev.data_ptr()
            chan_ptr = base + n_chunks * _DESC * 8
            if n_piz:
                scratch_piz = torch.empty(max(piz_scratch, 16), dtype=torch.uint8, device=device)
                _lib.exr_piz_decode(base + head, pos - head, base, n_piz, chan_ptr, B, out, clampv, scratch_piz, status[:n_piz])
            if n_zip:
                scratch_zip = torch.empty(max(zip_scratch, 16), dtype=torch.uint8, device=device)
                _lib.exr_zip_decode(base + head, pos - head, base + n_piz * _DESC * 8, n_zip, chan_ptr, B, out, clampv, scratch_zip,
                                    status[n_piz:])
    st = DecodeStatus(status, names)
    if not check:
        return out, st
    st.check()
    return out
