"""Batched OpenEXR depth decode on the device: the PIZ chunks of any number of files -> float32 [B, H, W] on a HIP device.

The host part parses the header (``exr._parse_header``), the offset table and each chunk's PIZ fields, picks the channel
``read_depth_exr`` picks (Y, B, Z, R, else the first name), validates every offset and size before anything is launched, packs the
descriptors and the file bytes into one pinned buffer, copies it to the device in one transfer on the current stream and launches
``se_exr_piz_decode_f32`` (``csrc/exr_piz.hip``: Huffman, wavelet, LUT, conversion, optional clamp and nearest resize).  The result
is bit-identical to ``exr.read_depth_exr`` (with ``out_hw`` / ``clamp``: to ``preprocess.prepare_depth(read_depth_exr(p))``, what
the reference's ``TestDataset.__getitem__`` computes).  Files that are not PIZ (NONE / ZIPS / ZIP) are decoded by ``exr.py`` on the
host and uploaded, so every file ``read_depth_exr`` accepts is accepted here.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib, exr
from .preprocess import DEPTH_CLAMP

_PIZ = 4
_PIZ_LINES = 32
_DESC = 16                  # int64 columns per chunk (include/sceneego_hip.h)
_CHAN = 8                   # int32 columns per file
_STATUS = {
    1: "descriptor out of range",
    2: "code-length table runs past the Huffman data",
    3: "code-length table larger than its scratch",
    4: "nBits runs past the Huffman data",
    5: "no code matches",
    6: "stream ended after {k} of {n} symbols",
    7: "run past end of output",
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
        self.piz = hdr["compression"] == _PIZ
        self.rows = []                                     # chunk descriptors (without file base / file index)
        if self.piz:
            self._parse_piz()

    def _parse_piz(self):
        hdr, buf, name = self.hdr, self.buf, self.name
        channels = hdr["channels"]
        if any(c[2] != 1 or c[3] != 1 for c in channels):
            raise NotImplementedError("sub-sampled EXR channels are not supported")
        if any(c[1] not in exr._PIXEL_SIZE for c in channels):
            raise ValueError(f"{name}: unknown pixel type in {channels}")
        sizes = [exr._PIXEL_SIZE[c[1]] // 2 for c in channels]
        k = _pick_channel(channels)
        self.chan = (self.W, self.H, channels[k][1], sum(sizes[:k]), sizes[k], sum(sizes), 0, 0)
        ymin, ymax = hdr["window"][1], hdr["window"][3]
        n_chunks = (self.H + _PIZ_LINES - 1) // _PIZ_LINES
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
            if y0 != ymin + i * _PIZ_LINES:
                raise ValueError(f"{where}: first row {y0}, expected {ymin + i * _PIZ_LINES}")
            ny = min(_PIZ_LINES, ymax - y0 + 1)
            row = [off + 8, size, 0, y0 - ymin, ny, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
            if size == bytes_per_line * ny:                 # stored uncompressed
                row[5] = 1
                self.rows.append(row)
                continue
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
            self.rows.append(row)

    def host_decode(self):
        return exr.depth_channel(exr.read_exr_buffer(self.buf))


class DecodeStatus:
    """The per-chunk status of a decode whose check was deferred (``check=False``): ``status`` is the device int32 [chunks, 2]
    vector, ``check()`` reads it back and raises ``ValueError`` naming the first bad file and chunk."""

    def __init__(self, status, chunks):
        self.status = status
        self._chunks = chunks                             # (file name, chunk index, words the decode needs)

    def check(self):
        if self.status.numel() == 0:
            return
        st = self.status.cpu().numpy()
        bad = np.nonzero(st[:, 0])[0]
        if len(bad):
            i = int(bad[0])
            name, ci, n = self._chunks[i]
            msg = _STATUS.get(int(st[i, 0]), f"status {int(st[i, 0])}").format(k=int(st[i, 1]), n=n)
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

    # descriptors and file bytes -> one pinned buffer: [chunk rows int64][file rows int32][file bytes, 16-byte aligned each]
    piz = [(b, f) for b, f in enumerate(files) if f.piz]
    n_chunks = sum(len(f.rows) for _, f in piz)
    chan = np.zeros((B, _CHAN), dtype=np.int32)
    desc = np.zeros((n_chunks, _DESC), dtype=np.int64)
    names = []
    head = ((n_chunks * _DESC * 8 + B * _CHAN * 4) + 15) & ~15
    pos, r = head, 0
    for b, f in piz:
        chan[b] = f.chan
        for ci, row in enumerate(f.rows):
            desc[r] = row
            desc[r, 0] += pos - head
            desc[r, 2] = b
            names.append((f.name, ci, (f.chan[3] + f.chan[4]) * f.W * row[4]))
            r += 1
        f.base = pos
        pos += (len(f.buf) + 15) & ~15
    status = torch.empty((n_chunks, 2), device=device, dtype=torch.int32)
    with torch.cuda.device(device):
        if n_chunks:
            scratch_bytes = _lib.exr_piz_scratch_bytes(desc, chan)
            pinned = torch.empty(pos, dtype=torch.uint8, pin_memory=True)
            host = pinned.numpy()
            host[:n_chunks * _DESC * 8] = desc.view(np.uint8).reshape(-1)
            host[n_chunks * _DESC * 8:n_chunks * _DESC * 8 + B * _CHAN * 4] = chan.view(np.uint8).reshape(-1)
            for _, f in piz:
                host[f.base:f.base + len(f.buf)] = np.frombuffer(f.buf, dtype=np.uint8)
            dev = torch.empty(pos, dtype=torch.uint8, device=device)
            dev.copy_(pinned, non_blocking=True)
            scratch = torch.empty(max(scratch_bytes, 16), dtype=torch.uint8, device=device)
            base = dev.data_ptr()
            _lib.exr_piz_decode(base + head, pos - head, base, n_chunks, base + n_chunks * _DESC * 8, B, out, clampv, scratch, status)
        for b, f in enumerate(files):
            if f.piz:
                continue
            d = f.host_decode()
            if d.shape != (oh, ow):
                ys = np.minimum(np.floor(np.arange(oh) * (d.shape[0] / oh)).astype(np.int64), d.shape[0] - 1)
                xs = np.minimum(np.floor(np.arange(ow) * (d.shape[1] / ow)).astype(np.int64), d.shape[1] - 1)
                d = d[ys][:, xs]
            d = np.array(d, dtype=np.float32, copy=True)
            if clampv > 0:
                d[d > clampv] = clampv
            out[b].copy_(torch.from_numpy(d))
    st = DecodeStatus(status, names)
    if not check:
        return out, st
    st.check()
    return out
