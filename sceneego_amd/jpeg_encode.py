"""Baseline JPEG files and Motion-JPEG AVIs from uint8 frames that live on a HIP device.

``JpegEncoder.encode`` runs ``se_jpeg_encode_u8`` (``csrc/jpeg_enc.hip``: libjpeg's integer colour conversion, 2x2 chroma average,
ISLOW forward DCT, quantiser and Huffman coding with the Annex K.3 tables, packed in parallel) and reads back only the compressed
scan of every frame; the host writes the markers around it (SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI when restart markers are
used, SOS, the scan, EOI).  The files equal, byte for byte in tables and scan, what libjpeg-turbo (``PIL.Image.save(format="JPEG",
quality=q, subsampling=0 or 2, optimize=False)``) writes for the same pixels.

``MjpegWriter`` puts such files into a plain RIFF AVI (``MJPG`` video stream, ``idx1`` index) that players open; below 2 GB.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib
from .jpeg_device import _STD_HUFF, ZIGZAG

# Annex K.1 / K.2 quantisation tables, natural order
_STD_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
             80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
             95, 98, 112, 100, 103, 99)
_STD_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
               99, 99) + (99,) * 32
_BLOCK_BYTES = 208           # worst case of one 8x8 block in the scan before stuffing (JE_BLOCK_BYTES of csrc/jpeg_enc.hip)
SUBSAMPLINGS = ("444", "420")


def quant_tables(quality):
    """(luma, chroma) uint16 [64] in natural order: libjpeg's ``jpeg_quality_scaling`` and ``jpeg_add_quant_table`` with
    ``force_baseline`` on the Annex K tables; ``quality`` 1..100."""
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"quality must be an integer in 1..100, got {quality!r}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(t, dtype=np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16) for t in (_STD_LUMA, _STD_CHROMA))


def mcu_grid(height, width, subsampling):
    """(MCUs per row, MCU rows, blocks per MCU)."""
    mcu = 16 if subsampling == "420" else 8
    return -(-width // mcu), -(-height // mcu), 6 if subsampling == "420" else 3


def file_header(height, width, quant_luma, quant_chroma, subsampling, restart_mcus=0) -> bytes:
    """SOI up to and including the SOS header."""
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for i, q in enumerate((quant_luma, quant_chroma)):
        out += b"\xff\xdb" + struct.pack(">HB", 67, i) + bytes(int(v) for v in np.asarray(q).reshape(64)[ZIGZAG])
    luma_hv = 0x22 if subsampling == "420" else 0x11
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, height, width, 3) + bytes([1, luma_hv, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls, t in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = _STD_HUFF[(cls, t)]
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), (cls << 4) | t) + bytes(bits) + bytes(vals)
    if restart_mcus:
        out += b"\xff\xdd" + struct.pack(">HH", 4, restart_mcus)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return bytes(out)


class JpegEncoder:
    """Encodes batches of uint8 [B,H,W,3] device frames; the workspace and the output buffer of a shape are kept between calls."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipExtensionError(f"JpegEncoder needs a HIP device, got {self.device}: the encoder has no CPU fallback")
        self._scratch = {}
        self._out = {}
        self.last_status = None          # int32 [B,2] on the host of the last launch (a retried call: of the retry)
        self.retries = 0                 # launches repeated with the worst-case capacity

    @staticmethod
    def worst_case_bytes(height, width, subsampling="444", restart_rows=0) -> int:
        """A capacity no scan of this shape can exceed: every block at its longest code, every byte stuffed, plus the markers."""
        mx, my, bpm = mcu_grid(height, width, subsampling)
        return 2 * _BLOCK_BYTES * mx * my * bpm + 2 * my

    def _check_frames(self, frames):
        if not isinstance(frames, torch.Tensor) or frames.device.type != "cuda":
            where = frames.device if isinstance(frames, torch.Tensor) else type(frames).__name__
            raise _lib.HipExtensionError(f"JpegEncoder.encode needs a tensor on a HIP device (got {where}): the encoder has no CPU fallback")
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or 0 in frames.shape:
            raise ValueError(f"frames must be uint8 [B,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
        if not frames.is_contiguous():
            raise ValueError("frames must be contiguous (call .contiguous() on a slice or a channel flip)")
        if frames.shape[1] > 65535 or frames.shape[2] > 65535:
            raise ValueError(f"a JPEG frame is at most 65535 x 65535, got {frames.shape[1]}x{frames.shape[2]}")
        return frames

    def launch(self, frames, quant_luma, quant_chroma, subsampling="444", restart_rows=0, order="rgb", capacity=None):
        """One ``se_jpeg_encode_u8`` call on the current stream, no synchronisation: (out uint8 [B,capacity], length int32 [B],
        status int32 [B,2]) on the device.  ``out`` is the encoder's buffer for this shape; the next call overwrites it."""
        frames = self._check_frames(frames)
        if subsampling not in SUBSAMPLINGS:
            raise ValueError(f"subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
        if order not in ("rgb", "bgr"):
            raise ValueError(f"order must be 'rgb' or 'bgr', got {order!r}")
        B, H, W = (int(v) for v in frames.shape[:3])
        mx = mcu_grid(H, W, subsampling)[0]
        restart_rows = int(restart_rows)
        if restart_rows < 0 or restart_rows * mx > 65535:
            raise ValueError(f"restart_rows must be >= 0 and span at most 65535 MCUs ({mx} per row), got {restart_rows}")
        cap = 3 * H * W if capacity is None else int(capacity)
        if cap < 1:
            raise ValueError(f"capacity must be >= 1, got {cap}")
        dev = frames.device
        with torch.cuda.device(dev):
            key = (dev, B, H, W, subsampling)
            if key not in self._scratch:
                n = _lib.jpeg_encode_scratch_bytes(B, H, W, int(subsampling))
                self._scratch[key] = (torch.empty(n, device=dev, dtype=torch.uint8), torch.empty(B, device=dev, dtype=torch.int32),
                                      torch.empty((B, 2), device=dev, dtype=torch.int32))
            scratch, length, status = self._scratch[key]
            okey = (dev, B, cap)
            if okey not in self._out:
                self._out = {k: v for k, v in self._out.items() if k[:2] != (dev, B)}     # one output buffer per batch size
                self._out[okey] = torch.empty((B, cap), device=dev, dtype=torch.uint8)
            out = self._out[okey]
            _lib.jpeg_encode(frames, quant_luma, quant_chroma, subsampling, restart_rows, out, length, status, scratch,
                             bgr=order == "bgr")
        return out, length, status

    def encode(self, frames_u8, quality=90, subsampling="444", restart_rows=0, order="rgb", capacity=None) -> list:
        """Complete JPEG files (``bytes``) of uint8 [B,H,W,3] (or [H,W,3]) frames on the device; ``order``: the channel order of
        the input.  ``capacity``: bytes of scan per frame to provide (default 3 H W); a frame that needs more makes the call run
        once more with the worst-case bound."""
        frames = self._check_frames(frames_u8)
        ql, qc = quant_tables(quality)
        B, H, W = (int(v) for v in frames.shape[:3])
        out, length, status = self.launch(frames, ql, qc, subsampling, restart_rows, order, capacity)
        st = status.cpu().numpy()
        if st[:, 0].any():
            self.retries += 1
            out, length, status = self.launch(frames, ql, qc, subsampling, restart_rows, order,
                                              self.worst_case_bytes(H, W, subsampling, restart_rows))
            st = status.cpu().numpy()
            if st[:, 0].any():
                raise _lib.HipExtensionError(f"se_jpeg_encode_u8: status {st.tolist()} with the worst-case capacity")
        self.last_status = st
        sizes = [int(n) for n in st[:, 1]]
        # only the compressed bytes cross to the host, in one copy
        packed = (out[0, :sizes[0]] if B == 1 else torch.cat([out[b, :sizes[b]] for b in range(B)])).cpu().numpy().tobytes()
        mx = mcu_grid(H, W, subsampling)[0]
        rows = int(restart_rows)
        head = file_header(H, W, ql, qc, subsampling, rows * mx)
        files, pos = [], 0
        for n in sizes:
            files.append(head + packed[pos:pos + n] + b"\xff\xd9")
            pos += n
        return files


_ENCODERS = {}


def default_encoder(device) -> JpegEncoder:
    """One shared ``JpegEncoder`` per device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _ENCODERS:
        _ENCODERS[device] = JpegEncoder(device)
    return _ENCODERS[device]


def save_jpeg(path, rgb, quality=90, subsampling="444", encoder=None) -> None:
    """uint8 [H,W,3] (R, G, B) -> a JPEG file encoded on the device.  A tensor on a HIP device is encoded where it is; an array or
    a host tensor is uploaded to ``encoder``'s device (default: the current HIP device)."""
    t = torch.as_tensor(rgb)
    if t.device.type != "cuda":
        if not torch.cuda.is_available():
            raise _lib.HipExtensionError("save_jpeg needs a HIP device: the encoder has no CPU fallback")
        t = t.to(encoder.device if encoder is not None else "cuda")
    enc = encoder if encoder is not None else default_encoder(t.device)
    (data,) = enc.encode(t.contiguous(), quality=quality, subsampling=subsampling)
    with open(path, "wb") as f:
        f.write(data)


# ------------------------------------------------------------------------------------------------------------------------- AVI
AVI_MAX_BYTES = 0x7FFFFFFF - 0x10000      # a plain RIFF AVI (no OpenDML index): 32-bit sizes, kept below 2 GB
_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10


def _rate_scale(fps):
    fps = float(fps)
    if not fps > 0 or fps != fps or fps > 1e6:
        raise ValueError(f"fps must be positive, got {fps}")
    if fps == int(fps):
        return int(fps), 1
    return int(round(fps * 1000)), 1000


class MjpegWriter:
    """A Motion-JPEG AVI: ``write(jpeg_bytes)`` per frame, ``close()`` (or the end of a ``with`` block) writes the index and patches
    the sizes and the frame count."""

    def __init__(self, path, width, height, fps=25):
        self.width, self.height = int(width), int(height)
        if not (0 < self.width <= 65535 and 0 < self.height <= 65535):
            raise ValueError(f"bad frame size {width}x{height}")
        self.rate, self.scale = _rate_scale(fps)
        self.path = path
        self.index = []                     # (offset from the 'movi' tag, bytes) per frame
        self.max_frame = 0
        self.closed = False
        self.f = open(path, "wb")
        self.f.write(self._headers(0, 0))
        self.movi_tag = self.f.tell() - 4   # position of the 'movi' fourcc
        self.pos = self.f.tell()

    def _headers(self, frames, movi_bytes):
        w, h = self.width, self.height
        usec = int(round(1e6 * self.scale / self.rate))
        per_sec = int(min(0xFFFFFFFF, self.max_frame * self.rate / self.scale))
        avih = struct.pack("<14I", usec, per_sec, 0, _AVIF_HASINDEX, frames, 0, 1, self.max_frame, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, frames, self.max_frame,
                           0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        riff = len(head) + movi_bytes + 8 + 16 * frames
        return b"RIFF" + struct.pack("<I", riff) + head

    def write(self, jpeg_bytes) -> None:
        if self.closed:
            raise ValueError(f"{self.path}: write after close")
        data = bytes(jpeg_bytes)
        if data[:2] != b"\xff\xd8" or data[-2:] != b"\xff\xd9":
            raise ValueError(f"{self.path}: frame {len(self.index)} is not a JPEG file (no SOI / EOI)")
        pad = len(data) & 1
        if self.pos + 8 + len(data) + pad + 8 + 16 * (len(self.index) + 1) > AVI_MAX_BYTES:
            raise ValueError(f"{self.path}: frame {len(self.index)} would take the file past the 2 GB a plain AVI holds "
                             f"(OpenDML is not written); start a new file or lower the quality")
        self.index.append((self.pos - self.movi_tag, len(data)))
        self.f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * pad)
        self.pos += 8 + len(data) + pad
        self.max_frame = max(self.max_frame, len(data))

    def close(self) -> None:
        if self.closed:
            return
        self.closed = True
        n = len(self.index)
        idx = b"".join(struct.pack("<4sIII", b"00dc", _AVIIF_KEYFRAME, off, size) for off, size in self.index)
        self.f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        self.f.seek(0)
        self.f.write(self._headers(n, self.pos - self.movi_tag - 4))
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
