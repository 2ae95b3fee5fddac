"""Lossless PNG files from uint8 frames that live on a HIP device.

``PngEncoder.encode`` runs ``se_png_encode_u8`` (``csrc/png_enc.hip``: libpng's minimum-sum-of-absolute-differences row filter,
then one deflate block per 16 KiB of filtered rows, each parsed greedily over a few fixed distances and coded with its own
length-limited Huffman code, all segments in parallel) and reads back only the zlib stream of every frame; the host writes the
signature, ``IHDR``, one ``IDAT``, ``IEND`` and the chunk CRCs around it.  The bytes have one right answer, stated in DESIGN.md 4h2
and restated by ``tests/png_encode_model.py``; every PNG reader gets the input's pixels back.
"""
from __future__ import annotations

import struct
import zlib

import torch

from . import _lib

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)))


def png_file(height, width, channels, idat) -> bytes:
    """The file around one zlib stream: signature, IHDR (8 bits, colour type 2 for 3 channels or 0 for 1, no interlace), IDAT, IEND."""
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2 if channels == 3 else 0, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"")


class PngEncoder:
    """Encodes batches of uint8 [B,H,W,3] (RGB) or [B,H,W] (gray) device frames; the workspace and the output buffer of a shape are
    kept between calls."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipExtensionError(f"PngEncoder needs a HIP device, got {self.device}: the encoder has no CPU fallback")
        self._buffers = {}
        self.last_status = None          # int32 [B,2] on the host of the last encode

    @staticmethod
    def bound(height, width, channels=3) -> int:
        """Bytes no zlib stream of this shape exceeds (every segment stored, plus the joints): what the output buffer holds."""
        return _lib.png_encode_bound(height, width, channels)

    def _check_frames(self, frames):
        """What is wrong with the tensor itself is a ValueError wherever it lives; a well-formed tensor that is not on a HIP device is
        a HipExtensionError."""
        if not isinstance(frames, torch.Tensor):
            raise _lib.HipExtensionError(f"PngEncoder needs a tensor on a HIP device (got {type(frames).__name__}): the encoder has no "
                                         f"CPU fallback")
        self._check_layout(frames)
        if frames.device.type != "cuda":
            raise _lib.HipExtensionError(f"PngEncoder needs a tensor on a HIP device (got {frames.device}): the encoder has no CPU "
                                         f"fallback")
        return frames

    @staticmethod
    def _check_layout(frames):
        if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3) or 0 in frames.shape:
            raise ValueError(f"frames must be uint8 [B,H,W,3] or [B,H,W], got {frames.dtype} {tuple(frames.shape)}")
        if not frames.is_contiguous():
            raise ValueError("frames must be contiguous (call .contiguous() on a slice or a channel flip)")
        channels = 3 if frames.dim() == 4 else 1
        if frames.shape[1] * (1 + frames.shape[2] * channels) >= 2 ** 31:
            raise ValueError(f"a frame's filtered rows must stay below 2^31 bytes, got {frames.shape[1]}x{frames.shape[2]}")
        return frames

    def launch(self, frames):
        """One ``se_png_encode_u8`` call on the current stream, no synchronisation: (out uint8 [B,bound], length int32 [B], status
        int32 [B,2]) on the device.  ``frames``: uint8 [B,H,W,3] or [B,H,W] (an [H,W,3] tensor is a batch of gray frames: pass
        ``image[None]`` for one RGB image).  ``out`` is the encoder's buffer for this shape; the next call overwrites it."""
        frames = self._check_frames(frames)
        B, H, W = (int(v) for v in frames.shape[:3])
        channels = 3 if frames.dim() == 4 else 1
        dev = frames.device
        with torch.cuda.device(dev):
            key = (dev, B, H, W, channels)
            if key not in self._buffers:
                cap = (self.bound(H, W, channels) + 255) & ~255
                self._buffers[key] = (torch.empty(_lib.png_encode_scratch_bytes(B, H, W, channels), device=dev, dtype=torch.uint8),
                                      torch.empty((B, cap), device=dev, dtype=torch.uint8),
                                      torch.empty(B, device=dev, dtype=torch.int32), torch.empty((B, 2), device=dev, dtype=torch.int32))
            scratch, out, length, status = self._buffers[key]
            _lib.png_encode(frames, out, length, status, scratch)
        return out, length, status

    def encode(self, frames_u8) -> list:
        """Complete PNG files (``bytes``) of uint8 [B,H,W,3] or [B,H,W] frames on the device."""
        frames = self._check_frames(frames_u8)
        B, H, W = (int(v) for v in frames.shape[:3])
        out, _, status = self.launch(frames)
        st = status.cpu().numpy()
        if st[:, 0].any():
            raise _lib.HipExtensionError(f"se_png_encode_u8: status {st.tolist()}")
        self.last_status = st
        sizes = [int(n) for n in st[:, 1]]
        # only the compressed bytes cross to the host, in one copy
        packed = (out[0, :sizes[0]] if B == 1 else torch.cat([out[b, :sizes[b]] for b in range(B)])).cpu().numpy().tobytes()
        files, pos = [], 0
        for n in sizes:
            files.append(png_file(H, W, 3 if frames.dim() == 4 else 1, packed[pos:pos + n]))
            pos += n
        return files


_ENCODERS = {}


def default_png_encoder(device) -> PngEncoder:
    """One shared ``PngEncoder`` per device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _ENCODERS:
        _ENCODERS[device] = PngEncoder(device)
    return _ENCODERS[device]


def save_png_device(path, image, encoder=None) -> None:
    """uint8 [H,W,3] (R, G, B) or [H,W] (gray) -> a PNG file encoded on the device.  A tensor on a HIP device is encoded where it is;
    an array or a host tensor is uploaded to ``encoder``'s device (default: the current HIP device)."""
    t = torch.as_tensor(image)
    if t.device.type != "cuda":
        if not torch.cuda.is_available():
            raise _lib.HipExtensionError("save_png_device needs a HIP device: the encoder has no CPU fallback")
        t = t.to(encoder.device if encoder is not None else "cuda")
    if t.dim() not in (2, 3):
        raise ValueError(f"image must be [H,W,3] or [H,W], got {tuple(t.shape)}")
    enc = encoder if encoder is not None else default_png_encoder(t.device)
    (data,) = enc.encode(t.contiguous()[None])
    with open(path, "wb") as f:
        f.write(data)
