"""The seeded case list of the JPEG encoder tests (host and GPU), and per-case results computed once per session: the model's files
(tests/jpeg_encode_model.py) and PIL's.  Frames are uint8 [B,H,W,3] in R, G, B; a case with ``order == "bgr"`` hands the encoder the
same pixels with the channels flipped and expects the same file."""
from __future__ import annotations

import functools
import io
import os

import numpy as np

import jpeg_encode_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(8, 8), (9, 9), (1, 1), (13, 21), (16, 24), (17, 33), (136, 200)]


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(2 * x + y + seed) % 256, (x + 3 * y) // 2 % 256, 255 - (x + y) % 256], axis=-1).astype(np.uint8)


def patch(h, w, seed):
    """Flat white with a coloured patch: EOB-only blocks and zero DC differences around it."""
    img = np.full((h, w, 3), 255, dtype=np.uint8)
    img[h // 3:h // 3 + max(1, h // 4), w // 2:w // 2 + max(1, w // 5)] = (200, 30 + seed % 50, 90)
    return img


def checker(h, w, seed):
    """A 0 / 255 one-pixel checkerboard in the upper half, a checkerboard of 8x8 squares below: the largest AC and DC categories."""
    y, x = np.mgrid[0:h, 0:w]
    top = ((x + y + seed) & 1) * 255
    bottom = (((x >> 3) + (y >> 3) + seed) & 1) * 255
    g = np.where(y < (h + 1) // 2, top, bottom).astype(np.uint8)
    return np.stack([g, g, g], axis=-1)


def texel(h, w, seed):
    """Smooth, with one isolated high-frequency texel per block at its last row and column: long zero runs (ZRL) and a non-zero
    coefficient 63."""
    img = ramp(h, w, seed) // 4 + 96
    img[7::8, 7::8] = (255, 0, 255)
    img[6::8, 7::8] = (0, 255, 0)
    img[7::8, 6::8] = (0, 255, 0)
    return img.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _demo_rgb():
    from PIL import Image
    with Image.open(os.path.join(GOLD, "demo", "img_001000.jpg")) as im:
        return np.asarray(im.convert("RGB")).copy()


def crop(h, w, seed):
    full = _demo_rgb()
    y0, x0 = 400 + 7 * seed, 500 + 11 * seed
    return np.ascontiguousarray(full[y0:y0 + h, x0:x0 + w])


CONTENT = {"noise": noise, "ramp": ramp, "patch": patch, "checker": checker, "texel": texel, "crop": crop}


class Case:
    def __init__(self, name, shape, kinds, quality, subsampling, restart_rows=0, order="rgb", seed=0):
        self.name, self.shape, self.kinds = name, shape, kinds
        self.quality, self.subsampling, self.restart_rows, self.order, self.seed = quality, subsampling, restart_rows, order, seed

    @property
    def frames(self):
        """uint8 [B,H,W,3], R, G, B."""
        return _frames(self.name)

    def __repr__(self):
        return self.name


def _make_cases():
    cases = []

    def add(shape, kinds, q, sub, rr=0, order="rgb"):
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        name = f"{shape[0]}x{shape[1]}-{'+'.join(kinds)}-q{q}-{sub}-r{rr}-{order}"
        cases.append(Case(name, shape, kinds, q, sub, rr, order, seed=len(cases)))

    # every shape, both subsamplings, noise at a quality that keeps all 64 coefficients
    for i, shape in enumerate(SHAPES[:-1]):
        for sub in ("444", "420"):
            add(shape, "noise", (90, 100, 95, 75, 100, 50)[i], sub, rr=i & 1)
    # every content at a small and an odd shape, qualities and channel orders spread over them
    for i, kind in enumerate(CONTENT):
        q = (10, 50, 75, 90, 95, 100)[i]
        add((16, 24), kind, q, "444", order="bgr" if i & 1 else "rgb")
        add((17, 33), kind, (100, 95, 90, 75, 50, 10)[i], "420", rr=1, order="rgb" if i & 1 else "bgr")
    add((16, 24), "checker", 100, "444")
    add((17, 33), "texel", 100, "444", rr=1)
    # batches of three with different content per frame
    add((13, 21), ("noise", "patch", "texel"), 90, "444")
    add((17, 33), ("crop", "checker", "ramp"), 75, "420", rr=1)
    add((9, 9), ("noise", "checker", "noise"), 100, "420", order="bgr")
    # more blocks than one workgroup of the coding kernels takes (256), several chunks and restart intervals
    add((136, 200), "crop", 90, "444")
    add((136, 200), "noise", 100, "444", rr=1)
    add((136, 200), ("texel", "crop", "noise"), 50, "420", rr=1)
    add((136, 200), "noise", 95, "420", order="bgr")
    return cases


CASES = _make_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def _frames(name):
    c = BY_NAME[name]
    h, w = c.shape
    out = np.stack([CONTENT[k](h, w, c.seed + 17 * i) for i, k in enumerate(c.kinds)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_files(name):
    """(files of the case's frames, Stats over them) of the numpy model."""
    c = BY_NAME[name]
    st = M.Stats()
    return tuple(M.encode(f, c.quality, c.subsampling, c.restart_rows, st) for f in c.frames), st


@functools.lru_cache(maxsize=None)
def pil_files(name):
    """PIL's (libjpeg-turbo's) files of the case's frames: Annex K Huffman tables (optimize=False), same restart interval."""
    from PIL import Image
    c = BY_NAME[name]
    kw = {"restart_marker_rows": c.restart_rows} if c.restart_rows else {}
    out = []
    for f in c.frames:
        b = io.BytesIO()
        Image.fromarray(f).save(b, format="JPEG", quality=c.quality, subsampling=0 if c.subsampling == "444" else 2, optimize=False, **kw)
        out.append(b.getvalue())
    return tuple(out)


def pil_decode(data):
    """uint8 [H,W,3] R, G, B."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).copy()


# ------------------------------------------------------------------------------------------------------------------ RIFF walker
def walk_avi(data):
    """Checks the structure of an AVI ``sceneego_amd.jpeg_encode.MjpegWriter`` wrote and returns
    {"avih", "strh", "strf" (raw bytes), "frames": [(offset of the 00dc chunk, payload bytes)], "idx1": [(tag, flags, offset, size)],
    "movi": offset of the 'movi' tag}.  Sizes must nest and sum to the file size."""
    import struct
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    (riff,) = struct.unpack_from("<I", data, 4)
    assert riff + 8 == len(data), (riff, len(data))
    found = {"frames": [], "idx1": []}

    def chunks(lo, hi, depth):
        pos = lo
        while pos < hi:
            assert pos + 8 <= hi, f"chunk header at {pos} crosses its parent's end {hi}"
            tag = data[pos:pos + 4]
            (size,) = struct.unpack_from("<I", data, pos + 4)
            end = pos + 8 + size
            assert end <= hi, f"{tag!r} at {pos} ({size} bytes) crosses its parent's end {hi}"
            if tag == b"LIST":
                kind = data[pos + 8:pos + 12]
                if kind == b"movi":
                    found["movi"] = pos + 8
                chunks(pos + 12, end, depth + 1)
            elif tag == b"00dc":
                found["frames"].append((pos, size))
                if size & 1:
                    assert data[end] == 0, "an odd-length frame is followed by a pad byte"
            elif tag == b"idx1":
                assert size % 16 == 0
                found["idx1"] = [struct.unpack_from("<4sIII", data, pos + 8 + 16 * i) for i in range(size // 16)]
            else:
                assert tag in (b"avih", b"strh", b"strf"), tag
                found[tag.decode()] = data[pos + 8:end]
            pos = end + (size & 1)
        assert pos == hi, f"children end at {pos}, parent at {hi}"

    chunks(12, len(data), 0)
    return found


def check_avi(data, n_frames, width, height, fps):
    """The assertions of the AVI tests; returns the decoded frames' payloads."""
    import struct
    a = walk_avi(data)
    avih = struct.unpack("<14I", a["avih"])
    assert avih[4] == n_frames and avih[8] == width and avih[9] == height and avih[6] == 1
    assert avih[0] == round(1e6 / fps) and avih[3] & 0x10
    strh = struct.unpack("<4s4sIHHIIIIIIII4H", a["strh"])
    assert strh[0] == b"vids" and strh[1] == b"MJPG"
    assert strh[7] / strh[6] == fps and strh[9] == n_frames                      # dwRate / dwScale, dwLength
    strf = struct.unpack("<IiiHH4sIiiII", a["strf"])
    assert strf[0] == 40 and strf[1] == width and strf[2] == height and strf[5] == b"MJPG" and strf[4] == 24
    assert len(a["frames"]) == n_frames and len(a["idx1"]) == n_frames
    payloads = []
    for (tag, flags, off, size), (pos, fsize) in zip(a["idx1"], a["frames"]):
        assert tag == b"00dc" and flags & 0x10
        at = a["movi"] + off
        assert at == pos and data[at:at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == size == fsize
        payload = data[at + 8:at + 8 + size]
        img = pil_decode(payload)
        assert img.shape == (height, width, 3)
        payloads.append(payload)
    return payloads
