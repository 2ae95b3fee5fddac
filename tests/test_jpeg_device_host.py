"""Host side of the device JPEG decode (sceneego_amd/jpeg_device.py) and a numpy model of its integer stages (tests/jpeg_model.py):
parser fields, unstuffing, device / host classification, validation errors, the model bit for bit against PIL, and the
speculative / synchronisation rounds of the parallel Huffman decode against the sequential decode."""
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_model as M  # noqa: E402

from sceneego_amd.jpeg_device import JpegFile, parse  # noqa: E402


def _enc(arr, **kw):
    from PIL import Image, ImageFile
    b = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 26
    try:
        Image.fromarray(arr).save(b, "JPEG", **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return b.getvalue()


def _pil(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _img(kind, H, W, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "const":
        return np.full((H, W, 3), 201, dtype=np.uint8)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([(7 * xs + 3 * ys) % 256, (2 * xs + 5 * ys) % 256, (xs * ys) % 256], axis=-1).astype(np.uint8)


def _markers(data):
    """[(marker, position, segment length)] up to and including SOS."""
    out, pos = [], 2
    while True:
        m = data[pos + 1]
        (n,) = struct.unpack_from(">H", data, pos + 2)
        out.append((m, pos, n))
        if m == 0xDA:
            return out
        pos += 2 + n


def _find(data, marker):
    return next(p for m, p, _ in _markers(data) if m == marker)


# ------------------------------------------------------------------------------------------------------------------ parser
@pytest.mark.parametrize("sub,hv,bpm", [(0, (1, 1), 3), (1, (2, 1), 4), (2, (2, 2), 6)])
def test_parser_fields(sub, hv, bpm):
    d = _enc(_img("grad", 40, 49), quality=80, subsampling=sub, restart_marker_rows=1)
    f = JpegFile(d)
    assert f.device and (f.W, f.H) == (49, 40)
    assert [(c[1], c[2]) for c in f.comps] == [hv, (1, 1), (1, 1)]
    assert (f.mcus_x, f.mcus_y) == (-(-49 // (8 * hv[0])), -(-40 // (8 * hv[1])))
    assert f.blocks_per_mcu == bpm and f.block_comp == [0] * (hv[0] * hv[1]) + [1, 2]
    assert [(s[0], s[1], s[2]) for s in f.scan] == [(0, 0, 0), (1, 1, 1), (2, 1, 1)]
    assert f.restart == f.mcus_x
    assert [s[:2] for s in f.segments] == [(r * f.mcus_x, f.mcus_x) for r in range(f.mcus_y)]
    g = JpegFile(_enc(_img("grad", 17, 33)[:, :, 0].copy(), quality=60, restart_marker_blocks=4))
    assert g.device and len(g.comps) == 1 and (g.mcus_x, g.mcus_y, g.blocks_per_mcu) == (5, 3, 1)
    assert [s[:2] for s in g.segments] == [(0, 4), (4, 4), (8, 4), (12, 3)]


def test_unstuffing_matches_bytewise_reference():
    d = _enc(_img("noise", 64, 96, 3), quality=100, restart_marker_blocks=5)
    f = JpegFile(d)
    start = _find(d, 0xDA)
    start += 2 + struct.unpack_from(">H", d, start + 2)[0]
    segs, cur, i = [], bytearray(), start
    while True:                                  # plain byte-by-byte walk of the entropy-coded data
        b = d[i]
        if b == 0xFF:
            nx = d[i + 1]
            if nx == 0x00:
                cur.append(0xFF)
                i += 2
                continue
            if 0xD0 <= nx <= 0xD7:
                segs.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
            segs.append(bytes(cur))
            break
        cur.append(b)
        i += 1
    assert sum(s.count(b"\xff") for s in segs) > 50
    assert [s[2] for s in f.segments] == segs


# ------------------------------------------------------------------------------------------------------------------ classification
def _patch(data, pos, new):
    return data[:pos] + bytes(new) + data[pos + len(new):]


def test_classification():
    from PIL import Image
    arr = _img("grad", 24, 40)
    base = _enc(arr, quality=85)
    assert JpegFile(base).device
    for kw in ({"subsampling": 0}, {"subsampling": 1}, {"optimize": True}, {"restart_marker_blocks": 3}):
        assert JpegFile(_enc(arr, quality=85, **kw)).device
    assert JpegFile(_enc(arr[:, :, 0].copy(), quality=85)).device
    sof = _find(base, 0xC0)
    sof1 = _patch(base, sof + 1, [0xC1])                               # extended sequential: device, same pixels
    assert JpegFile(sof1).device and np.array_equal(M.decode(JpegFile(sof1)), _pil(sof1))
    # 16-bit quantisation tables with the same values: device
    dqt = _find(base, 0xDB)
    n = struct.unpack_from(">H", base, dqt + 2)[0]
    body, q, new = base[dqt + 4:dqt + 2 + n], 0, b""
    while q < len(body):
        new += bytes([0x10 | body[q] & 15]) + np.frombuffer(body, np.uint8, 64, q + 1).astype(">u2").tobytes()
        q += 65
    q16 = base[:dqt] + b"\xff\xdb" + struct.pack(">H", len(new) + 2) + new + base[dqt + 2 + n:]
    f16 = JpegFile(q16)
    assert f16.device and np.array_equal(M.decode(f16), _pil(q16)) and np.array_equal(_pil(q16), _pil(base))
    # no DHT: libjpeg-turbo's standard tables
    dht = [(p, ln) for m, p, ln in _markers(base) if m == 0xC4]
    nodht = base
    for p, ln in reversed(dht):
        nodht = nodht[:p] + nodht[p + 2 + ln:]
    fd = JpegFile(nodht)
    assert fd.device and np.array_equal(M.decode(fd), _pil(nodht))
    # host fall-backs
    assert not JpegFile(_enc(arr, quality=85, progressive=True)).device
    cmyk = io.BytesIO()
    Image.fromarray(arr).convert("CMYK").save(cmyk, "JPEG")
    assert not JpegFile(cmyk.getvalue()).device
    for marker in (0xC3, 0xC9, 0xC2):                                   # lossless, arithmetic, progressive
        assert not JpegFile(_patch(base, sof + 1, [marker])).device
    assert not JpegFile(_patch(base, sof + 4, [12])).device            # 12-bit samples
    assert not JpegFile(_patch(base, sof + 11, [0x12])).device         # luma 1x2: another sampling layout
    app0 = _find(base, 0xE0)
    n0 = struct.unpack_from(">H", base, app0 + 2)[0]
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"         # transform 0: RGB
    rgb = base[:app0] + adobe + base[app0 + 2 + n0:]
    assert not JpegFile(rgb).device
    png = io.BytesIO()
    Image.fromarray(arr).save(png, "PNG")
    f = JpegFile(png.getvalue())
    assert not f.device and np.array_equal(f.host_decode(), arr[:, :, ::-1])
    assert JpegFile(base[:app0] + adobe[:-1] + b"\x01" + base[app0 + 2 + n0:]).device     # transform 1: YCbCr


# ------------------------------------------------------------------------------------------------------------------ validation
def _raises(data, tmp_path, match):
    p = tmp_path / "bad.jpg"
    p.write_bytes(data)
    with pytest.raises(ValueError, match="bad.jpg: .*" + match):
        JpegFile(str(p))


def test_validation_errors(tmp_path):
    base = _enc(_img("grad", 24, 40), quality=85)
    sof = _find(base, 0xC0)
    sos = _find(base, 0xDA)
    _raises(base[:sof + 6], tmp_path, "truncated")
    _raises(_patch(base, sof + 9 + 3 * 1, [3]), tmp_path, "quantisation table 3 referenced but not defined")
    _raises(_patch(base, sos + 6 + 2, [0x22]), tmp_path, "Huffman table 2 referenced but not defined")
    dht = _find(base, 0xC4)
    _raises(_patch(base, dht + 5, [2, 1, 3]), tmp_path, "oversubscribed")     # two 1-bit codes, then more: same count
    _raises(_patch(base, sof + 5, [0, 0]), tmp_path, "zero width or height")
    _raises(_patch(base, sof + 7, [0, 0]), tmp_path, "zero width or height")
    rst = _enc(_img("grad", 24, 40), quality=85, restart_marker_blocks=1)
    first = rst.index(b"\xff\xd1")
    _raises(_patch(rst, first + 1, [0xD3]), tmp_path, "RST markers out of sequence")
    dri = _find(rst, 0xDD)
    _raises(_patch(rst, dri + 4, [0, 2]), tmp_path, "more than the")
    a, b = _enc(_img("grad", 24, 40), quality=85), _enc(_img("grad", 24, 48), quality=85)
    with pytest.raises(ValueError, match="different sizes"):
        parse([a, b])


# ------------------------------------------------------------------------------------------------------------------ model vs PIL
@pytest.mark.parametrize("sub", [0, 1, 2, "L"])
@pytest.mark.parametrize("hw", [(40, 48), (17, 33), (9, 17), (16, 16), (5, 3), (2, 2), (1, 1)])
def test_model_equals_pil(hw, sub):
    H, W = hw
    for i, kind in enumerate(("noise", "grad", "const")):
        arr = _img(kind, H, W, seed=i)
        kw = dict(quality=(100, 50, 5)[i], optimize=bool(i & 1), **({"restart_marker_blocks": 2} if i == 1 else {}))
        d = _enc(arr[:, :, 1].copy(), **kw) if sub == "L" else _enc(arr, subsampling=sub, **kw)
        f = JpegFile(d)
        assert f.device
        np.testing.assert_array_equal(M.decode(f), _pil(d))


@pytest.mark.parametrize("kind,rounds", [("noise", 0), ("noise", 1), ("grad", 2), ("const", 0)])
def test_sync_rounds_give_sequential_states(kind, rounds):
    d = _enc(_img(kind, 40, 48, 7), quality=90)
    f = JpegFile(d)
    _, _, data = f.segments[0]
    nblocks = f.mcus_x * f.mcus_y * f.blocks_per_mcu
    _, states = M.decode_segment(f, data, nblocks)
    bounds = sorted(states)
    S = 16 if kind == "const" else 64           # a constant image codes mostly EOBs: a few hundred bits
    entries, counts = M.sync_lanes(f, data, lane_bits=S, wg=4, rounds=rounds)
    assert len(entries) > 8
    for j, e in enumerate(entries):
        p = next((b for b in bounds if b >= S * j), None)
        if p is None or p == bounds[-1] and j > 0 and S * j > bounds[-1]:
            continue                             # a lane of padding bits only
        assert e[:3] == (p, *states[p]), (j, e, p, states[p])
    # the DC-code counts up to the last real block sum to the segment's blocks
    assert sum(counts) >= nblocks
