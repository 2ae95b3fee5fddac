"""GPU: the ZIP / ZIPS / NONE decode on the device (se_exr_zip_inflate_kernel / se_exr_zip_recon_kernel) is bit-identical to exr.py on
every test-side case and on the demo maps re-encoded, with and without prepare_depth's clamp and resize, alone and in batches mixed
with PIZ; no file is decoded on the host; every bad stream is reported with its file, chunk and reason and leaves its rows of `out`
untouched; single-byte corruptions are accepted exactly where zlib accepts them; the forward and run_sequence.py give the same
results on device- and host-decoded ZIP depth."""
import os
import pickle
import struct
import zlib

import numpy as np
import pytest
import torch

import exr_zip_cases as Z
from conftest import GOLD, synthetic_state_dict
from sceneego_amd import exr
from sceneego_amd.exr_device import decode_depth_exr_batch
from sceneego_amd.preprocess import DEPTH_CLAMP, prepare_depth

pytestmark = pytest.mark.gpu

DEMO = [os.path.join(GOLD, "demo", n + ".jpg.exr") for n in ("img_001000", "img_001796", "img_002376")]
CASES = Z.make_cases()
COMPS = ("zip", "zips", "none")
REENC = {(c, i): Z.reencode(p, c) for c in COMPS for i, p in enumerate(DEMO)}


def _host(src):
    buf = src if isinstance(src, bytes) else open(src, "rb").read()
    return exr.depth_channel(exr.read_exr_buffer(buf))


def _bits_equal(dev, ref):
    a = dev.cpu().numpy().view(np.int32)
    b = np.ascontiguousarray(ref, dtype=np.float32).view(np.int32)
    assert a.shape == b.shape
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{len(bad)} pixels differ, first at {bad[:4].tolist()}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_bit_identical(name):
    buf = CASES[name][0]
    ref = _host(buf)
    _bits_equal(decode_depth_exr_batch([buf], "cuda", clamp=None)[0], ref)
    _bits_equal(decode_depth_exr_batch([buf], "cuda", out_hw=(1024, 1280))[0], prepare_depth(ref, 1280, 1024).numpy())
    _bits_equal(decode_depth_exr_batch([buf], "cuda", out_hw=(37, 21), clamp=DEPTH_CLAMP)[0], prepare_depth(ref, 21, 37).numpy())


@pytest.mark.parametrize("comp", COMPS)
def test_demo_maps_reencoded(comp):
    bufs = [REENC[(comp, i)] for i in range(3)]
    out = decode_depth_exr_batch(bufs, "cuda", clamp=None)
    raw = decode_depth_exr_batch(bufs, "cuda", out_hw=(1024, 1280))
    for b in range(3):
        ref = _host(DEMO[b])
        assert np.array_equal(_host(bufs[b]), ref)
        _bits_equal(out[b], ref)
        _bits_equal(raw[b], prepare_depth(ref, 1280, 1024).numpy())


def _mixed(n):
    pool = [DEMO[0], REENC[("zip", 1)], REENC[("zips", 2)], REENC[("none", 0)]] + [CASES[k][0] for k in sorted(CASES)]
    return [pool[(7 * i) % len(pool)] for i in range(n)]


@pytest.mark.parametrize("B", [8, 32])
def test_mixed_batch(B):
    srcs = _mixed(B)
    out = decode_depth_exr_batch(srcs, "cuda", out_hw=(96, 120), clamp=DEPTH_CLAMP)
    for b, s in enumerate(srcs):
        _bits_equal(out[b], prepare_depth(_host(s), 120, 96).numpy())


def test_into_callers_tensor_on_side_stream():
    srcs = [REENC[("zip", 0)], DEMO[1], REENC[("zips", 2)], REENC[("none", 1)]]
    s = torch.cuda.Stream()
    out = torch.full((4, 512, 640), -7.0, device="cuda")
    with torch.cuda.stream(s):
        got, st = decode_depth_exr_batch(srcs, "cuda", out=out, clamp=None, check=False)
    s.synchronize()
    st.check()
    assert got.data_ptr() == out.data_ptr()
    for b, i in enumerate([0, 1, 2, 1]):
        _bits_equal(out[b], _host(DEMO[i]))


def test_no_host_decode(monkeypatch):
    srcs = [REENC[("zip", 0)], REENC[("zips", 1)], REENC[("none", 2)], DEMO[1], CASES["zip_wide_rgba"][0], CASES["zip_cinfo"][0]]
    refs = [prepare_depth(_host(s), 120, 96).numpy() for s in srcs]

    def boom(*a, **k):
        raise AssertionError("host decode")
    monkeypatch.setattr(exr, "read_exr_buffer", boom)
    monkeypatch.setattr(exr, "_zip_decompress", boom)
    monkeypatch.setattr(exr, "_piz_decompress", boom)
    monkeypatch.setattr(zlib, "decompress", boom)
    out = decode_depth_exr_batch(srcs, "cuda", out_hw=(96, 120))
    for b in range(len(srcs)):
        _bits_equal(out[b], refs[b])


# ------------------------------------------------------------------------------------------------------------------------------
# bad streams: one crafted chunk per status code
# ------------------------------------------------------------------------------------------------------------------------------
class _BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):                      # fields: least significant bit first
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, c, n):                     # Huffman codes: most significant bit first
        self.bits += [(c >> i) & 1 for i in range(n - 1, -1, -1)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def _fixed(symbols):
    """A zlib header and one final fixed-Huffman block of the given (kind, value) codes, then 4 zero bytes."""
    w = _BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    for kind, v in symbols:
        if kind == "lit":                     # literal/length symbol v
            if v < 144:
                w.code(0x30 + v, 8)
            elif v < 256:
                w.code(0x190 + v - 144, 9)
            elif v < 280:
                w.code(v - 256, 7)
            else:
                w.code(0xC0 + v - 280, 8)
        else:                                 # distance symbol v
            w.code(v, 5)
    return b"\x78\x01" + w.bytes() + b"\0" * 4


def _oversubscribed():
    w = _BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(0, 5)
    w.put(0, 5)
    w.put(15, 4)
    for _ in range(19):
        w.put(1, 3)                           # 19 codes of length 1
    return b"\x78\x01" + w.bytes() + b"\0" * 8


BASE = {"Y": (1, Z.W._smooth(48, 64, 3))}
RAW1 = Z.W._raw_lines(sorted((n, pt, np.asarray(a)) for n, (pt, a) in BASE.items()), 16, 16)
GOOD1 = Z.deflate(Z.predict(RAW1))
BAD = {
    "truncated": (GOOD1[:len(GOOD1) // 2], 14, "ended before its final block"),
    "btype3": (b"\x78\x01\x07" + b"\0" * 8, 9, "block type 3"),
    "len_nlen": (b"\x78\x01\x01" + struct.pack("<HH", 5, 0) + b"\0" * 9, 10, "LEN does not match NLEN"),
    "oversubscribed": (_oversubscribed(), 11, "bad Huffman code-length set"),
    "symbol286": (_fixed([("lit", 65), ("lit", 286)]), 12, "invalid deflate symbol"),
    "too_far": (_fixed([("lit", 65), ("lit", 257), ("dist", 4)]), 13, "distance too far back"),
    "adler": (GOOD1[:-1] + bytes([GOOD1[-1] ^ 0xFF]), 16, "Adler-32 mismatch"),
    "extra_byte": (Z.deflate(Z.predict(RAW1) + b"\x80"), 15, "does not inflate to the chunk's 2048 bytes"),
}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_bad_stream_reported(kind):
    stream, code, msg = BAD[kind]
    if kind not in ("extra_byte", "truncated"):
        with pytest.raises(zlib.error):
            zlib.decompress(stream)
    bad = Z.write_zip_exr(BASE, override={1: stream})
    good = Z.write_zip_exr(BASE)
    with pytest.raises(ValueError, match=rf"<bytes #1>: chunk 1: .*{msg}"):
        decode_depth_exr_batch([good, bad], "cuda")
    out = torch.full((3, 48, 64), -7.0, device="cuda")
    got, st = decode_depth_exr_batch([DEMO[0], good, bad], "cuda", out=out, out_hw=(48, 64), clamp=None, check=False)
    codes = st.status.cpu().numpy()
    n_piz = 16
    assert codes[n_piz + 3 + 1, 0] == code
    assert (np.delete(codes[:, 0], n_piz + 3 + 1) == 0).all()
    assert st.bad() == [("<bytes #2>", 1, code, st.bad()[0][3])]
    o = out.cpu().numpy()
    ref = _host(good)
    assert (o[2, 16:32] == -7.0).all()                                           # the bad chunk's rows are untouched
    assert np.array_equal(o[2, :16].view(np.int32), ref[:16].view(np.int32))
    assert np.array_equal(o[2, 32:].view(np.int32), ref[32:].view(np.int32))
    _bits_equal(got[1], ref)


def test_corruption_sweep():
    """Single-byte corruptions of ZIP chunks: where zlib accepts the chunk and yields its size, the device output is bit-identical;
    otherwise the device reports that chunk (and only it)."""
    base = Z.write_zip_exr({"Y": (1, Z.W._smooth(40, 48, 11))}, "zip", stream=lambda d, i: Z.deflate(d, level=(1, 6, 9)[i]))
    blocks = Z.chunks(base)
    hdr = exr._parse_header(base)
    offs = struct.unpack_from("<3Q", base, hdr["data_start"])
    expect = [2 * 48 * 16, 2 * 48 * 16, 2 * 48 * 8]
    rng = np.random.default_rng(1234)
    files, meta = [], []
    for _ in range(300):
        c = int(rng.integers(0, 3))
        size = len(blocks[c][1])
        k = int(rng.integers(2, size))
        buf = bytearray(base)
        old = buf[offs[c] + 8 + k]
        buf[offs[c] + 8 + k] = (old + int(rng.integers(1, 256))) & 0xFF
        try:
            ok = len(zlib.decompress(bytes(buf[offs[c] + 8:offs[c] + 8 + size]))) == expect[c]
        except zlib.error:
            ok = False
        files.append(bytes(buf))
        meta.append((c, ok))
    out, st = decode_depth_exr_batch(files, "cuda", clamp=None, check=False)
    codes = st.status.cpu().numpy()[:, 0].reshape(len(files), 3)
    n_ok = 0
    for b, (c, ok) in enumerate(meta):
        assert (np.delete(codes[b], c) == 0).all(), (b, codes[b])
        if ok:
            n_ok += 1
            assert codes[b, c] == 0, (b, c, codes[b])
            _bits_equal(out[b], _host(files[b]))
        else:
            assert codes[b, c] != 0, (b, c)
    assert 0 < n_ok < len(files)


# ------------------------------------------------------------------------------------------------------------------------------
# callers
# ------------------------------------------------------------------------------------------------------------------------------
def test_forward_on_device_zip_depth_equals_host_depth(config):
    from sceneego_amd import synth
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    net = VoxelNetwork_depth(config, device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    net = net.to("cuda").eval()
    img, _ = synth.make_inputs(5, 3, "floor")
    img = img.cuda()
    srcs = [REENC[("zip", 0)], REENC[("zips", 1)], REENC[("zip", 2)]]
    dev = decode_depth_exr_batch(srcs, "cuda", out_hw=(1024, 1280))
    host = torch.stack([prepare_depth(_host(s), 1280, 1024) for s in srcs]).cuda()
    assert torch.equal(dev, host)
    with torch.no_grad():
        a = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=dev)[0].cpu()
        b = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=host)[0].cpu()
        a2 = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=dev)[0].cpu()
    noise = float((a - a2).abs().max())              # backbone split-K atomics (pipeline.py)
    assert float((a - b).abs().max()) <= noise


def test_run_sequence_zip_depth(tmp_path, capsys):
    import run_sequence
    from sceneego_amd import synth
    srcs = []
    for i, c in enumerate(("zip", "zips", "zip")):
        p = tmp_path / f"src{i}.exr"
        p.write_bytes(REENC[(c, i)])
        srcs.append(str(p))
    root = tmp_path / "seq"
    synth.make_sequence(str(root), "zseq", 11, srcs, estimated_depth_name="est_depth", seed=5)
    preds = {}
    for decode in ("device", "host"):
        out = str(tmp_path / f"pred_{decode}.pkl")
        run_sequence.main(["--root_dir", str(root), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights",
                           "synthetic", "--depth_decode", decode, "--output", out])
        with open(out, "rb") as f:
            preds[decode] = np.stack(pickle.load(f))
    capsys.readouterr()
    assert preds["device"].shape == (11, 15, 3)
    assert np.abs(preds["device"] - preds["host"]).max() <= 2e-5          # split-K atomics of the forward (pipeline.py)
