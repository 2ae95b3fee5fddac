"""GPU: the PNG encoder (csrc/png_enc.hip through sceneego_amd/png_encode.py) against the numpy model, PIL and zlib on the case list
of tests/png_encode_cases.py; batches, repeatability, guard bands, graph capture, full-size frames, and demo.py / run_sequence.py
end to end."""
import functools
import os
import shutil
import zlib

import numpy as np
import pytest
import torch

import png_encode_cases as C
import png_encode_model as M
from conftest import GOLD
from sceneego_amd import _lib, synth
from sceneego_amd.png_encode import PngEncoder

pytestmark = pytest.mark.gpu
CASE_IDS = [c.name for c in C.CASES]


@functools.lru_cache(maxsize=None)
def _encoder():
    return PngEncoder("cuda")


def _first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


@pytest.mark.parametrize("name", CASE_IDS)
def test_kernel_bytes_equal_model_bytes(name):
    c = C.BY_NAME[name]
    (got,) = _encoder().encode(torch.from_numpy(c.image).cuda()[None])
    want, _ = C.model_file(name)
    assert len(got) == len(want), (len(got), len(want), _first_difference(got, want))
    assert got == want, f"first differing byte {_first_difference(got, want)}"
    pixels, mode = C.pil_decode(got)
    assert mode == ("RGB" if c.channels == 3 else "L") and np.array_equal(pixels, c.image)


def test_batch_of_three_equals_each_alone_and_repeats():
    frames = torch.from_numpy(np.stack([C.BY_NAME[n].image for n in C.BATCH])).cuda()
    enc = _encoder()
    three = enc.encode(frames)
    assert three == enc.encode(frames)                                       # two calls, the same bytes
    assert len({len(f) for f in three}) == 3
    for b, name in enumerate(C.BATCH):
        assert three[b] == enc.encode(frames[b:b + 1])[0]
        assert three[b] == C.model_file(name)[0]
    st = enc.last_status
    assert st.shape == (1, 2) and st[0, 0] == 0
    gray = torch.from_numpy(np.stack([C.BY_NAME["zeros-over-two-segments-gray"].image] * 2)).cuda()
    assert enc.encode(gray) == [C.model_file("zeros-over-two-segments-gray")[0]] * 2


def test_guard_bands_stay_intact():
    """Output, length and status sit inside larger buffers filled with a pattern: nothing outside them is written, and inside the
    output nothing beyond the stream."""
    name = "uniform-random-gray"                                             # stored: the stream is as long as a stream gets
    image = C.BY_NAME[name].image
    frames = torch.from_numpy(np.stack([image, image[::-1].copy()])).cuda()
    B, H, W = frames.shape
    want = [M.idat_of(M.encode(f.cpu().numpy())) for f in frames]
    bound = PngEncoder.bound(H, W, 1)
    assert max(len(w) for w in want) == bound - 5 * 2                        # two segments, both stored
    guard = 4096
    n = _lib.png_encode_scratch_bytes(B, H, W, 1)
    scratch = torch.empty(n, device="cuda", dtype=torch.uint8)
    for cap in (bound, bound + 37):
        buf = torch.full((guard + B * cap + guard,), 0xA5, device="cuda", dtype=torch.uint8)
        ints = torch.full((64 + B + 64 + 2 * B + 64,), -7, device="cuda", dtype=torch.int32)
        out = buf[guard:guard + B * cap].view(B, cap)
        length, status = ints[64:64 + B], ints[128 + B:128 + 3 * B].view(B, 2)
        _lib.png_encode(frames, out, length, status, scratch)
        host, ih = buf.cpu().numpy(), ints.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + B * cap:] == 0xA5).all()
        assert (ih[:64] == -7).all() and (ih[64 + B:128 + B] == -7).all() and (ih[128 + 3 * B:] == -7).all()
        for b in range(B):
            slot = host[guard + b * cap:guard + (b + 1) * cap]
            assert ih[64 + b] == len(want[b]) and ih[128 + B + 2 * b:130 + B + 2 * b].tolist() == [0, len(want[b])]
            assert slot[:len(want[b])].tobytes() == want[b] and (slot[len(want[b]):] == 0xA5).all()
    # bad arguments are refused before anything is launched
    lib = _lib.load()
    out = torch.empty((B, bound), device="cuda", dtype=torch.uint8)
    length = torch.empty(B, device="cuda", dtype=torch.int32)
    status = torch.empty((B, 2), device="cuda", dtype=torch.int32)
    args = lambda **k: {**dict(f=frames.data_ptr(), o=out.data_ptr(), b=B, h=H, w=W, ch=1, cap=bound, nbytes=n), **k}    # noqa: E731

    def call(f, o, b, h, w, ch, cap, nbytes):
        return lib.se_png_encode_u8(f, o, length.data_ptr(), status.data_ptr(), scratch.data_ptr(), nbytes, b, h, w, ch, cap, None)
    assert call(**args()) == 0
    for bad in (args(f=None), args(o=None), args(b=0), args(h=0), args(w=0), args(ch=2), args(cap=bound - 1), args(nbytes=n - 1)):
        assert call(**bad) == -1
    torch.cuda.synchronize()


def test_launch_under_graph_capture():
    name = "render-like-96x128"
    frames = torch.from_numpy(C.BY_NAME[name].image).cuda()[None]
    want = M.idat_of(C.model_file(name)[0])
    enc = PngEncoder("cuda")
    enc.launch(frames)                                                       # buffers exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, length, status = enc.launch(frames)
    for _ in range(2):
        out.zero_()
        status.zero_()
        length.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert status.cpu().numpy().tolist() == [[0, len(want)]] and int(length[0]) == len(want)
        assert out[0, :len(want)].cpu().numpy().tobytes() == want


@functools.lru_cache(maxsize=None)
def _golden_frame():
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLD, "demo", "img_001000.jpg")).convert("RGB"))


@pytest.mark.parametrize("which", ["render-like-720x960", "golden-demo-1024x1280"])
def test_full_size_frames(which):
    image = C.render_like(720, 960) if which.startswith("render") else _golden_frame()
    h, w = image.shape[:2]
    (data,) = _encoder().encode(torch.from_numpy(image).cuda()[None])
    pixels, mode = C.pil_decode(data)
    assert mode == "RGB" and np.array_equal(pixels, image)                   # the exact pixels
    idat = M.idat_of(data)
    f = zlib.decompress(idat)                                                # inflates, and the Adler-32 is right
    assert len(f) == h * (1 + 3 * w) and f == M.filter_stream(image)[0].tobytes()
    assert len(idat) <= M.zlib_bound(len(f)) == PngEncoder.bound(h, w, 3)
    print(f"{which}: device {len(data)} bytes, PIL {C.pil_size(image)} bytes, raw {image.size}")


# --------------------------------------------------------------------------------------------------------------- end to end
def _same_pixels(dir_a, dir_b, names):
    for n in names:
        a, _ = C.pil_decode((dir_a / n).read_bytes())
        b, _ = C.pil_decode((dir_b / n).read_bytes())
        assert a.shape == b.shape and np.array_equal(a, b), n


def test_demo_png_encoder_device(tmp_path, capsys):
    import demo
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg"), img_dir / "a_001000.jpg")
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), depth_dir / "a_001000.jpg.exr")
    common = ["--img_dir", str(img_dir), "--depth_dir", str(depth_dir), "--weights", "synthetic"]
    demo.main(common + ["--output_dir", str(tmp_path / "o1"), "--render_dir", str(tmp_path / "host")])
    demo.main(common + ["--output_dir", str(tmp_path / "o2"), "--render_dir", str(tmp_path / "device"), "--png_encoder", "device"])
    capsys.readouterr()
    names = ["a_001000.jpg.overlay.png", "a_001000.jpg.render.png"]
    assert sorted(os.listdir(tmp_path / "device")) == names == sorted(os.listdir(tmp_path / "host"))
    assert (tmp_path / "o1" / "a_001000.jpg.pkl").read_bytes() == (tmp_path / "o2" / "a_001000.jpg.pkl").read_bytes()
    _same_pixels(tmp_path / "host", tmp_path / "device", names)
    for n in names:                                                          # the device wrote these, not PIL
        assert M.idat_of((tmp_path / "device" / n).read_bytes())[:2] == b"\x78\x01"


def test_run_sequence_png_encoder_device(tmp_path, capsys):
    import run_sequence
    depths = [os.path.join(GOLD, "demo", n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 3, depths, estimated_depth_name="est_depth", seed=5)
    common = ["--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
    host = run_sequence.main(common + ["--output", str(tmp_path / "host.pkl"), "--render_dir", str(tmp_path / "host")])
    dev = run_sequence.main(common + ["--output", str(tmp_path / "dev.pkl"), "--render_dir", str(tmp_path / "device"),
                                      "--png_encoder", "device"])
    capsys.readouterr()
    assert (tmp_path / "host.pkl").read_bytes() == (tmp_path / "dev.pkl").read_bytes()
    assert len(host["predictions"]) == len(dev["predictions"]) == 3
    names = sorted(os.listdir(tmp_path / "host"))
    assert len(names) == 6 and names == sorted(os.listdir(tmp_path / "device"))
    _same_pixels(tmp_path / "host", tmp_path / "device", names)
    for n in names:
        assert M.idat_of((tmp_path / "device" / n).read_bytes())[:2] == b"\x78\x01"
