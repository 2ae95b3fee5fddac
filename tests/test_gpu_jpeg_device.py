"""Device JPEG decode (sceneego_amd/jpeg_device.py, csrc/jpeg.hip): bit-identical to load_image_bgr (PIL) over sizes, sampling,
quality, Huffman tables, restart intervals, content and batch sizes; the committed demo frame; the repair-only path; host fall-backs
inside a batch; a cut file; repeatability and streams; run_sequence.py and demo.py with either image decoder."""
import io
import os

import numpy as np
import pytest
import torch

from sceneego_amd.jpeg_device import decode_jpeg_batch
from sceneego_amd.preprocess import load_image_bgr, normalize_u8, preprocess_image_device

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEMO = os.path.join(HERE, "golden", "demo")
DEV = "cuda"


def _enc(arr, **kw):
    from PIL import Image, ImageFile
    b = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 26        # an optimized encode of a large noise image needs its whole output in one buffer
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


def _content(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "const":
        return np.full((H, W, 3), 93, dtype=np.uint8)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = rng.uniform(0, 6.283, 3)
    rgb = np.stack([127 + 100 * np.sin(xs / (37 + 9 * c) + ys / (53 - 7 * c) + ph[c]) for c in range(3)], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _check(datas, **kw):
    out = decode_jpeg_batch(datas, DEV, **kw)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i, d in enumerate(datas):
        ref = _pil(d)
        assert got[i].shape == ref.shape
        if not np.array_equal(got[i], ref):
            bad = np.argwhere(got[i] != ref)
            pytest.fail(f"slot {i}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[i][tuple(bad[0])]} != {ref[tuple(bad[0])]}")
    return out


SIZES = [(1024, 1280), (1024, 1024), (1023, 1279), (17, 33), (16, 16), (8, 8), (1, 1)]
SUBS = [0, 1, 2, "L"]
QUALITIES = [5, 50, 90, 100]
RESTARTS = [{}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1}, {"restart_marker_rows": 3}]
CONTENTS = ["noise", "grad", "const"]


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("hw", SIZES, ids=[f"{w}x{h}" for h, w in SIZES])
def test_matrix_equals_pil(hw, sub):
    H, W = hw
    datas = []
    for i in range(12):
        arr = _content(CONTENTS[i % 3], H, W, seed=17 * i + H + W)
        kw = dict(quality=QUALITIES[i % 4], optimize=bool((i // 2) % 2), **RESTARTS[(i // 3) % 4])
        if sub == "L":
            datas.append(_enc(arr[:, :, 1].copy(), **kw))
        else:
            datas.append(_enc(arr, subsampling=sub, **kw))
    _check(datas)


@pytest.mark.parametrize("B", [1, 8, 32])
def test_batches_demo_size(B):
    datas = [_enc(_content("grad" if b % 4 else "noise", 1024, 1280, seed=100 + b), quality=(90, 95, 75, 100)[b % 4],
                  subsampling=(2, 2, 1, 0)[b % 4]) for b in range(B)]
    _check(datas)


def test_demo_frame():
    p = os.path.join(DEMO, "img_001000.jpg")
    out = decode_jpeg_batch([p], DEV)
    np.testing.assert_array_equal(out[0].cpu().numpy(), load_image_bgr(p))
    small = np.load(os.path.join(DEMO, "img_001000_256_bgr_u8.npz"))
    small = small[small.files[0]]
    got = preprocess_image_device(out).cpu()
    assert torch.equal(got[0], normalize_u8(small))


def test_repair_only_is_identical():
    datas = [_enc(_content("noise", 1024, 1280, 5), quality=100), _enc(_content("const", 1024, 1280, 0), quality=90),
             open(os.path.join(DEMO, "img_001000.jpg"), "rb").read(),
             _enc(_content("grad", 1024, 1280, 9), quality=50, restart_marker_rows=3)]
    a = _check(datas, rounds=0)
    b = decode_jpeg_batch(datas, DEV)
    c = decode_jpeg_batch(datas, DEV, rounds=8)
    assert torch.equal(a, b) and torch.equal(b, c)


def test_mixed_batch_falls_back_in_order():
    from PIL import Image
    arr = _content("grad", 48, 64, 3)
    cmyk, png = io.BytesIO(), io.BytesIO()
    Image.fromarray(arr).convert("CMYK").save(cmyk, "JPEG", quality=90)
    Image.fromarray(arr).save(png, "PNG")
    datas = [_enc(arr, quality=90), _enc(arr, quality=80, progressive=True), cmyk.getvalue(), _enc(arr[:, :, 0].copy(), quality=70),
             png.getvalue(), _enc(_content("noise", 48, 64, 4), quality=95, subsampling=1)]
    _check(datas)


def test_cut_file_raises_and_recovers(tmp_path):
    good = _enc(_content("noise", 256, 320, 1), quality=90)
    sos = good.find(b"\xff\xda")
    cut = good[:sos + (len(good) - sos) // 2]
    p = tmp_path / "cut.jpg"
    p.write_bytes(cut)
    with pytest.raises(ValueError, match="cut.jpg.*stream ended"):
        decode_jpeg_batch([str(p)], DEV)
    torch.cuda.synchronize()
    _check([good, good])


def test_repeatable_and_streams():
    datas = [_enc(_content("noise", 512, 640, s), quality=95) for s in range(4)]
    a = decode_jpeg_batch(datas, DEV)
    b = decode_jpeg_batch(datas, DEV)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = decode_jpeg_batch(datas, DEV)
    s.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


# ------------------------------------------------------------------------------------------------------------------ callers
def test_run_sequence_device_vs_host(tmp_path, config, monkeypatch):
    import run_sequence
    from sceneego_amd import synth
    depths = [os.path.join(DEMO, n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
    synth.make_sequence(str(tmp_path), "seq", 11, depths, seed=5)
    images, _, deps = run_sequence.frame_list(str(tmp_path), "seq", "est_depth")
    captured = {}
    orig = run_sequence.SequenceRunner._images

    def spy(self, frames):
        out = orig(self, frames)
        captured.setdefault(self.image_decode, []).append(out.clone())
        return out

    monkeypatch.setattr(run_sequence.SequenceRunner, "_images", spy)
    preds = {}
    for mode in ("device", "host"):
        runner = run_sequence.SequenceRunner(config, weights="synthetic", image_decode=mode)
        preds[mode] = np.stack(runner.run(images, deps, 4))
    assert len(captured["device"]) == len(captured["host"]) == 3            # 4 + 4 + 3: a partial last batch
    for a, b in zip(captured["device"], captured["host"]):
        assert torch.equal(a, b)
    assert np.abs(preds["device"] - preds["host"]).max() <= 2e-5


def test_demo_device_vs_host(tmp_path, config):
    import shutil

    import demo
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    shutil.copy(os.path.join(DEMO, "img_001000.jpg"), img_dir)
    shutil.copy(os.path.join(DEMO, "img_001000.jpg.exr"), depth_dir)
    got = {}
    for mode in ("device", "host"):
        d = demo.Demo(config, str(img_dir), str(depth_dir), weights="synthetic", image_decode=mode)
        seen = []
        fwd = d.network.forward

        def spy(img, *a, **k):
            seen.append(img.clone())
            return fwd(img, *a, **k)

        d.network.forward = spy
        res = d.run()
        got[mode] = (seen[0], res[0]["predicted_keypoints"])
    assert torch.equal(got["device"][0], got["host"][0])
    assert np.abs(got["device"][1] - got["host"][1]).max() <= 2e-5
