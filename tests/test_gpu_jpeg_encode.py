"""GPU: the JPEG encoder (csrc/jpeg_enc.hip through sceneego_amd/jpeg_encode.py) against the numpy model, PIL and the project's own
decoder on the case list of tests/jpeg_encode_cases.py; reproducibility, streams, the capacity contract, and demo.py /
run_sequence.py end to end."""
import functools
import io
import os
import shutil

import numpy as np
import pytest
import torch

import jpeg_encode_cases as C
import jpeg_encode_model as M
from conftest import GOLD
from sceneego_amd import _lib, synth
from sceneego_amd.jpeg_device import decode_jpeg_batch
from sceneego_amd.jpeg_encode import JpegEncoder, quant_tables

pytestmark = pytest.mark.gpu
CASE_IDS = [c.name for c in C.CASES]


@functools.lru_cache(maxsize=None)
def _encoder():
    return JpegEncoder("cuda")


def _device_frames(case):
    f = case.frames if case.order == "rgb" else case.frames[..., ::-1]
    return torch.from_numpy(np.array(f)).cuda()


@functools.lru_cache(maxsize=None)
def _device_files(name):
    c = C.BY_NAME[name]
    return tuple(_encoder().encode(_device_frames(c), quality=c.quality, subsampling=c.subsampling, restart_rows=c.restart_rows,
                                   order=c.order))


@pytest.mark.parametrize("name", CASE_IDS)
def test_files_equal_the_model_and_pil(name):
    got = _device_files(name)
    want, _ = C.model_files(name)
    pil = C.pil_files(name)
    assert len(got) == len(want)
    for b, (g, w, p) in enumerate(zip(got, want, pil)):
        assert len(M.scan_of(g)) == len(M.scan_of(w)), (b, len(M.scan_of(g)), len(M.scan_of(w)))
        assert g == w, f"frame {b}: first differing byte {next(i for i, (x, y) in enumerate(zip(g, w)) if x != y)}"
        assert M.scan_of(g) == M.scan_of(p) and M.dqt_of(g) == M.dqt_of(p)


@pytest.mark.parametrize("name", CASE_IDS)
def test_pil_reads_the_same_pixels(name):
    for g, p in zip(_device_files(name), C.pil_files(name)):
        assert np.array_equal(C.pil_decode(g), C.pil_decode(p))


@pytest.mark.parametrize("name", CASE_IDS)
def test_round_trip_through_the_device_decoder(name):
    files = _device_files(name)
    back = decode_jpeg_batch(list(files), "cuda").cpu().numpy()              # B, G, R
    for b, g in enumerate(files):
        assert np.array_equal(back[b][:, :, ::-1], C.pil_decode(g))


def test_repeatable_and_independent_of_stream_and_batch_position():
    c = C.BY_NAME["136x200-noise-q100-444-r1-rgb"]
    other = C.BY_NAME["136x200-crop-q90-444-r0-rgb"]
    a, x = _device_frames(c)[0], _device_frames(other)[0]
    enc = _encoder()
    first = enc.encode(a[None], quality=100, restart_rows=1)
    assert enc.encode(a[None], quality=100, restart_rows=1) == first
    assert first[0] == C.model_files(c.name)[0][0]
    # frames 0 and 2 equal, frame 1 different
    three = enc.encode(torch.stack([a, x, a]), quality=100, restart_rows=1)
    assert three[0] == first[0] and three[2] == first[0] and three[1] != first[0]
    assert three[1] == enc.encode(x[None], quality=100, restart_rows=1)[0]
    # a second encoder on a side stream, interleaved with this one on the current stream
    side_enc, side = JpegEncoder("cuda"), torch.cuda.Stream()
    ql, qc = quant_tables(100)
    cap = JpegEncoder.worst_case_bytes(136, 200, "444", 1)           # quality-100 noise codes to more than the default 3 H W bytes
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_s, _, status_s = side_enc.launch(x[None], ql, qc, "444", 1, capacity=cap)
    out_m, _, status_m = enc.launch(a[None], ql, qc, "444", 1, capacity=cap)
    with torch.cuda.stream(side):
        from_side = side_enc.encode(x[None], quality=100, restart_rows=1)
    torch.cuda.synchronize()
    assert enc.retries >= 1                                           # ... so the calls on the noise frame above ran twice
    for out, status, want in ((out_s, status_s, three[1]), (out_m, status_m, first[0])):
        st = status.cpu().numpy()
        assert st[0, 0] == 0 and out[0, :st[0, 1]].cpu().numpy().tobytes() == M.scan_of(want)
    assert from_side[0] == three[1]


def test_capacity_contract():
    c = C.BY_NAME["16x24-noise-q100-444-r0-rgb"]
    frames = _device_frames(c)
    want = C.model_files(c.name)[0][0]
    need = len(M.scan_of(want))
    assert need > 64
    lib = _lib.load()
    ql, qc = quant_tables(100)
    n = _lib.jpeg_encode_scratch_bytes(1, 16, 24, 444)
    scratch = torch.empty(n, device="cuda", dtype=torch.uint8)
    length = torch.full((1,), -7, device="cuda", dtype=torch.int32)
    status = torch.full((1, 2), -7, device="cuda", dtype=torch.int32)
    for cap in (64, need - 1, need, need + 5):
        buf = torch.full((cap + 4096,), 0xA5, device="cuda", dtype=torch.uint8)        # the slot, then a guard region
        _lib.jpeg_encode(frames, ql, qc, 444, 0, buf[:cap].view(1, cap), length, status, scratch)
        host, st = buf.cpu().numpy(), status.cpu().numpy()
        assert (host[cap:] == 0xA5).all(), f"capacity {cap}: bytes written past the slot"
        assert st[0, 1] == need
        if cap < need:
            assert st[0, 0] == 1 and int(length[0]) == 0
            assert host[:cap].tobytes() == M.scan_of(want)[:cap]
        else:
            assert st[0, 0] == 0 and int(length[0]) == need
            assert host[:need].tobytes() == M.scan_of(want) and (host[need:cap] == 0xA5).all()
    # the wrapper: one retry with the worst-case bound
    enc = JpegEncoder("cuda")
    assert enc.encode(frames, quality=100, capacity=64) == [want] and enc.retries == 1
    assert enc.encode(frames, quality=100, capacity=need) == [want] and enc.retries == 1
    # bad arguments are refused before anything is launched
    out = torch.empty((1, 4096), device="cuda", dtype=torch.uint8)
    args = lambda **k: {**dict(f=frames.data_ptr(), b=1, h=16, w=24, sub=444, rr=0, cap=4096, nbytes=n), **k}    # noqa: E731

    def call(f, b, h, w, sub, rr, cap, nbytes, q=ql):
        return lib.se_jpeg_encode_u8(f, b, h, w, 0, q.ctypes.data, qc.ctypes.data, sub, rr, out.data_ptr(), cap, length.data_ptr(),
                                     status.data_ptr(), scratch.data_ptr(), nbytes, None)
    assert call(**args()) == 0
    zero_q = ql.copy()
    zero_q[5] = 0
    for bad in (args(f=None), args(b=0), args(h=0), args(sub=422), args(rr=-1), args(cap=-1), args(nbytes=n - 1), args(q=zero_q)):
        assert call(**bad) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        enc.encode(frames.float())
    with pytest.raises(ValueError):
        enc.encode(frames[:, :, ::2])
    with pytest.raises(ValueError):
        enc.encode(frames, quality=0)
    with pytest.raises(ValueError):
        enc.encode(frames, subsampling="422")


def test_encode_under_graph_capture():
    c = C.BY_NAME["17x33-texel-q100-444-r1-rgb"]
    frames = _device_frames(c)
    want = M.scan_of(C.model_files(c.name)[0][0])
    enc = JpegEncoder("cuda")
    ql, qc = quant_tables(100)
    cap = JpegEncoder.worst_case_bytes(17, 33, "444", 1)
    enc.launch(frames, ql, qc, "444", 1, capacity=cap)   # buffers exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _, status = enc.launch(frames, ql, qc, "444", 1, capacity=cap)
    out.zero_()
    status.zero_()
    g.replay()
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert st.tolist() == [[0, len(want)]] and out[0, :st[0, 1]].cpu().numpy().tobytes() == want


# --------------------------------------------------------------------------------------------------------------- end to end
def _pil_jpeg(rgb):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format="JPEG", quality=90, subsampling=0, optimize=False)
    return b.getvalue()


def test_demo_render_format_jpg(tmp_path, capsys):
    import demo
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg"), img_dir / "a_001000.jpg")
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), depth_dir / "a_001000.jpg.exr")
    common = ["--img_dir", str(img_dir), "--depth_dir", str(depth_dir), "--weights", "synthetic"]
    demo.main(common + ["--output_dir", str(tmp_path / "o1"), "--render_dir", str(tmp_path / "png")])
    demo.main(common + ["--output_dir", str(tmp_path / "o2"), "--render_dir", str(tmp_path / "jpg"), "--render_format", "jpg"])
    capsys.readouterr()
    assert sorted(os.listdir(tmp_path / "jpg")) == ["a_001000.jpg.overlay.jpg", "a_001000.jpg.render.jpg"]
    assert (tmp_path / "o1" / "a_001000.jpg.pkl").read_bytes() == (tmp_path / "o2" / "a_001000.jpg.pkl").read_bytes()
    for view, size in (("render", (720, 960)), ("overlay", (1024, 1280))):
        saved = C.pil_decode((tmp_path / "png" / f"a_001000.jpg.{view}.png").read_bytes())      # what the PNG path saved
        assert saved.shape == size + (3,)
        got = (tmp_path / "jpg" / f"a_001000.jpg.{view}.jpg").read_bytes()
        want = _pil_jpeg(saved)
        assert np.array_equal(C.pil_decode(got), C.pil_decode(want))
        assert M.scan_of(got) == M.scan_of(want)


def test_run_sequence_render_video(tmp_path, capsys):
    import run_sequence
    depths = [os.path.join(GOLD, "demo", n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 3, depths, estimated_depth_name="est_depth", seed=5)
    common = ["--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
    plain = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl")])
    drawn = run_sequence.main(common + ["--output", str(tmp_path / "drawn.pkl"), "--render_video", str(tmp_path / "v" / "seq.avi"),
                                        "--render_fps", "30", "--render_dir", str(tmp_path / "jpg"), "--render_format", "jpg"])
    capsys.readouterr()
    assert (tmp_path / "plain.pkl").read_bytes() == (tmp_path / "drawn.pkl").read_bytes()
    assert len(plain["predictions"]) == len(drawn["predictions"]) == 3
    payloads = C.check_avi((tmp_path / "v" / "seq.avi").read_bytes(), 3, 960, 720, 30)
    assert len({p for p in payloads}) >= 2                               # different depth maps: different views
    assert len(os.listdir(tmp_path / "jpg")) == 6
    from sceneego_amd.jpeg_device import JpegFile
    for p in payloads:
        f = JpegFile(p)
        assert f.device and (f.hmax, f.vmax) == (2, 2) and f.restart == 0          # 4:2:0, what players expect of MJPG
