"""GPU: the PIZ decode on the device (se_exr_piz_huffman_kernel / se_exr_piz_wavelet_kernel) is bit-identical to exr.read_depth_exr on
the three demo maps and every case of the test-side writer, with and without the clamp / nearest resize of prepare_depth; a stream
whose nBits is cut short is reported with its chunk; the forward on device-decoded depth equals the forward on host-decoded depth;
run_sequence.py gives the same predictions with either decoder, close to per-frame batch-1 runs, and prints metrics.py's numbers."""
import os
import pickle
import re
import struct

import numpy as np
import pytest
import torch

import exr_piz_writer as W
from conftest import GOLD, synthetic_state_dict
from sceneego_amd import exr
from sceneego_amd.exr_device import decode_depth_exr_batch
from sceneego_amd.preprocess import DEPTH_CLAMP, prepare_depth

pytestmark = pytest.mark.gpu

DEMO = [os.path.join(GOLD, "demo", n + ".jpg.exr") for n in ("img_001000", "img_001796", "img_002376")]
CASES = W.make_cases()


def _host(src):
    buf = src if isinstance(src, bytes) else open(src, "rb").read()
    return exr.depth_channel(exr.read_exr_buffer(buf))


def _bits_equal(dev, ref):
    a = dev.cpu().numpy().view(np.int32)
    b = np.ascontiguousarray(ref, dtype=np.float32).view(np.int32)
    assert a.shape == b.shape
    bad = np.argwhere(a != b)
    assert len(bad) == 0, f"{len(bad)} pixels differ, first at {bad[:4].tolist()}"


@pytest.mark.parametrize("src", DEMO + sorted(CASES), ids=[os.path.basename(p) for p in DEMO] + sorted(CASES))
def test_b1_bit_identical(src):
    src = CASES[src][0] if src in CASES else src
    out = decode_depth_exr_batch([src], "cuda", clamp=None)
    _bits_equal(out[0], _host(src))


@pytest.mark.parametrize("src", [DEMO[1], "odd_window", "bgr_z", "stored", "uint"])
def test_b1_clamp_and_resize_bit_identical(src):
    src = CASES[src][0] if src in CASES else src
    out = decode_depth_exr_batch([src], "cuda", out_hw=(1024, 1280))
    _bits_equal(out[0], prepare_depth(_host(src), 1280, 1024).numpy())
    out = decode_depth_exr_batch([src], "cuda", out_hw=(37, 21), clamp=DEPTH_CLAMP)           # down-sampling, odd
    _bits_equal(out[0], prepare_depth(_host(src), 21, 37).numpy())


def test_mixed_batch_of_8_with_zip_fallback():
    zip_buf = W.write_exr(CASES["odd_window"][1], compression="zip", window=(5, -3))
    srcs = [DEMO[0], CASES["w16"][0], zip_buf, CASES["skew58"][0], DEMO[2], CASES["float_z"][0], CASES["runs"][0], CASES["a_y"][0]]
    out = decode_depth_exr_batch(srcs, "cuda", out_hw=(1024, 1280))
    for b, s in enumerate(srcs):
        _bits_equal(out[b], prepare_depth(_host(s), 1280, 1024).numpy())


def test_b32_demo_maps():
    srcs = [DEMO[i % 3] for i in range(32)]
    out = decode_depth_exr_batch(srcs, "cuda", clamp=None)
    refs = [_host(p) for p in DEMO]
    for b in range(32):
        _bits_equal(out[b], refs[b % 3])


def test_b32_all_cases_resized():
    names = sorted(CASES)
    srcs = [CASES[names[i % len(names)]][0] if i % 4 else DEMO[i % 3] for i in range(32)]
    out = decode_depth_exr_batch(srcs, "cuda", out_hw=(96, 120), clamp=DEPTH_CLAMP)
    for b, s in enumerate(srcs):
        _bits_equal(out[b], prepare_depth(_host(s), 120, 96).numpy())


def test_into_callers_tensor_on_side_stream():
    s = torch.cuda.Stream()
    out = torch.full((3, 512, 640), -7.0, device="cuda")
    with torch.cuda.stream(s):
        got, st = decode_depth_exr_batch(DEMO, "cuda", out=out, clamp=None, check=False)
    s.synchronize()
    st.check()
    assert got.data_ptr() == out.data_ptr()
    for b in range(3):
        _bits_equal(out[b], _host(DEMO[b]))


def test_cut_nbits_reports_the_chunk():
    buf = bytearray(open(DEMO[0], "rb").read())
    hdr = exr._parse_header(bytes(buf))
    offs = struct.unpack_from("<16Q", buf, hdr["data_start"])
    off = offs[5]
    mn, mx = struct.unpack_from("<HH", buf, off + 8)
    p = off + 8 + 4 + (mx - mn + 1) + 4
    nbits = struct.unpack_from("<I", buf, p + 12)[0]
    struct.pack_into("<I", buf, p + 12, nbits // 2)               # every read stays inside the chunk's bytes
    with pytest.raises(ValueError, match=r"<bytes #1>: chunk 5: stream ended after \d+ of 20480 symbols"):
        decode_depth_exr_batch([DEMO[1], bytes(buf)], "cuda")
    _, st = decode_depth_exr_batch([DEMO[1], bytes(buf)], "cuda", check=False)
    codes = st.status.cpu().numpy()
    assert codes[16 + 5, 0] == 6 and (np.delete(codes[:, 0], 16 + 5) == 0).all()
    assert 0 < codes[16 + 5, 1] < 20480


def test_forward_on_device_depth_equals_host_depth(config):
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    from sceneego_amd import synth
    net = VoxelNetwork_depth(config, device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    net = net.to("cuda").eval()
    img, _ = synth.make_inputs(5, 3, "floor")
    img = img.cuda()
    dev = decode_depth_exr_batch(DEMO, "cuda", out_hw=(1024, 1280))
    host = torch.stack([prepare_depth(_host(p), 1280, 1024) for p in DEMO]).cuda()
    assert torch.equal(dev, host)
    with torch.no_grad():
        a = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=dev)[0].cpu()
        b = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=host)[0].cpu()
        a2 = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=dev)[0].cpu()
    # identical inputs; the forward itself repeats to the bit unless its backbone's split-K atomics reorder (pipeline.py: ~6e-6 m)
    noise = float((a - a2).abs().max())
    assert float((a - b).abs().max()) <= noise, (float((a - b).abs().max()), noise)


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    from sceneego_amd import synth
    root = tmp_path_factory.mktemp("seq")
    synth.make_sequence(str(root), "seq19", 19, DEMO, estimated_depth_name="est_depth", seed=3)
    return str(root)


def _run(root, capsys, tmp, decode):
    import run_sequence
    out = os.path.join(tmp, f"pred_{decode}.pkl")
    r = run_sequence.main(["--root_dir", root, "--seq_name", "seq19", "--estimated_depth_name", "est_depth", "--weights", "synthetic",
                           "--depth_decode", decode, "--output", out])
    text = capsys.readouterr().out
    with open(out, "rb") as f:
        preds = pickle.load(f)
    return r, text, preds


def test_run_sequence(sequence, capsys, tmp_path, config):
    import run_sequence
    from sceneego_amd import metrics as M
    r_dev, text, p_dev = _run(sequence, capsys, str(tmp_path), "device")
    _, _, p_host = _run(sequence, capsys, str(tmp_path), "host")
    assert len(p_dev) == 19 and all(p.shape == (15, 3) and p.dtype == np.float32 for p in p_dev)
    # same depth bits -> the same forward, to its run-to-run reproducibility (backbone split-K atomics: ~6e-6 m, pipeline.py)
    assert np.abs(np.stack(p_dev) - np.stack(p_host)).max() <= 2e-5
    # printed metrics are metrics.py on the pickled predictions
    _, poses, _ = run_sequence.frame_list(sequence, "seq19", "est_depth")
    pred, gt = np.stack(p_dev).astype(np.float64), np.stack(poses).astype(np.float64)
    assert float(re.search(r"^mpjpe: (\S+)$", text, re.M).group(1)) == M.mpjpe(pred, gt)
    assert float(re.search(r"^pa mpjpe: (\S+)$", text, re.M).group(1)) == M.pa_mpjpe(pred, gt)
    assert re.search(r"^frames/s: [0-9.]+ \(19 frames", text, re.M)
    # per-frame batch-1 runs of demo.py on the same images and depth maps
    import demo
    d = demo.Demo(config, os.path.join(sequence, "seq19", "imgs"), os.path.join(sequence, "seq19", "est_depth"), weights="synthetic")
    ref = np.stack([x["predicted_keypoints"] for x in d.run()])
    assert ref.shape == (19, 15, 3)
    assert np.abs(ref - np.stack(p_dev)).max() <= 1e-4
