"""CPU: the numpy model of the JPEG encoder (tests/jpeg_encode_model.py) against PIL (libjpeg-turbo) on the case list, the AVI
writer, the new command-line switches and the encoder's refusal of host tensors.  No GPU."""
import numpy as np
import pytest
import torch

import jpeg_encode_cases as C
import jpeg_encode_model as M
import jpeg_model
from sceneego_amd import _lib
from sceneego_amd.jpeg_device import JpegFile
from sceneego_amd.jpeg_encode import JpegEncoder, MjpegWriter, file_header, quant_tables

CASE_IDS = [c.name for c in C.CASES]
WORKGROUP_BLOCKS = 256        # JE_CHUNK of csrc/jpeg_enc.hip: blocks per workgroup of the size / pack kernels


def _coefficients(data):
    """Quantised coefficients of a file through the project's own reader: int32 [blocks, 64], natural order, DC predicted."""
    f = JpegFile(data)
    assert f.device, f.why
    rows, nbs = [], []
    for _, mc, seg in f.segments:
        rows.append(jpeg_model.decode_segment(f, seg, mc * f.blocks_per_mcu)[0])
        nbs.append(mc * f.blocks_per_mcu)
    return jpeg_model.dc_predict(np.concatenate(rows), f, nbs)


def test_case_list_covers_what_the_issue_names():
    shapes = {c.shape for c in C.CASES}
    assert shapes == set(C.SHAPES)
    assert {c.quality for c in C.CASES} == {10, 50, 75, 90, 95, 100}
    assert {c.subsampling for c in C.CASES} == {"444", "420"} and {c.restart_rows for c in C.CASES} == {0, 1}
    assert {len(c.kinds) for c in C.CASES} == {1, 3} and {c.order for c in C.CASES} == {"rgb", "bgr"}
    assert {k for c in C.CASES for k in c.kinds} == set(C.CONTENT)
    for c in C.CASES:
        if len(c.kinds) == 3:
            assert not np.array_equal(c.frames[0], c.frames[1]) and not np.array_equal(c.frames[1], c.frames[2])


def test_case_list_exercises_every_coding_path():
    """A condition on the inputs, from the model's own statistics.  DC category 11 and AC category 10 are the largest an 8-bit
    baseline file can hold (|DC difference| <= 2040, |AC| <= 1023 with a quantiser of 1) and both are reached."""
    stats = [C.model_files(c.name)[1] for c in C.CASES]
    assert sum(s.zrl for s in stats) > 0, "no ZRL symbol"
    assert sum(s.no_eob for s in stats) > 0, "no block without EOB"
    assert sum(s.stuffed for s in stats) > 0, "no FF byte to stuff"
    assert max(s.max_ac_cat for s in stats) == 10, max(s.max_ac_cat for s in stats)
    assert max(s.max_dc_cat for s in stats) == 11, max(s.max_dc_cat for s in stats)
    assert sum(s.pad_bits for s in stats) > 0, "no padding bits"
    per_frame = max(s.blocks // len(c.kinds) for s, c in zip(stats, C.CASES))
    assert per_frame > 2 * WORKGROUP_BLOCKS, per_frame
    # ... also with restart intervals longer than one workgroup's share, and with intervals shorter than it
    assert any(c.restart_rows == 0 and s.blocks // len(c.kinds) > WORKGROUP_BLOCKS for s, c in zip(stats, C.CASES))


@pytest.mark.parametrize("name", CASE_IDS)
def test_model_tables_and_scan_equal_pil(name):
    files, _ = C.model_files(name)
    for mine, pil in zip(files, C.pil_files(name)):
        assert M.dqt_of(mine) == M.dqt_of(pil)
        assert M.scan_of(mine) == M.scan_of(pil)


@pytest.mark.parametrize("name", CASE_IDS)
def test_model_coefficients_equal_pil(name):
    files, _ = C.model_files(name)
    for mine, pil in zip(files, C.pil_files(name)):
        a, b = _coefficients(mine), _coefficients(pil)
        assert a.shape == b.shape and int((a != b).sum()) == 0


@pytest.mark.parametrize("name", CASE_IDS)
def test_model_files_decode_like_pil(name):
    files, _ = C.model_files(name)
    c = C.BY_NAME[name]
    for data in files:
        f = JpegFile(data)
        assert f.device, f.why
        assert (f.H, f.W) == c.shape and f.restart == (c.restart_rows * f.mcus_x if c.restart_rows else 0)
        assert np.array_equal(jpeg_model.decode(f)[:, :, ::-1], C.pil_decode(data))


def test_package_headers_and_tables_equal_the_model():
    for q in (1, 10, 49, 50, 75, 90, 95, 100):
        for a, b in zip(quant_tables(q), M.quant_tables(q)):
            assert a.dtype == np.uint16 and np.array_equal(a, b)
    ql, qc = quant_tables(75)
    for sub in ("444", "420"):
        for rst in (0, 7):
            assert file_header(17, 33, ql, qc, sub, rst) == M.headers(17, 33, ql, qc, sub, rst)
    for bad in (0, 101, 50.5):
        with pytest.raises(ValueError):
            quant_tables(bad)


# ------------------------------------------------------------------------------------------------------------------------- AVI
def _frames_for_avi():
    files = [C.model_files(n)[0][0] for n in CASE_IDS if C.BY_NAME[n].shape == (17, 33)]
    assert any(len(f) & 1 for f in files) and any(not len(f) & 1 for f in files)      # odd and even lengths
    return files


@pytest.mark.parametrize("fps", [25, 30, 12.5])
def test_mjpeg_writer(tmp_path, fps):
    files = _frames_for_avi()
    path = tmp_path / "clip.avi"
    with MjpegWriter(str(path), 33, 17, fps) as w:
        for f in files:
            w.write(f)
    data = path.read_bytes()
    payloads = C.check_avi(data, len(files), 33, 17, fps)
    assert payloads == files
    with pytest.raises(ValueError):
        w.write(files[0])                          # closed


def test_mjpeg_writer_refuses_what_it_cannot_hold(tmp_path, monkeypatch):
    import sceneego_amd.jpeg_encode as je
    files = _frames_for_avi()
    w = MjpegWriter(str(tmp_path / "small.avi"), 33, 17, 25)
    with pytest.raises(ValueError, match="not a JPEG"):
        w.write(b"RIFFxxxx")
    monkeypatch.setattr(je, "AVI_MAX_BYTES", 2 * len(files[0]) + 700)
    w.write(files[0])
    with pytest.raises(ValueError, match="2 GB"):
        for f in files:
            w.write(f)
    w.close()
    C.check_avi((tmp_path / "small.avi").read_bytes(), len(w.index), 33, 17, 25)      # what was written stays a valid file
    w = MjpegWriter(str(tmp_path / "empty.avi"), 8, 8, 25)
    w.close()
    C.check_avi((tmp_path / "empty.avi").read_bytes(), 0, 8, 8, 25)
    with pytest.raises(ValueError):
        MjpegWriter(str(tmp_path / "bad.avi"), 8, 8, 0)


# ------------------------------------------------------------------------------------------------------------------------- CLI
def test_demo_and_visualize_switches():
    import demo
    import visualize
    assert demo.parse_args([]).render_format == "png"
    assert demo.parse_args(["--render_dir", "x", "--render_format", "jpg"]).render_format == "jpg"
    with pytest.raises(SystemExit):
        demo.parse_args(["--render_format", "bmp"])
    base = ["--img_path", "a.jpg", "--depth_path", "a.exr", "--pose_path", "a.pkl"]
    a = visualize.parse_args(base)
    assert a.format == "png" and a.output == "render.png" and a.overlay == "overlay.png"
    a = visualize.parse_args(base + ["--format", "jpg"])
    assert a.format == "jpg" and a.output == "render.jpg" and a.overlay == "overlay.jpg"
    a = visualize.parse_args(base + ["--format", "jpg", "--output", "mine.jpeg", "--overlay", ""])
    assert a.output == "mine.jpeg" and a.overlay == ""
    with pytest.raises(SystemExit):
        visualize.parse_args(base + ["--format", "gif"])


def test_run_sequence_switches(capsys):
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    a = run_sequence.build_parser().parse_args(base)
    assert a.render_format == "png" and a.render_video is None and a.render_dir is None and a.render_every == 1
    assert a.render_fps == 25 and a.render_view == "render" and a.render_quality == 90
    a = run_sequence.build_parser().parse_args(base + ["--render_dir", "d", "--render_format", "jpg", "--render_video", "v.avi",
                                                       "--render_fps", "12.5", "--render_view", "both", "--render_quality", "80",
                                                       "--render_every", "3"])
    assert (a.render_format, a.render_video, a.render_fps, a.render_view, a.render_quality, a.render_every) == \
        ("jpg", "v.avi", 12.5, "both", 80, 3)
    for bad in (["--render_format", "bmp"], ["--render_view", "left"], ["--render_quality", "0"], ["--render_quality", "101"],
                ["--render_fps", "0"]):
        with pytest.raises(SystemExit):
            run_sequence.build_parser().parse_args(base + bad)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------------- binding
def test_encoder_refuses_host_tensors():
    with pytest.raises(_lib.HipExtensionError):
        JpegEncoder("cpu")
    enc = JpegEncoder("cuda")                       # touches no device until it encodes
    with pytest.raises(_lib.HipExtensionError):
        enc.encode(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(_lib.HipExtensionError):
        enc.encode(np.zeros((8, 8, 3), dtype=np.uint8))
    with pytest.raises(_lib.HipExtensionError):
        _lib.jpeg_encode(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), *quant_tables(90), 444, 0, torch.zeros((1, 64), dtype=torch.uint8),
                         torch.zeros(1, dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32), torch.zeros(64, dtype=torch.uint8))


def test_scratch_helper_is_pure_host():
    lib = _lib.load()
    n = lib.se_jpeg_encode_scratch_bytes(1, 1024, 1280, 444)
    blocks = 128 * 160 * 3
    assert n >= blocks * (128 + 208) and n < blocks * 400                  # coefficients + worst-case bit buffer, little else
    assert lib.se_jpeg_encode_scratch_bytes(8, 1024, 1280, 444) > 7 * n
    assert 0 < lib.se_jpeg_encode_scratch_bytes(1, 1, 1, 420) < 65536
    for bad in ((0, 8, 8, 444), (1, 0, 8, 444), (1, 8, 8, 422), (1, 8, 70000, 444), (1, 65535, 65535, 444)):
        assert lib.se_jpeg_encode_scratch_bytes(*bad) == -1
    assert _lib.ABI_VERSION >= 29
