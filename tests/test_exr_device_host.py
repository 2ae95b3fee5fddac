"""CPU: the test-side PIZ writer round-trips through exr.py on every case the device decoder is tested on; the device decoder's host
part rejects malformed files before anything is launched; run_sequence.py builds TestDataset's frame list."""
import json
import os
import pickle
import struct

import numpy as np
import pytest

import exr_piz_writer as W
from conftest import GOLD
from sceneego_amd import _lib, exr, exr_device

CASES = W.make_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_writer_round_trip_through_exr_py(name):
    buf, chans, _what, _stats = CASES[name]
    planes = exr.read_exr_buffer(buf)
    exp = W.expected_planes(chans)
    assert sorted(planes) == sorted(exp)
    for k in exp:
        assert np.array_equal(planes[k].view(np.int32), exp[k].view(np.int32)), k


def test_cases_cover_what_they_claim():
    st = {k: v[3] for k, v in CASES.items()}
    assert st["w16"]["w16"] > 0                                  # max_value >= 2^14 -> wdec16
    assert st["skew58"]["max_len"] == 58                          # a 58-bit code in the bitstream
    assert st["stored"]["stored"] == 1 and st["skew58"]["stored"] == 0 and st["uint"]["stored"] == 0
    assert st["runs"]["max_run"] > 255 and st["odd_window"]["max_run"] > 255
    d = CASES["odd_window"][1]["Y"][1]
    assert np.isnan(d).any() and np.isposinf(d).any() and (d[np.isfinite(d)] > 10).any()
    assert exr._parse_header(CASES["odd_window"][0])["window"] == (5, -3, 337, 73)        # 77 rows: 32 + 32 + 13
    assert exr.depth_channel(exr.read_exr_buffer(CASES["bgr_z"][0])) is not None
    f = exr_device._File(CASES["bgr_z"][0], 0)
    assert f.chan[2:6] == (1, 0, 1, 5)                            # B (HALF) picked, first plane of B, G, R, Z(FLOAT)
    f = exr_device._File(CASES["a_y"][0], 0)
    assert f.chan[2:6] == (1, 1, 1, 2)                            # Y after A


@pytest.mark.parametrize("comp", ["zip", "none"])
def test_writer_zip_and_none_round_trip(comp):
    chans = CASES["odd_window"][1]
    buf = W.write_exr(chans, compression=comp, window=(5, -3))
    assert np.array_equal(exr.read_exr_buffer(buf)["Y"].view(np.int32), W.expected_planes(chans)["Y"].view(np.int32))


def test_demo_fixtures_parse_as_piz():
    for n in ("img_001000", "img_001796", "img_002376"):
        f = exr_device._File(os.path.join(GOLD, "demo", n + ".jpg.exr"), 0)
        assert f.piz and (f.H, f.W) == (512, 640) and len(f.rows) == 16 and f.chan[2:6] == (1, 0, 1, 1)
        assert all(r[5] == 0 and r[9] > 20 for r in f.rows)


# ------------------------------------------------------------------------------------------------------------------------------
# validation: ValueError before any device call
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "exr_piz_decode", boom)
    monkeypatch.setattr(_lib, "exr_piz_scratch_bytes", boom)


def _chunk_offsets(buf):
    hdr = exr._parse_header(buf)
    H = hdr["window"][3] - hdr["window"][1] + 1
    n = (H + 31) // 32
    return hdr["data_start"], list(struct.unpack_from(f"<{n}Q", buf, hdr["data_start"]))


def _huf_fields(buf, off):
    """Byte position of the Huffman header (im, iM, tableLength, nBits) of the PIZ chunk at file offset `off`."""
    mn, mx = struct.unpack_from("<HH", buf, off + 8)
    p = off + 8 + 4 + (mx - mn + 1 if mn <= mx else 0)
    return p + 4


def test_rejects_offset_outside_file(no_device):
    buf = bytearray(CASES["odd_window"][0])
    start, offs = _chunk_offsets(buf)
    struct.pack_into("<Q", buf, start + 8, len(buf) + 100)
    with pytest.raises(ValueError, match="chunk 1: offset"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


def test_rejects_offset_into_header(no_device):
    buf = bytearray(CASES["odd_window"][0])
    start, _ = _chunk_offsets(buf)
    struct.pack_into("<Q", buf, start, 8)
    with pytest.raises(ValueError, match="chunk 0: offset 8 outside"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


def test_rejects_chunk_size_past_end(no_device):
    buf = bytearray(CASES["odd_window"][0])
    _, offs = _chunk_offsets(buf)
    struct.pack_into("<i", buf, offs[2] + 4, 10 ** 6)
    with pytest.raises(ValueError, match="chunk 2: .* run past the end"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


def test_rejects_oversized_nbits(no_device):
    buf = bytearray(open(os.path.join(GOLD, "demo", "img_001796.jpg.exr"), "rb").read())
    _, offs = _chunk_offsets(buf)
    p = _huf_fields(buf, offs[3])
    struct.pack_into("<I", buf, p + 12, 8 * 10 ** 6)
    with pytest.raises(ValueError, match=r"<bytes #1>: chunk 3: nBits 8000000 exceeds"):
        exr_device.decode_depth_exr_batch([CASES["odd_window"][0], bytes(buf)], "cuda", out_hw=(64, 64))


def test_rejects_bad_symbol_range(no_device):
    buf = bytearray(CASES["runs"][0])
    _, offs = _chunk_offsets(buf)
    p = _huf_fields(buf, offs[0])
    struct.pack_into("<I", buf, p + 4, 70000)
    with pytest.raises(ValueError, match="chunk 0: symbol range"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


def test_rejects_mismatched_batch_shapes(no_device):
    a = os.path.join(GOLD, "demo", "img_001000.jpg.exr")
    with pytest.raises(ValueError, match="different sizes"):
        exr_device.decode_depth_exr_batch([a, CASES["odd_window"][0]], "cuda")


def test_rejects_cpu_device():
    with pytest.raises(_lib.HipExtensionError):
        exr_device.decode_depth_exr_batch([CASES["runs"][0]], "cpu")


# ------------------------------------------------------------------------------------------------------------------------------
# run_sequence.py: TestDataset.get_gt_data
# ------------------------------------------------------------------------------------------------------------------------------
def _tree(tmp_path, layout):
    base = tmp_path / "seq"
    (base / "imgs").mkdir(parents=True)
    with open(base / "syn.json", "w") as f:
        json.dump({"ego": 100, "ext": 10}, f)
    items = []
    for ext_id in range(10, 17):
        pose = None if ext_id == 12 else np.full((15, 3), ext_id, dtype=np.float32)
        items.append({"ext_id": ext_id, "ego_pose_gt": pose})
    with open(base / "local_pose_gt.pkl", "wb") as f:
        pickle.dump(items, f)
    for ext_id in range(10, 17):
        if ext_id == 15:
            continue                                               # image missing
        (base / "imgs" / ("img_%06d.jpg" % (ext_id + 90))).write_bytes(b"")
    return tmp_path


@pytest.mark.parametrize("layout", ["estimated", "rendered"])
def test_frame_list(tmp_path, layout):
    import run_sequence
    root = _tree(tmp_path, layout)
    name = "est_depth" if layout == "estimated" else None
    images, poses, depths = run_sequence.frame_list(str(root), "seq", name)
    ids = [100, 101, 103, 104, 106]                                # ext 12 has no pose, ext 15 no image
    assert [os.path.basename(p) for p in images] == ["img_%06d.jpg" % i for i in ids]
    assert [float(p[0, 0]) for p in poses] == [i - 90 for i in ids]
    if layout == "estimated":
        assert depths == [str(root / "seq" / "est_depth" / ("img_%06d.jpg.exr" % i)) for i in ids]
    else:
        assert depths == [str(root / "seq" / "rendered" / "depths" / ("img_%06d" % i) / "Image0001.exr") for i in ids]



def test_scratch_layout_is_aligned_and_sized():
    """se_exr_piz_scratch_bytes (host): every chunk's scratch slice starts 16-byte aligned and holds its plane words and 2 x cap
    records; cap bounds the code-length records a table of that many bytes can hold."""
    f = exr_device._File(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), 0)
    g = exr_device._File(CASES["float_z"][0], 1)
    desc = np.array(f.rows + g.rows, dtype=np.int64)
    desc[len(f.rows):, 2] = 1
    chan = np.array([f.chan, g.chan], dtype=np.int32)
    total = _lib.exr_piz_scratch_bytes(desc, chan)
    off, cap = desc[:, 13], desc[:, 14]
    assert (off % 16 == 0).all() and off[0] == 0
    words = np.where(desc[:, 2] == 0, 640, 2 * 96) * desc[:, 4]
    need = ((2 * words + 15) // 16) * 16 + 8 * cap
    assert (off[1:] >= off[:-1] + need[:-1]).all() and total >= off[-1] + need[-1]
    piz = desc[:, 5] == 0
    assert (cap[piz] == np.minimum(desc[piz, 11] - desc[piz, 10] + 1, 8 * (desc[piz, 9] - 20) // 6 + 1)).all()
    assert (cap[~piz] == 0).all()
