"""CPU: the test-side ZIP / ZIPS / NONE cases round-trip through exr.py and cover what they claim; the device decoder's host part
builds their descriptors and rejects malformed offset tables, chunk sizes, first rows and zlib headers before anything is launched;
se_exr_zip_scratch_bytes lays out the scratch slices as include/sceneego_hip.h documents."""
import struct

import numpy as np
import pytest

import exr_piz_writer as W
import exr_zip_cases as Z
from sceneego_amd import _lib, exr, exr_device

CASES = Z.make_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_round_trip_through_exr_py(name):
    buf, chans, _what, _info = CASES[name]
    planes = exr.read_exr_buffer(buf)
    exp = W.expected_planes(chans)
    assert sorted(planes) == sorted(exp)
    for k in exp:
        assert np.array_equal(planes[k].view(np.int32), exp[k].view(np.int32)), k


def _types(name):
    buf, _, _, info = CASES[name]
    out = []
    for (_, blk), inf in zip(Z.chunks(buf), info):
        if not inf["stored"]:
            out.append(Z.block_types(blk))
    return out


def test_cases_cover_what_they_claim():
    flat = lambda name: [t for ts in _types(name) for t in ts]                             # noqa: E731
    assert set(flat("zip_fixed")) == {1} and 2 in flat("zip_level9") and 2 in flat("zip_odd_window")
    stored = [t for t in flat("zip_level0_sync") if isinstance(t, tuple)]
    assert stored and all(t[0] == 0 for t in stored) and any(t[1] == 0 for t in stored)       # empty stored blocks
    assert all(len(ts) > 1 for ts in _types("zip_level0_sync"))
    assert all(len(ts) > 2 for ts in _types("zip_sync_flush")) and (0, 0) in flat("zip_full_flush")
    assert sum(isinstance(t, tuple) and t[1] > 0 for t in _types("zip_wide_level0")[0]) >= 3      # several stored blocks
    assert sorted({i["cinfo"] for i in CASES["zip_cinfo"][3]}) == list(range(8))
    assert [i["stored"] for i in CASES["zip_stored_chunk"][3]] == [False, True, False]
    assert all(i["stored"] for i in CASES["none_odd_window"][3]) and not any(i["stored"] for i in CASES["zip_odd_window"][3])
    assert max(i["size"] for i in CASES["zip_wide_level0"][3]) > 320_000                        # a chunk far beyond LDS
    hdr = exr._parse_header(CASES["zips_odd_window"][0])
    assert hdr["window"] == (5, -3, 337, 73) and hdr["compression"] == 2 and len(CASES["zips_odd_window"][3]) == 77
    d = CASES["zip_odd_window"][1]["Y"][1]
    assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any()
    assert exr._parse_header(CASES["zip_1px"][0])["window"][2] == 0


def test_file_descriptors():
    f = exr_device._File(CASES["zip_odd_window"][0], 0)
    assert not f.piz and f.chan == (333, 77, 1, 0, 1, 1, 0, 0)
    assert [r[3] for r in f.rows] == [0, 16, 32, 48, 64] and [r[4] for r in f.rows] == [16, 16, 16, 16, 13]
    assert all(r[5] == 0 for r in f.rows)
    assert [r[1] for r in f.rows] == [i["size"] for i in CASES["zip_odd_window"][3]]
    f = exr_device._File(CASES["zip_multi_float"][0], 3)
    assert f.chan == (70, 35, 2, 1, 2, 6, 0, 0) and f.name == "<bytes #3>"                  # B after A: 1 word before it
    f = exr_device._File(CASES["zips_uint"][0], 0)
    assert f.chan[2:6] == (0, 0, 2, 4) and len(f.rows) == 35 and all(r[4] == 1 for r in f.rows)
    f = exr_device._File(CASES["none_odd_window"][0], 0)
    assert len(f.rows) == 77 and all(r[5] == 1 for r in f.rows)
    f = exr_device._File(CASES["zip_stored_chunk"][0], 0)
    assert [r[5] for r in f.rows] == [0, 1, 0]
    buf = CASES["zip_odd_window"][0]
    _, blk = Z.chunks(buf)[2]
    g = exr_device._File(buf, 0)
    assert buf[g.rows[2][0]:g.rows[2][0] + g.rows[2][1]] == blk


# ------------------------------------------------------------------------------------------------------------------------------
# validation: ValueError before any device call
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device call was made")
    for fn in ("exr_piz_decode", "exr_piz_scratch_bytes", "exr_zip_decode", "exr_zip_scratch_bytes"):
        monkeypatch.setattr(_lib, fn, boom)


def _offsets(buf):
    hdr = exr._parse_header(buf)
    H = hdr["window"][3] - hdr["window"][1] + 1
    lpc = exr._LINES_PER_CHUNK[hdr["compression"]]
    n = (H + lpc - 1) // lpc
    return hdr["data_start"], list(struct.unpack_from(f"<{n}Q", buf, hdr["data_start"]))


@pytest.mark.parametrize("name", ["zip_odd_window", "zips_odd_window", "none_odd_window"])
def test_rejects_offset_outside_file(no_device, name):
    buf = bytearray(CASES[name][0])
    start, _ = _offsets(buf)
    struct.pack_into("<Q", buf, start + 8, len(buf) + 100)
    with pytest.raises(ValueError, match=r"<bytes #1>: chunk 1: offset"):
        exr_device.decode_depth_exr_batch([CASES["zip_level1"][0], bytes(buf)], "cuda", out_hw=(8, 8))


def test_rejects_offset_into_header(no_device):
    buf = bytearray(CASES["zips_odd_window"][0])
    start, _ = _offsets(buf)
    struct.pack_into("<Q", buf, start + 8 * 4, 8)
    with pytest.raises(ValueError, match="chunk 4: offset 8 outside"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


def test_rejects_chunk_size_past_end(no_device):
    buf = bytearray(CASES["zip_odd_window"][0])
    _, offs = _offsets(buf)
    struct.pack_into("<i", buf, offs[2] + 4, 10 ** 6)
    with pytest.raises(ValueError, match="chunk 2: .* run past the end"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


def test_rejects_short_none_chunk(no_device):
    buf = bytearray(CASES["none_odd_window"][0])
    _, offs = _offsets(buf)
    struct.pack_into("<i", buf, offs[6] + 4, 100)
    with pytest.raises(ValueError, match="chunk 6: 100 bytes hold less than its 666 bytes"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


@pytest.mark.parametrize("name", ["zip_odd_window", "zips_odd_window"])
def test_rejects_wrong_first_row(no_device, name):
    buf = bytearray(CASES[name][0])
    _, offs = _offsets(buf)
    struct.pack_into("<i", buf, offs[3], 999)
    with pytest.raises(ValueError, match="chunk 3: first row 999, expected"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


@pytest.mark.parametrize("hdr2,why", [(b"\x79\x9c", "CM"), (b"\x88\x98", "CINFO"), (b"\x78\x9d", "FCHECK"), (b"\x78\xbb", "FDICT")])
def test_rejects_bad_zlib_header(no_device, hdr2, why):
    buf = bytearray(CASES["zip_odd_window"][0])
    _, offs = _offsets(buf)
    if why == "CINFO":
        assert ((hdr2[0] << 8) | hdr2[1]) % 31 == 0
    if why == "FDICT":
        assert ((hdr2[0] << 8) | hdr2[1]) % 31 == 0 and hdr2[1] & 32
    buf[offs[1] + 8:offs[1] + 10] = hdr2
    with pytest.raises(ValueError, match=r"<bytes #0>: chunk 1: bad zlib header"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


def test_rejects_chunk_too_short_for_zlib(no_device):
    buf = Z.write_zip_exr(CASES["zip_level1"][1], override={2: b"\x78"})
    with pytest.raises(ValueError, match="chunk 2: 1 bytes cannot hold a zlib stream"):
        exr_device.decode_depth_exr_batch([buf], "cuda")


def test_unsupported_files_raise_what_exr_py_raises(no_device):
    buf = bytearray(CASES["zips_odd_window"][0])                                 # 1 line per chunk, as RLE
    i = buf.index(b"compression\0compression\0") + len(b"compression\0compression\0") + 4
    for comp in (6, 8):                                                          # B44, DWAA
        buf[i] = comp
        with pytest.raises(NotImplementedError, match=f"EXR compression {comp} is not supported"):
            exr.read_exr_buffer(bytes(buf))
        with pytest.raises(NotImplementedError, match=f"EXR compression {comp} is not supported"):
            exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")
    buf[i] = 1                                                                   # RLE with chunks that are not stored
    with pytest.raises(NotImplementedError, match="RLE"):
        exr.read_exr_buffer(bytes(buf))
    with pytest.raises(NotImplementedError, match="RLE"):
        exr_device.decode_depth_exr_batch([bytes(buf)], "cuda")


def test_zip_scratch_layout():
    """se_exr_zip_scratch_bytes (host): every compressed chunk gets a 16-byte aligned slice of bytes_per_line * rows bytes, stored
    chunks none."""
    f = exr_device._File(CASES["zip_stored_chunk"][0], 0)
    g = exr_device._File(CASES["zip_odd_window"][0], 1)
    desc = np.array(f.rows + g.rows, dtype=np.int64)
    desc[len(f.rows):, 2] = 1
    chan = np.array([f.chan, g.chan], dtype=np.int32)
    total = _lib.exr_zip_scratch_bytes(desc, chan)
    off, cap = desc[:, 13], desc[:, 14]
    bpl = np.where(desc[:, 2] == 0, 2 * 96, 2 * 333)
    assert (cap == np.where(desc[:, 5] == 1, 0, bpl * desc[:, 4])).all()
    assert (off % 16 == 0).all() and off[0] == 0
    assert (off[1:] >= off[:-1] + cap[:-1]).all() and total >= off[-1] + cap[-1]
    assert total == sum((int(c) + 15) // 16 * 16 for c in cap)
    bad = desc.copy()
    bad[0, 2] = 5                                                                # file index out of range
    with pytest.raises(_lib.HipExtensionError):
        _lib.exr_zip_scratch_bytes(bad, chan)
