"""Device JPEG decode (sceneego_amd/jpeg_device.py, csrc/jpeg.hip) on hand-built files (tests/jpeg_craft_cases.py): byte for byte
PIL's output on every file PIL decodes - singly, in mixed batches of one size beside PIL-written files and a PNG, with and without
the inter-workgroup rounds; the files PIL refuses raise and name the file; a decode is repeated on the host exactly where a case says
so (blocks outside the plain domain of the IDCT, damaged segments) and nowhere else, so the fall-back cannot hide a wrong kernel."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_craft_cases as K  # noqa: E402

from sceneego_amd.jpeg_device import decode_jpeg_batch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEMO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo", "img_001000.jpg")
CASES = K.cases()
GOOD = [c for c in CASES if c.pil]
SIZES = sorted({(c.H, c.W) for c in GOOD})
_REF = {}


def _pil(data):
    from PIL import Image
    if data not in _REF:                       # one reference decode per file, shared by every test
        with Image.open(io.BytesIO(data)) as im:
            rgb = np.asarray(im.convert("RGB"))
        _REF[data] = np.ascontiguousarray(rgb[:, :, ::-1])
        _REF[data].setflags(write=False)
    return _REF[data]


def _enc(arr, fmt="JPEG", **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, fmt, **kw)
    return b.getvalue()


def _decode(datas, **kw):
    """(uint8 [B, H, W, 3] on the host, slots decoded again on the host)."""
    out, st = decode_jpeg_batch(datas, DEV, check=False, **kw)
    st.check()
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.redecoded


def _same(got, datas):
    for i, d in enumerate(datas):
        ref = _pil(d)
        assert got[i].shape == ref.shape
        if not np.array_equal(got[i], ref):
            bad = np.argwhere(got[i] != ref)
            pytest.fail(f"slot {i}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[i][tuple(bad[0])]} != {ref[tuple(bad[0])]}")


def _batch(H, W):
    """Every good case of one size in a fixed order, beside three PIL-written files and a PNG of that size -> (files, slots whose
    decode must be repeated on the host)."""
    rng = np.random.default_rng(H * 1000 + W)
    arr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    datas = [c.data for c in GOOD if (c.H, c.W) == (H, W)]
    again = [i for i, c in enumerate(c for c in GOOD if (c.H, c.W) == (H, W)) if c.status]
    extra = [_enc(arr, quality=90, subsampling=2), _enc(arr, "PNG"), _enc(arr, quality=50, subsampling=0, restart_marker_blocks=1),
             _enc(arr[:, :, 1].copy(), quality=75, optimize=True)]
    for j, e in enumerate(extra):              # spread among the cases: slots 1, 3, 5, 7 where there are that many
        pos = min(2 * j + 1, len(datas))
        datas.insert(pos, e)
        again = [i + 1 if i >= pos else i for i in again]
    return datas, again


@pytest.mark.parametrize("case", GOOD, ids=repr)
def test_single_file_equals_pil(case):
    got, again = _decode([case.data])
    _same(got, [case.data])
    assert again == ([0] if case.status else [])


@pytest.mark.parametrize("rounds", [0, None, 8])
def test_long_segment_over_several_workgroups(rounds):
    data = K.by_name("g6_long_segment").data
    got, again = _decode([data, data], rounds=rounds)
    _same(got, [data, data])
    assert again == []


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_mixed_batch_equals_pil(hw):
    datas, want = _batch(*hw)
    got, again = _decode(datas)
    _same(got, datas)
    assert again == want
    got0, again0 = _decode(datas, rounds=0)
    assert np.array_equal(got0, got) and again0 == want


@pytest.mark.parametrize("name", [c.name for c in CASES if not c.pil])
def test_refused_files_raise_and_recover(name, tmp_path):
    p = tmp_path / (name + ".jpg")
    p.write_bytes(K.by_name(name).data)
    good, _ = _batch(K.H0, K.W0)
    for srcs in ([str(p)], good[:3] + [str(p)] + good[3:5]):
        with pytest.raises((ValueError, OSError), match=name + r"\.jpg") as e:
            decode_jpeg_batch(srcs, DEV)
        assert isinstance(e.value.__cause__, OSError)           # PIL's own error
    torch.cuda.synchronize()
    got, _ = _decode(good)
    _same(got, good)


def test_host_decode_only_where_a_case_says_so():
    """Group 7 (blocks outside the plain domain) and the two damaged files come back through PIL; nothing else does: not the other
    groups, not the noisiest files PIL writes, not the demo frame."""
    for c in GOOD:
        if c.group == 7:
            assert c.status == 4
    same = [c for c in GOOD if (c.H, c.W) == (K.H0, K.W0)]
    got, again = _decode([c.data for c in same])
    _same(got, [c.data for c in same])
    assert [same[i].name for i in again] == [c.name for c in same if c.status]
    assert {same[i].name for i in again} >= {c.name for c in GOOD if c.group == 7}
    worst = []
    for kind in ("uniform", "binary"):
        for quality in (1, 5, 100):
            for sub in (0, 2):
                rng = np.random.default_rng(quality + sub)
                arr = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8) if kind == "uniform" else \
                    (rng.integers(0, 2, (64, 96, 3)) * 255).astype(np.uint8)
                worst.append(_enc(arr, quality=quality, subsampling=sub))
    got, again = _decode(worst)
    _same(got, worst)
    assert again == []
    got, again = _decode([DEMO])
    from sceneego_amd.preprocess import load_image_bgr
    assert np.array_equal(got[0], load_image_bgr(DEMO)) and again == []


def test_status_is_kept_and_reported():
    """The status vector itself: 4 with a block of the segment for a block outside the plain domain, the write kernel's own code
    where a segment is damaged (the IDCT kernel does not overwrite it), 0 everywhere else."""
    names = ["g7_c", "g8_short_segment", "g8_all_ones_segment", "g8_junk_after_segment", "g4_inside_c", "g7_mixed_420"]
    out, st = decode_jpeg_batch([K.by_name(n).data for n in names], DEV, check=False)
    s = st.status.cpu().numpy()
    rows = {n: [] for n in names}
    for (_, si, _, _, slot), row in zip(st._segs, s):
        rows[names[slot]].append((si, int(row[0]), int(row[1])))
    assert [r[1] for r in rows["g7_c"]] == [4] and rows["g7_c"][0][2] in K.by_name("g7_c").classes
    assert [r[1] for r in rows["g8_short_segment"]] == [0, 0, 3, 0, 0, 0]
    assert [r[1] for r in rows["g8_all_ones_segment"]] == [0, 0, 2, 0, 0, 0]
    assert all(r[1] == 0 for r in rows["g8_junk_after_segment"] + rows["g4_inside_c"])
    assert [r[1] for r in rows["g7_mixed_420"]] == [4] and rows["g7_mixed_420"][0][2] in K.by_name("g7_mixed_420").classes
    st.check()
    assert st.redecoded == [0, 1, 2, 5]
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), [K.by_name(n).data for n in names])


def test_repeatable_and_streams():
    datas, want = _batch(K.H0, K.W0)
    a, ra = _decode(datas)
    b, rb = _decode(datas)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c, rc = _decode(datas)
    s.synchronize()
    assert np.array_equal(a, b) and np.array_equal(a, c) and ra == rb == rc == want
    _same(a, datas)
