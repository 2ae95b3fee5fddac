"""Hand-built JPEG files (tests/jpeg_craft.py, tests/jpeg_craft_cases.py) on the host: the parser's classification of every case, the
numpy model of csrc/jpeg.hip (tests/jpeg_model.py) against PIL on every case the device path takes, what PIL does with the damaged
files, the plain-block predicate against PIL over a sweep of crafted blocks, and the margin ordinary files keep from its bounds."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_craft as C  # noqa: E402
import jpeg_craft_cases as K  # noqa: E402
import jpeg_model as M  # noqa: E402

from sceneego_amd.jpeg_device import HostDecodeError, HuffTable, JpegFile, parse  # noqa: E402

CASES = K.cases()


def _pil(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


def _enc(arr, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", **kw)
    return b.getvalue()


# ------------------------------------------------------------------------------------------------------------------ the writer
def test_canonical_tables_are_valid_and_long():
    for bits, vals in (K.DC16, K.DC12_LONG, K.AC10, K.AC16, K.AC_SPREAD, K.DC_SPREAD):
        HuffTable(bits, vals, len(vals) <= 16, "table")          # libjpeg's check: raises on an oversubscribed table
        codes = C.code_table(bits, vals)
        assert len(codes) == len(vals) == sum(bits)
        longest = max(ln for _, ln in codes.values())
        assert all(code != (1 << ln) - 1 for code, ln in codes.values() if ln == longest)        # the all-ones code stays free
    assert K.DC16[0][4] == 16 and sum(K.DC16[0]) == 16                        # a complete 16-symbol table needs 5-bit codes
    assert min(ln for _, ln in C.code_table(*K.AC10).values()) == 10 and len(K.AC10[1]) == 162
    assert min(ln for _, ln in C.code_table(*K.DC12_LONG).values()) == 12
    assert {ln for _, ln in C.code_table(*K.AC16).values()} == {16}
    assert {ln for _, ln in C.code_table(*K.AC_SPREAD).values()} == set(range(10, 17))
    with pytest.raises(ValueError):
        C.canonical_table(list(range(8)) * 2)


def test_writer_round_trip_through_the_model():
    """What the writer is given is what the model's entropy decode returns: coefficients, tables, quantisation, segments."""
    rng = np.random.default_rng(1)
    comps = K.YCC["420"]
    coefs = K.rand_coefs(rng, K.H0, K.W0, comps)
    quant = K.rand_quant(rng, (0, 1))
    f = JpegFile(C.write_jpeg(K.H0, K.W0, comps, coefs, quant, restart=5, dht=K.LONG_TABLES, rst_fill=2, pad_ones=False))
    assert f.device and (f.H, f.W, f.mcus_x, f.mcus_y, f.restart) == (K.H0, K.W0, 4, 3, 5)
    assert [s[:2] for s in f.segments] == [(0, 5), (5, 5), (10, 2)]
    got = M.file_coefficients(f)
    for m in range(12):
        r, c = divmod(m, 4)
        want = [coefs[0][2 * r, 2 * c], coefs[0][2 * r, 2 * c + 1], coefs[0][2 * r + 1, 2 * c], coefs[0][2 * r + 1, 2 * c + 1],
                coefs[1][r, c], coefs[2][r, c]]
        np.testing.assert_array_equal(got[6 * m:6 * m + 6], np.stack(want))
    np.testing.assert_array_equal(f.quant[0], quant[0][0])
    np.testing.assert_array_equal(f.quant[2], quant[1][0])


# ------------------------------------------------------------------------------------------------------------------ the cases
def test_case_list_covers_the_groups():
    assert {c.group for c in CASES} == set(range(1, 9))
    assert all(max(c.H, c.W) <= 56 or c.name in ("g6_long_segment", "g4_dc_wrap_workgroup") for c in CASES)
    long = K.by_name("g6_long_segment")
    f = JpegFile(long.data)
    assert len(f.segments) == 1 and len(f.segments[0][2]) > 8192 and len(f.segments[0][2]) * 8 > 2 * 256 * 128
    chroma_w = {(c.name, -(-c.W // 2)) for c in CASES if c.group == 1 and "19x37" not in c.name}
    assert {w for _, w in chroma_w} == {1, 2, 3}
    # both paths of the DC kernel: at most 64 blocks of a component in the segment, and more
    assert JpegFile(K.by_name("g4_dc_wrap_thread").data).mcus_x * 4 <= 64 < JpegFile(K.by_name("g4_dc_wrap_workgroup").data).mcus_x * 4


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_classification(case):
    if case.path == "host":
        f = JpegFile(case.data)
        assert not f.device and case.why in f.why, f.why
    else:
        assert JpegFile(case.data).device


@pytest.mark.parametrize("case", [c for c in CASES if c.path == "device" and c.status in (None, 4)], ids=repr)
def test_model_equals_pil(case):
    f = JpegFile(case.data)
    got, ref = M.decode(f), _pil(case.data)
    plain = M.file_plain(f)
    if case.status is None:
        assert plain.all(), np.flatnonzero(~plain)
        np.testing.assert_array_equal(got, ref)
        return
    # group 7: exactly the marked blocks leave the plain domain, each by the class the case names
    a, b, c = M.file_classes(f)
    first = {int(i): ("a" if not a[i] else "b" if not b[i] else "c") for i in np.flatnonzero(~plain)}
    assert first == case.classes
    bad = np.argwhere(got != ref)
    print(f"{case.name}: {len(bad)} bytes of the C-code model differ from PIL")
    # whatever PIL's IDCT does there, every plain block around them is equal (gray: 7 blocks per row)
    if len(f.comps) == 1:
        blk = (bad[:, 0] // 8) * f.mcus_x + bad[:, 1] // 8
        assert set(blk.tolist()) <= set(case.classes)


def test_dc_predictor_passes_16_bits():
    for name in ("g4_dc_wrap_thread", "g4_dc_wrap_workgroup"):
        f = JpegFile(K.by_name(name).data)
        diffs = M.decode_segment(f, f.segments[0][2], f.mcus_x * 6)[0][:, 0].astype(np.int64)
        luma = np.array([i % 6 < 4 for i in range(len(diffs))])
        run = np.cumsum(diffs[luma])
        assert run.max() > 65536 and run.min() < -65536
        stored = M.file_coefficients(f)[:, 0][luma]
        assert np.abs(stored[M.file_real(f)[luma]]).max() <= 200 and np.abs(stored).max() > 30000


def test_overruns_land_on_coefficient_63():
    f = JpegFile(K.by_name("g4_overrun").data)
    coef = M.file_coefficients(f)
    assert coef[1, 63] == 7 and coef[1 * 7 + 3, 63] == -9 and coef[1 * 7 + 3, C.ZIGZAG[59]] == 3
    assert coef[2 * 7, 1] == 5 and np.count_nonzero(coef[2 * 7, 1:]) == 1 and coef[-1, 63] == -4


def test_damaged_files():
    """What PIL makes of the damaged files, and what the device path will: a status (and PIL again), nothing, or PIL's error."""
    for name, text in (("g8_short_segment", "end"), ("g8_all_ones_segment", "no code")):
        case = K.by_name(name)
        f = JpegFile(case.data)
        assert f.device and _pil(case.data).shape == (K.H0, K.W0, 3)
        with pytest.raises(ValueError, match=text):
            M.decode(f)
    for case in CASES:
        if not case.pil:
            with pytest.raises(OSError):
                _pil(case.data)
            with pytest.raises(HostDecodeError, match=r"<bytes #1>: .*" + case.why) as e:
                parse([K.by_name("g1_420_5x3").data, case.data])
            assert isinstance(e.value, ValueError) and isinstance(e.value, OSError) and isinstance(e.value.__cause__, OSError)


def test_host_error_names_the_file(tmp_path):
    p = tmp_path / "cut.jpg"
    p.write_bytes(K.by_name("g8_cut_in_half").data)
    with pytest.raises(ValueError, match="cut.jpg.*stream ended"):
        parse([str(p)])
    q = tmp_path / "noeoi.jpg"
    q.write_bytes(K.by_name("g8_no_eoi").data)
    with pytest.raises(OSError, match="noeoi.jpg.*truncated"):
        parse([str(q)])


def test_status_check_decodes_again_or_raises():
    """``DecodeStatus.check`` on host tensors: a file with a status is decoded by PIL into its slot and listed; where PIL refuses it
    too, the status raises as before, chained from PIL's error; a later segment of a file already decoded again changes nothing."""
    import torch

    from sceneego_amd.jpeg_device import DecodeStatus

    class Stub:
        def __init__(self, img=None):
            self.img = img

        def host_decode(self):
            if self.img is None:
                raise OSError("image file is truncated")
            return self.img

    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    segs = [("a.jpg", 0, 12, 1, 0), ("b.jpg", 0, 6, 2, 1), ("b.jpg", 1, 6, 2, 1), ("c.jpg", 0, 12, 1, 2)]
    out = torch.zeros((3, 2, 3, 3), dtype=torch.uint8)
    st = DecodeStatus(torch.tensor([[0, 0], [4, 1], [3, 2], [0, 0]], dtype=torch.int32), segs, [Stub(), Stub(img), Stub()], out)
    st.check()
    assert st.redecoded == [1] and np.array_equal(out[1].numpy(), img) and not out[0].any() and not out[2].any()
    st = DecodeStatus(torch.tensor([[0, 0], [0, 0], [3, 2], [2, 77]], dtype=torch.int32), segs, [Stub(), Stub(img), Stub()], out)
    with pytest.raises(ValueError, match=r"^c\.jpg: no code matches at bit 77$") as e:
        st.check()
    assert isinstance(e.value.__cause__, OSError) and st.redecoded == [1]
    st = DecodeStatus(torch.tensor([[3, 5], [0, 0], [0, 0], [0, 0]], dtype=torch.int32), segs, [Stub(), Stub(img), Stub()], out)
    with pytest.raises(ValueError, match=r"^a\.jpg: stream ended after 5 of 12 blocks$"):
        st.check()
    st = DecodeStatus(torch.tensor([[1, 0], [0, 0], [0, 0], [0, 0]], dtype=torch.int32), segs, [Stub(img), Stub(img), Stub(img)], out)
    with pytest.raises(ValueError, match=r"^a\.jpg: descriptor out of range$"):        # never handed to PIL: not the file's fault
        st.check()
    assert st.redecoded == []
    st = DecodeStatus(torch.tensor([[0, 0], [0, 0], [2, 9], [0, 0]], dtype=torch.int32), segs, [Stub(), Stub(), Stub()], out)
    with pytest.raises(ValueError, match=r"^b\.jpg: restart segment 1: no code matches at bit 9$"):
        st.check()


# ------------------------------------------------------------------------------------------------------------------ the predicate
def _sweep_file(rng, amp_log2, flat):
    """A gray 4 x 6-block file: coefficients of magnitude up to 2^amp_log2 at a random density, a flat or a random quantisation."""
    n = 24
    dens = rng.choice([0.05, 0.2, 0.5])
    amp = 1 << amp_log2
    a = rng.integers(-amp, amp + 1, (4, 6, 64)) * (rng.random((4, 6, 64)) < dens)
    a[:, :, 0] = rng.integers(-amp, amp + 1, (4, 6))
    a = np.clip(a, -32767, 32767)
    q = np.full(64, rng.choice([1, 2, 8])) if flat else rng.integers(1, 1 << rng.integers(1, 8), 64)
    dht = [((0, 0), K.DC16), ((1, 0), C.canonical_table([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 16)], 8))]
    return C.write_jpeg(32, 48, K.GRAY, [a], {0: (q, False)}, dht=dht), n


def test_plain_blocks_equal_pil_over_a_sweep():
    """Seeded crafted blocks with amplitudes 2^0 .. 2^12: every block the predicate calls plain equals PIL; how many of the others
    differ is printed, not asserted (it depends on whether this machine's libjpeg-turbo runs its SIMD IDCT)."""
    rng = np.random.default_rng(2024)
    n_plain = n_other = plain_diff = other_diff = 0
    for i in range(260):
        data, n = _sweep_file(rng, i % 13, flat=bool((i // 13) & 1))
        f = JpegFile(data)
        assert f.device
        got, ref = M.decode(f)[:, :, 0], _pil(data)[:, :, 0]
        plain = M.file_plain(f)
        differs = (got != ref).reshape(4, 8, 6, 8).any(axis=(1, 3)).reshape(-1)
        n_plain += int(plain.sum())
        n_other += int((~plain).sum())
        plain_diff += int((differs & plain).sum())
        other_diff += int((differs & ~plain).sum())
    print(f"sweep: {n_plain} plain blocks, {plain_diff} differ from PIL; {n_other} other blocks, {other_diff} differ")
    assert n_plain + n_other >= 5000 and n_plain >= 1500 and n_other >= 1500
    assert plain_diff == 0


@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("quality", [1, 5, 100])
@pytest.mark.parametrize("kind", ["uniform", "binary"])
def test_ordinary_files_are_plain(kind, quality, sub):
    """PIL-encoded noise, the worst an ordinary encoder produces, stays inside the plain domain: no host decode for such files."""
    rng = np.random.default_rng(quality + sub)
    arr = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8) if kind == "uniform" else (rng.integers(0, 2, (64, 96, 3)) * 255).astype(np.uint8)
    f = JpegFile(_enc(arr, quality=quality, subsampling=sub))
    assert f.device and all(x.all() for x in M.file_classes(f))
