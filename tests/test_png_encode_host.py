"""CPU: the numpy model of the PNG encoder (tests/png_encode_model.py) against PIL, zlib and brute force on the case list of
tests/png_encode_cases.py; what each case is there for; the encoder's argument errors, the command-line switches and the binding.
No GPU."""
import zlib

import numpy as np
import pytest
import torch

import png_encode_cases as C
import png_encode_model as M
from sceneego_amd import _lib
from sceneego_amd.png_encode import PngEncoder, png_file, save_png_device

CASE_IDS = [c.name for c in C.CASES]


def _f(name):
    return M.filter_stream(C.BY_NAME[name].image)


def _tokens(name):
    return [t for seg in C.model_file(name)[1] for t in seg["tokens"]]


def _matches(name):
    return [t for t in _tokens(name) if isinstance(t, tuple)]


# ------------------------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", CASE_IDS)
def test_pil_reads_the_input_back(name):
    c = C.BY_NAME[name]
    pixels, mode = C.pil_decode(C.model_file(name)[0])
    assert mode == ("RGB" if c.channels == 3 else "L")
    assert pixels.shape == c.image.shape and np.array_equal(pixels, c.image)


@pytest.mark.parametrize("name", CASE_IDS)
def test_zlib_inflates_the_filtered_stream_and_the_bound_holds(name):
    f, _ = _f(name)
    idat = M.idat_of(C.model_file(name)[0])
    assert idat[:2] == b"\x78\x01"
    assert zlib.decompress(idat) == f.tobytes()                       # the Adler-32 is checked by zlib
    assert len(idat) <= M.zlib_bound(len(f))
    assert M.zlib_bound(len(f)) == 2 + len(f) + 10 * -(-len(f) // M.SEG) + 4


def _brute_force_filter_types(image):
    """Filter per row by plain loops over pixels, sharing nothing with the model's array arithmetic."""
    img = image.astype(int)
    h, w = img.shape[:2]
    bpp = 1 if img.ndim == 2 else 3
    rows = img.reshape(h, w * bpp)
    types = []
    for y in range(h):
        sums = [0] * 5
        for x in range(w * bpp):
            a = rows[y][x - bpp] if x >= bpp else 0
            b = rows[y - 1][x] if y else 0
            c = rows[y - 1][x - bpp] if y and x >= bpp else 0
            p = a + b - c
            paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else (b if abs(p - b) <= abs(p - c) else c)
            for t, pred in enumerate((0, a, b, (a + b) // 2, paeth)):
                v = (rows[y][x] - pred) % 256
                sums[t] += min(v, 256 - v)
        types.append((sums.index(min(sums)), sums))
    return types


@pytest.mark.parametrize("name", CASE_IDS)
def test_filter_bytes_equal_a_brute_force_choice(name):
    c = C.BY_NAME[name]
    f, types = _f(name)
    r = 1 + c.image.shape[1] * c.channels
    assert f[::r].tolist() == types.tolist()
    assert [t for t, _ in _brute_force_filter_types(c.image)] == types.tolist()


@pytest.mark.parametrize("name", CASE_IDS)
def test_chosen_block_is_the_smallest_of_three_real_encodings(name):
    """Each segment is written in all three forms; raw inflate accepts each and returns the segment, so their lengths are the lengths
    of valid encodings.  The arithmetic counts the choice is made from equal them, and the choice is the smallest (ties: stored,
    fixed, dynamic)."""
    c = C.BY_NAME[name]
    f, _ = _f(name)
    dists = M.distances(c.image.shape[1], c.channels)
    info = C.model_file(name)[1]
    for k, s0 in enumerate(range(0, len(f), M.SEG)):
        s1 = min(s0 + M.SEG, len(f))
        bits = []
        for kind in range(3):
            data, i = M.encode_segment(f, s0, s1, dists, True, force=kind)
            d = zlib.decompressobj(-15, zdict=f[max(0, s0 - 32768):s0].tobytes()) if s0 else zlib.decompressobj(-15)
            assert d.decompress(data) == f[s0:s1].tobytes() and d.eof
            assert len(data) == -(-i["block_bits"] // 8)
            bits.append(i["block_bits"])
        assert tuple(bits) == info[k]["counts"]
        assert info[k]["kind"] == min(range(3), key=lambda j: (bits[j], j))
        # a segment that is not the last ends on a byte boundary, with the empty stored block unless it is stored itself
        if s1 != len(f):
            data, i = M.encode_segment(f, s0, s1, dists, False)
            assert len(data) <= s1 - s0 + 10
            if i["kind"] == 0:          # stored: the five header bytes and the segment, nothing after it
                assert data == bytes([0]) + (s1 - s0).to_bytes(2, "little") + ((s1 - s0) ^ 0xFFFF).to_bytes(2, "little") + f[s0:s1].tobytes()
            else:                       # the block, BFINAL = 0 BTYPE = 00, zero bits to the byte, LEN = 0, NLEN = FFFF
                assert len(data) == -(-(i["block_bits"] + 3) // 8) + 4 and data[-4:] == b"\x00\x00\xff\xff"
                assert int.from_bytes(data[:-4], "little") >> i["block_bits"] == 0


# ------------------------------------------------------------------------------------------------------ what each case is for
def test_segment_boundaries():
    assert len(_f("f-exactly-seg-gray")[0]) == M.SEG and len(C.model_file("f-exactly-seg-gray")[1]) == 1
    assert len(_f("f-seg-plus-1-gray")[0]) == M.SEG + 1 and len(C.model_file("f-seg-plus-1-gray")[1]) == 2
    assert len(C.model_file("f-seg-plus-1-gray")[1][1]["tokens"]) == 1                    # a one-byte last segment
    assert _f("w7-rgb")[0].size // 5 == 22
    # all zeros: 258-byte matches at distance 1 that begin right at a segment's first byte (reaching back before it) and a last
    # match of every segment that the segment's end cuts short
    f, _ = _f("zeros-over-two-segments-gray")
    info = C.model_file("zeros-over-two-segments-gray")[1]
    assert 2 * M.SEG < len(f) < 2 * M.SEG + 258 and len(info) == 3
    assert info[0]["tokens"][0] == 0 and info[1]["tokens"][0] == (258, 1) and info[2]["tokens"][0][1] == 1
    for i in info[:2]:
        assert 3 <= i["tokens"][-1][0] < 258 and set(i["tokens"][1:-1]) == {(258, 1)}


def test_matches_at_every_candidate_distance():
    """The list the size measurements chose is (1, bpp): the cases written for a distance of a row now show that such a match is
    NOT taken (their second row is coded by literals or by the Up filter's zeros)."""
    assert M.distances(128, 3) == (1, 3) and M.distances(128, 1) == (1,) and M.distances(40000, 3) == (1, 3)
    assert {d for _, d in _matches("sub-period-3-rgb")} == {3} and 1 in _f("sub-period-3-rgb")[1]
    assert {d for _, d in _matches("one-row-rgb")} == {3}
    assert {d for _, d in _matches("two-identical-noisy-rows-gray")} == {1}                 # the Up filter turns row 1 into zeros
    f, types = _f("two-shifted-rows-gray")
    assert types.tolist() == [1, 1] and f[2:301].tobytes() == f[303:].tobytes()              # equal filtered rows, a row apart
    assert {d for _, d in _matches("two-shifted-rows-gray")} <= {1}
    # a match of either distance that begins in a segment's first bytes and reaches back into the segment before
    for name, d in (("zeros-over-two-segments-gray", 1), ("sub-period-3-over-a-segment-rgb", 3)):
        firsts = [i["tokens"][0] for i in C.model_file(name)[1][1:]]
        assert any(isinstance(t, tuple) and t[1] == d for t in firsts), (name, firsts)
    assert {d for n in CASE_IDS for _, d in _matches(n)} == {1, 3}


def test_stored_fixed_and_dynamic_are_all_chosen():
    kinds = {n: [i["kind"] for i in C.model_file(n)[1]] for n in CASE_IDS}
    for name in ("uniform-random-gray", "uniform-random-rgb", "all-values-equally-gray"):
        assert set(kinds[name]) == {0}, name
        f, _ = _f(name)
        # stored: 5 bytes a segment, no empty block after it: the bound less 5 bytes a segment
        assert len(M.idat_of(C.model_file(name)[0])) == M.zlib_bound(len(f)) - 5 * len(kinds[name])
    assert kinds["1x1-gray"] == [1] and kinds["1x1-rgb"] == [1]
    # the fixed form with matches: a length symbol of 8 bits (285), of 7 bits (257..279) and distance symbols 0 and 2
    assert kinds["one-literal-one-match-gray"] == [1] and kinds["fixed-with-matches-rgb"] == [1]
    assert {t for t in _tokens("fixed-with-matches-rgb") if isinstance(t, tuple)} >= {(258, 3), (258, 1)}
    assert {M.length_symbol(n)[0] < 280 for n, _ in _matches("fixed-with-matches-rgb")} == {True, False}
    assert set(kinds["render-like-96x128"]) == {2} and len(kinds["render-like-96x128"]) == 3
    seen = {k for v in kinds.values() for k in v}
    assert seen == {0, 1, 2}


def test_two_coded_symbols_rule():
    toks = _tokens("one-literal-one-match-gray")
    assert toks == [0, (258, 1)]
    lit, dist = M.histograms(toks)
    assert sum(1 for c in dist if c) == 1
    assert M.code_lengths(dist, 15)[:3] == [1, 1, 0]                    # symbol 1 joins symbol 0
    assert M.code_lengths([0] * 30, 15)[:3] == [1, 1, 0]                # no match at all: symbols 0 and 1
    assert M.code_lengths([0, 0, 0, 5] + [0] * 26, 15)[:4] == [1, 0, 0, 1]
    assert not _matches("uniform-random-gray")


def test_fibonacci_counts_run_the_15_bit_repair():
    toks = _tokens("fibonacci-counts-gray")
    assert not [t for t in toks if isinstance(t, tuple)] and _f("fibonacci-counts-gray")[1].tolist() == [0]
    lit, _ = M.histograms(toks)
    assert sorted(c for c in lit if c) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181]
    assert sum(lit) < M.SEG
    assert max(M.code_lengths(lit, 32)) == 18 and max(M.code_lengths(lit, 15)) == 15
    assert C.model_file("fibonacci-counts-gray")[1][0]["kind"] == 2


def test_code_length_alphabet_needs_its_7_bit_limit():
    info = C.model_file("code-length-limit-gray")[1]
    assert len(info) == 1 and info[0]["kind"] == 2
    lit, dist = M.histograms(info[0]["tokens"])
    ll, dl, hlit, hdist, toks, cl, hclen, _ = M.dynamic_plan(lit, dist)
    counts = [0] * 19
    for s, _ in toks:
        counts[s] += 1
    assert not [t for t in info[0]["tokens"] if isinstance(t, tuple)] and _f("code-length-limit-gray")[1].tolist() == [0]
    assert sorted(c for c in counts if c) == [1, 1, 2, 3, 5, 8, 13, 21, 34]
    assert (counts[16], counts[17], counts[18], counts[0], counts[1]) == (1, 1, 3, 8, 2)
    assert max(M.code_lengths(counts, 32)) == 8 and max(cl) == 7


def test_code_lengths_are_complete_prefix_codes():
    rng = np.random.default_rng(0)
    for trial in range(200):
        n = int(rng.integers(2, 287))
        counts = (rng.integers(0, 4, n) * rng.integers(1, 2000, n) ** int(rng.integers(1, 3))).tolist()
        for limit in (15, 7) if n <= 19 else (15,):
            lengths = M.code_lengths(counts, limit)
            used = [x for x in lengths if x]
            assert len(used) >= 2 and max(used) <= limit and sum(2 ** (limit - x) for x in used) == 2 ** limit
            assert all(lengths[s] for s, c in enumerate(counts) if c)


def test_length_tokens_rule():
    assert M.length_tokens([0] * 2) == [(0, 0), (0, 0)]
    assert M.length_tokens([0] * 3) == [(17, 0)] and M.length_tokens([0] * 10) == [(17, 7)] and M.length_tokens([0] * 11) == [(18, 0)]
    assert M.length_tokens([0] * 140) == [(18, 127), (0, 0), (0, 0)]
    assert M.length_tokens([5] * 4) == [(5, 0), (16, 0)] and M.length_tokens([5] * 3) == [(5, 0)] * 3
    assert M.length_tokens([5] * 9) == [(5, 0), (16, 3), (5, 0), (5, 0)]
    assert M.length_tokens([5] * 10) == [(5, 0), (16, 3), (16, 0)]


def test_five_filters_and_the_tie_rule():
    c = C.BY_NAME["five-filters-gray"]
    _, types = _f(c.name)
    brute = _brute_force_filter_types(c.image)
    assert set(types.tolist()) == {0, 1, 2, 3, 4}
    # row 0: nothing above, so Sub and Paeth give the same bytes and the lower number wins; the zero rows: all five tie, None wins
    t0, sums0 = brute[0]
    assert t0 == 1 and sums0[1] == sums0[4] == min(sums0)
    assert brute[-1][0] == 0 and brute[-1][1] == [0] * 5


def test_adler_partials_combine_to_zlib_adler():
    rng = np.random.default_rng(1)
    for n in (1, 5, M.SEG - 1, M.SEG, M.SEG + 1, 3 * M.SEG + 77):
        f = rng.integers(0, 256, n, dtype=np.uint8)
        assert M.adler32_segments(f) == zlib.adler32(f.tobytes())
    assert M.adler32_segments(np.full(5 * M.SEG, 255, dtype=np.uint8)) == zlib.adler32(b"\xff" * (5 * M.SEG))


# ------------------------------------------------------------------------------------------------------------------- package
def test_package_container_equals_the_model():
    for h, w, ch in ((1, 1, 1), (7, 5, 3)):
        assert png_file(h, w, ch, b"\x78\x01abc") == M.png_container(h, w, ch, b"\x78\x01abc")


def test_encoder_argument_errors_on_cpu_tensors():
    with pytest.raises(_lib.HipExtensionError):
        PngEncoder("cpu")
    enc = PngEncoder("cuda")                        # touches no device until it encodes
    good = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for call in (enc.encode, enc.launch):
        with pytest.raises(_lib.HipExtensionError):
            call(good)                              # a host tensor: no CPU fallback
        with pytest.raises(_lib.HipExtensionError):
            call(np.zeros((1, 8, 8, 3), dtype=np.uint8))
        with pytest.raises(ValueError):
            call(good.float())                      # dtype
        with pytest.raises(ValueError):
            call(good[0, 0, 0])                     # rank
        with pytest.raises(ValueError):
            call(torch.zeros((1, 8, 8, 4), dtype=torch.uint8))      # channels
        with pytest.raises(ValueError):
            call(good[:, :, ::2])                   # not contiguous
        with pytest.raises(ValueError):
            call(torch.zeros((1, 0, 8, 3), dtype=torch.uint8))
    with pytest.raises(_lib.HipExtensionError):
        _lib.png_encode(good, torch.zeros((1, 512), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32),
                        torch.zeros((1, 2), dtype=torch.int32), torch.zeros(64, dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HipExtensionError):
            save_png_device("never-written.png", np.zeros((4, 4, 3), dtype=np.uint8))


def test_size_helpers_are_pure_host():
    lib = _lib.load()
    for h, w, ch in ((1, 1, 1), (1, 1, 3), (128, 127, 1), (145, 112, 1), (1024, 1280, 3)):
        n = h * (1 + w * ch)
        assert lib.se_png_encode_bound(h, w, ch) == M.zlib_bound(n) == PngEncoder.bound(h, w, ch)
        assert lib.se_png_encode_bound(h, w, ch) <= n * 1.001 + 16 + 6                 # within 0.1 % of the raw size
    one = lib.se_png_encode_scratch_bytes(1, 1024, 1280, 3)
    assert 2 * 1024 * 3841 <= one < 2.1 * 1024 * 3841                                  # F and the segments' slots, little else
    assert lib.se_png_encode_scratch_bytes(8, 1024, 1280, 3) > 7 * one
    for bad in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 8, 8, 2), (1, 8, 8, 4), (70000, 8, 8, 3), (1, 40000, 20000, 3)):
        assert lib.se_png_encode_scratch_bytes(*bad) == -1
    assert lib.se_png_encode_bound(0, 8, 3) == -1
    assert _lib.ABI_VERSION >= 42


# ----------------------------------------------------------------------------------------------------------------------- CLI
def test_parsers_accept_png_encoder_and_default_to_host(capsys):
    import demo
    import run_sequence
    import visualize
    assert demo.parse_args([]).png_encoder == "host"
    assert demo.parse_args(["--render_dir", "x", "--png_encoder", "device"]).png_encoder == "device"
    base = ["--img_path", "a.jpg", "--depth_path", "a.exr", "--pose_path", "a.pkl"]
    assert visualize.parse_args(base).png_encoder == "host"
    assert visualize.parse_args(base + ["--png_encoder", "device"]).png_encoder == "device"
    seq = ["--root_dir", "r", "--seq_name", "s"]
    assert run_sequence.build_parser().parse_args(seq).png_encoder == "host"
    assert run_sequence.build_parser().parse_args(seq + ["--render_dir", "d", "--png_encoder", "device"]).png_encoder == "device"
    for parse, args in ((demo.parse_args, []), (visualize.parse_args, base), (run_sequence.build_parser().parse_args, seq)):
        with pytest.raises(SystemExit):
            parse(args + ["--png_encoder", "gpu"])
    capsys.readouterr()
