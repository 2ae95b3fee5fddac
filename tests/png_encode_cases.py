"""The case list of the PNG encoder tests: the smallest images at which the encoder can go wrong, each named after what it
exercises.  ``model_file(name)`` is the numpy model's file of a case, computed once per process."""
import functools
import io
import os
from dataclasses import dataclass

import numpy as np

import png_encode_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
SEG = M.SEG


@dataclass(frozen=True)
class Case:
    name: str
    image: np.ndarray = None          # uint8 [H,W] (gray) or [H,W,3]

    @property
    def channels(self):
        return 1 if self.image.ndim == 2 else 3


def _rng(seed):
    return np.random.default_rng(seed)


def _rows_of_f(n, r):
    assert n % r == 0
    return n // r, r - 1


def _textured_gray(h, w, seed):
    """A gradient with a little noise: compressible, with matches at every candidate distance."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 3 + y * 5) // 4 + _rng(seed).integers(0, 3, (h, w))).astype(np.uint8)


def _sub_period3(h, w, seed):
    """Pixel k of a row is k * (1, 2, 3) plus a per-row offset: the Sub filter leaves (1, 2, 3) repeating, a distance-3 match."""
    k = np.arange(w)[None, :, None] * np.array([1, 2, 3])[None, None, :]
    return ((k + _rng(seed).integers(0, 256, (h, 1, 3))) & 255).astype(np.uint8)


def _shifted_rows(w, seed):
    """A random walk of small steps and the same row plus 128: both rows take the Sub filter and their filtered bytes are equal from
    the second byte on, a distance-R match."""
    row = np.cumsum(_rng(seed).integers(-3, 4, w)) & 255
    return np.stack([row, (row + 128) & 255]).astype(np.uint8)


def _fibonacci_row(seed=0):
    """One gray row whose byte counts (with the filter byte and end-of-block) are the Fibonacci numbers 1, 1, 2, ..., 4181: 10945
    symbols, an unrestricted code 19 bits deep.  No value equals its neighbour, and the values between two zeros differ, so the parse
    finds no match and the histogram is exactly that."""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    values = [0]
    for k in range(1, 10):
        values += [k, 256 - k]                      # small magnitudes: the None filter wins on a single row
    counts = dict(zip(values, reversed(fib[1:])))   # end-of-block is the other 1
    zeros = counts.pop(0) - 1                       # the filter byte is a zero too
    rest = []
    prev = None
    while any(counts.values()):                     # the most frequent value left that differs from the one before
        v = max((c, -i, v) for i, (v, c) in enumerate(counts.items()) if c and v != prev)[2]
        rest.append(v)
        counts[v] -= 1
        prev = v
    out = []
    for i, v in enumerate(rest):                    # a zero after each of the first `zeros` values
        out.append(v)
        if i < zeros:
            out.append(0)
    return np.array(out, dtype=np.uint8)[None, :]


def _code_length_limit_row():
    """One gray row (254 bytes, no match, filter None) whose literal code has 8 symbols of 4 bits, 13 of 6, 21 of 7 and 34 of 8
    (counts 16, 4, 2 and 1: 8/16 + 13/64 + 21/128 + 34/256 = 1), laid out over the byte values so that the code-length symbols
    occur 1 (code 16: the one run of four 4s), 1 (code 17), 2 (the two distance lengths), 3 (code 18), 5 (length 4), 8 (single
    zeros), 13, 21 and 34 times: Fibonacci counts, an unrestricted code 8 bits deep."""
    layout = [(0, 8), (1, 4), (2, 4), (3, 4), (4, 4)]               # (value, code length); value 0 is the filter byte alone
    left = {6: 12, 7: 21, 8: 32}
    middle = []
    while any(left.values()):                                       # the class with most left, never three equal in a row
        length = max((n, k) for k, n in left.items() if n and middle[-2:] != [k, k])[1]
        middle.append(length)
        left[length] -= 1
    gaps = {2 + 4 * i: 1 for i in range(8)}                         # after the middle symbol of that index: unused values
    gaps.update({36: 5, 44: 56, 52: 56, 60: 56})
    value = 5
    for i, length in enumerate(middle):
        layout.append((value, length))
        value += 1 + gaps.get(i, 0)
    assert value == 251
    layout += [(251, 4), (252, 4), (253, 6), (254, 4), (255, 4)]
    row = np.concatenate([np.full(1 << (8 - length) if length > 4 else 16, v) for v, length in layout[1:]])
    _rng(3).shuffle(row)
    return row.astype(np.uint8)[None, :]


def _five_filters(w=48, seed=11):
    """Rows built for one filter each; row 0 ties Sub with Paeth (nothing above), the two zero rows tie all five."""
    r = _rng(seed)
    rows = [np.cumsum(r.integers(1, 4, w)) * 2 & 255]                          # a steep ramp: Sub (= Paeth on row 0)
    rows.append(r.integers(0, 3, w) * 255 & 255)                               # 0 / 255 after a ramp: None
    rows.append(r.integers(0, 256, w))                                         # noise: whatever wins
    rows.append((rows[-1] + r.integers(0, 2, w)) & 255)                        # the row above plus 0 / 1: Up
    cur = np.zeros(w, dtype=np.int64)
    noise = r.integers(0, 256, w)
    rows.append(noise)
    for x in range(w):                                                         # the average of left and above: Average
        cur[x] = (((cur[x - 1] if x else 0) + noise[x]) >> 1) & 255
    rows.append(cur.copy())
    above = r.integers(0, 256, w)
    rows.append(above)
    for x in range(w):                                                         # the Paeth predictor itself: Paeth
        a, b, c = (cur[x - 1] if x else 0), above[x], (above[x - 1] if x else 0)
        p = a + b - c
        cur[x] = min((abs(p - a), 0, a), (abs(p - b), 1, b), (abs(p - c), 2, c))[2]
    rows.append(cur.copy())
    rows += [np.zeros(w, dtype=np.int64), np.zeros(w, dtype=np.int64)]
    return np.stack(rows).astype(np.uint8)


def render_like(h, w, seed=7):
    """A flat background, single-pixel splats of random colours and a thick line: what the renderer's pictures are made of."""
    r = _rng(seed)
    img = np.full((h, w, 3), (24, 26, 32), dtype=np.uint8)
    n = h * w // 12
    img[r.integers(0, h, n), r.integers(0, w, n)] = r.integers(0, 256, (n, 3))
    for t in range(max(h, w)):
        y, x = t * (h - 1) // max(h, w), t * (w - 1) // max(h, w)
        img[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = (255, 120, 20)
    return img


def photo_crop(h=96, w=128):
    from PIL import Image
    img = np.array(Image.open(os.path.join(HERE, "golden", "demo", "img_001000.jpg")).convert("RGB"))
    return np.ascontiguousarray(img[400:400 + h, 500:500 + w])


def _build():
    noise = lambda shape, seed: _rng(seed).integers(0, 256, shape, dtype=np.uint8)          # noqa: E731
    h_exact, w_exact = _rows_of_f(SEG, 128)
    h_plus1, w_plus1 = _rows_of_f(SEG + 1, 113)
    cases = [
        Case("1x1-gray", np.array([[200]], dtype=np.uint8)),
        Case("1x1-rgb", np.array([[[1, 2, 3]]], dtype=np.uint8)),
        Case("one-row-rgb", _sub_period3(1, 40, 1)),
        Case("w7-rgb", noise((5, 7, 3), 2) // 32 * 32),
        Case("f-exactly-seg-gray", _textured_gray(h_exact, w_exact, 3)),
        Case("f-seg-plus-1-gray", _textured_gray(h_plus1, w_plus1, 4)),
        Case("zeros-over-two-segments-gray", np.zeros((255, 128), dtype=np.uint8)),
        Case("two-identical-noisy-rows-gray", np.repeat(noise((1, 300), 5), 2, axis=0)),
        Case("two-shifted-rows-gray", _shifted_rows(300, 6)),
        Case("sub-period-3-rgb", _sub_period3(6, 90, 7)),
        Case("sub-period-3-over-a-segment-rgb", _sub_period3(70, 90, 12)),
        Case("uniform-random-gray", noise((130, 130), 8)),
        Case("uniform-random-rgb", noise((75, 75, 3), 9)),
        Case("single-colour-rgb", np.full((40, 50, 3), 77, dtype=np.uint8)),
        Case("one-literal-one-match-gray", np.zeros((7, 36), dtype=np.uint8)),
        Case("fixed-with-matches-rgb", np.repeat(_sub_period3(1, 100, 13), 2, axis=0)),   # Sub: period 3; Up: zeros; few tokens
        Case("all-values-equally-gray", np.stack([_rng(20 + i).permutation(256) for i in range(8)]).astype(np.uint8)),
        Case("fibonacci-counts-gray", _fibonacci_row()),
        Case("code-length-limit-gray", _code_length_limit_row()),
        Case("five-filters-gray", _five_filters()),
        Case("render-like-96x128", render_like(96, 128)),
        Case("photo-crop-96x128", photo_crop()),
        Case("noise-96x128", noise((96, 128, 3), 10)),
    ]
    return tuple(cases)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
BATCH = ("render-like-96x128", "photo-crop-96x128", "noise-96x128")        # three different frames of one shape


@functools.lru_cache(maxsize=None)
def model_file(name):
    """(file, per-segment info) of the numpy model."""
    info = []
    return M.encode(BY_NAME[name].image, info=info), tuple(info)


def pil_decode(data):
    from PIL import Image
    img = Image.open(io.BytesIO(data))
    return np.array(img), img.mode


def pil_size(image):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(image).save(b, format="PNG")
    return len(b.getvalue())
