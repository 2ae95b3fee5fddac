"""Float64 numpy model of the packed float32 convolution weights (se_conv3d_pack_f32), written from the layout comments of
csrc/conv3d_pack.h and independent of its code: for every element of every section the exact value, its magnitude
|scale| * sum_k |G_k * w_k| (what a rounding bound scales with) and whether it is zero padding.

Sections (all index lists are C order, the last index runs fastest; lane = 16 * h + c16):
  A  [cin_pad/16 cg][tap][nt][lane][j 4]           W[16 nt + c16][16 cg + 4 h + j][tap]
  B  [cin_pad/4 ch][g 86][nt][lane][j 4]           W[16 nt + c16][4 ch + j][tap 4 g + h], tap 343 is padding
  E  [cg][cb][tap2d 9][xi 6][nt2 2][lane][j 4]     F(4,3) along z of W[32 cb + 16 nt2 + c16][16 cg + 4 h + j][. , tap2d]
  F  [ceil(cin_pad/3) ch][g 13]{[lane][xi 0..3][j 3], [lane][xi 4..7][j 3], [lane][xi 8..9][j 3]}   F(4,7) of W[c16][3 ch + j][. , tap2d 4 g + h],
                                                   taps >= 49 padding
  G  [cb][cin_pad/8 ch][xi_z 6][q 2][dx 3][ct 2][lane][e 2][c 2]   (F(4,3) over dz) x (F(2,3) over dy), xi_y = 2 q + e,
                                                   of W[32 cb + 16 ct + c16][8 ch + 2 h + c][., ., dx]
  H  [ceil(cin_pad/3) ch][g 37][lane][xi 12]       F(6,7) along z; slot 4 g + h = channel * 49 + tap2d, slot 147 padding
  I  [cb][cin_pad/4 ch][q 9][dx 3][ct 2][lane][j 4]   xi = 4 q + j = 6 xi_y + xi_z, (F(4,3) over dz) x (F(4,3) over dy),
                                                   of W[32 cb + 16 ct + c16][4 ch + h][., ., dx]
Every value is times the folded BatchNorm scale gamma / sqrt(var + eps) of its output channel (1 without BatchNorm); an element whose
output channel is >= cout or whose input channel is >= cin is zero padding."""
from fractions import Fraction as Fr

import numpy as np


def cook_toom_G(points, r):
    """G of the Cook-Toom transform with these finite points and the point at infinity: row i = p_i^j / prod_{k != i} (p_i - p_k)."""
    rows = []
    for i, p in enumerate(points):
        n = Fr(1)
        for k, q in enumerate(points):
            if k != i:
                n *= p - q
        rows.append([p ** j / n for j in range(r)])
    rows.append([Fr(0)] * (r - 1) + [Fr(1)])
    return np.array([[float(v) for v in row] for row in rows], dtype=np.float64)


def _pm(*ps):
    out = [Fr(0)]
    for p in ps:
        out += [p, -p]
    return out


G23 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
G43 = np.array([[Fr(1, 4), 0, 0], [Fr(-1, 6)] * 3, [Fr(-1, 6), Fr(1, 6), Fr(-1, 6)], [Fr(1, 24), Fr(1, 12), Fr(1, 6)],
                [Fr(1, 24), Fr(-1, 12), Fr(1, 6)], [0, 0, 1]], dtype=np.float64)
G47 = cook_toom_G(_pm(Fr(1), Fr(2), Fr(1, 2), Fr(3, 4)), 7)             # points 0, +-1, +-2, +-1/2, +-3/4, inf
G67 = cook_toom_G(_pm(Fr(1), Fr(3, 4), Fr(3, 2), Fr(1, 3), Fr(5, 2)), 7)  # points 0, +-1, +-3/4, +-3/2, +-1/3, +-5/2, inf
assert G43.shape == (6, 3) and G47.shape == (10, 7) and G67.shape == (12, 7)


def round_up(v, m):
    return (v + m - 1) // m * m


def section_sizes(cout, cin_pad, k, transposed):
    """{section: floats} in buffer order, from the conditions and block shapes of the layout comment."""
    nts, cb = round_up(cout, 16) // 16, cout // 32
    taps = 8 if transposed else k ** 3
    s = {"A": (cin_pad // 16) * taps * nts * 256}
    if not transposed and k == 7:
        s["B"] = (cin_pad // 4) * 86 * nts * 256
        if cout <= 16:
            s["F"] = round_up(cin_pad, 3) // 3 * 13 * 10 * 64 * 3
            s["H"] = round_up(cin_pad, 3) // 3 * 37 * 64 * 12
    if not transposed and k == 3 and cout % 32 == 0:
        s["E"] = (cin_pad // 16) * cb * 9 * 6 * 2 * 256
        s["G"] = cb * (cin_pad // 8) * 6 * 2 * 3 * 2 * 64 * 2 * 2
        s["I"] = cb * (cin_pad // 4) * 9 * 3 * 2 * 256
    return s


def scale(c):
    if c["gamma"] is None:
        return np.ones(c["cout"])
    return c["gamma"].astype(np.float64) / np.sqrt(c["var"].astype(np.float64) + np.float64(np.float32(c["eps"])))


def bias_model(c):
    """(value, magnitude |b - mean| * |scale| + |beta|) of bpack [round_up(cout, 16)]; zero beyond cout."""
    cout = c["cout"]
    n = round_up(cout, 16)
    b = np.zeros(cout) if c["b"] is None else c["b"].astype(np.float64)
    val, mag = np.zeros(n), np.zeros(n)
    if c["gamma"] is None:
        val[:cout], mag[:cout] = b, np.abs(b)
    else:
        sc, mean, beta = scale(c), c["mean"].astype(np.float64), c["beta"].astype(np.float64)
        val[:cout] = (b - mean) * sc + beta
        mag[:cout] = np.abs(b - mean) * np.abs(sc) + np.abs(beta)
    return val, mag


def _terms(c, co, ci, coef, tap, extra_pad=None):
    """sum_k coef[..., k] * W[co][ci][tap[..., k]] * scale[co] for index arrays of one section -> (value, magnitude, padding)."""
    cout, cin = c["cout"], c["cin"]
    w = c["w"].astype(np.float64)
    if c["transposed"]:
        w = w.transpose(1, 0, 2)
    pad = (co >= cout) | (ci >= cin)
    if extra_pad is not None:
        pad = pad | extra_pad
    coc, cic = np.where(pad, 0, co), np.where(pad, 0, ci)
    tap = np.where(pad[..., None], 0, tap)
    prod = coef * w[coc[..., None], cic[..., None], tap]
    sc = scale(c)[coc]
    val = np.where(pad, 0.0, sc * prod.sum(-1))
    mag = np.where(pad, 0.0, np.abs(sc) * np.abs(prod).sum(-1))
    return val.ravel(), mag.ravel(), pad.ravel()


def _lane(lane):
    return lane >> 4, lane & 15


def _section(c, name):
    cout, cin_pad, k = c["cout"], c["cin_pad"], c["k"]
    nts, cb = round_up(cout, 16) // 16, cout // 32
    one = np.ones(1)
    if name == "A":
        taps = 8 if c["transposed"] else k ** 3
        cg, tap, nt, lane, j = np.indices((cin_pad // 16, taps, nts, 64, 4))
        h, c16 = _lane(lane)
        return _terms(c, 16 * nt + c16, 16 * cg + 4 * h + j, one, tap[..., None])
    if name == "B":
        ch, g, nt, lane, j = np.indices((cin_pad // 4, 86, nts, 64, 4))
        h, c16 = _lane(lane)
        tap = 4 * g + h
        return _terms(c, 16 * nt + c16, 4 * ch + j, one, tap[..., None], tap >= 343)
    if name == "E":
        cg, b, tap2d, xi, nt2, lane, j = np.indices((cin_pad // 16, cb, 9, 6, 2, 64, 4))
        h, c16 = _lane(lane)
        return _terms(c, 32 * b + 16 * nt2 + c16, 16 * cg + 4 * h + j, G43[xi], tap2d[..., None] + 9 * np.arange(3))
    if name == "F":
        parts = []
        for xi0, nxi in ((0, 4), (4, 4), (8, 2)):
            ch, g, lane, x, j = np.indices((round_up(cin_pad, 3) // 3, 13, 64, nxi, 3))
            h, c16 = _lane(lane)
            tap2d = 4 * g + h
            v = _terms(c, c16, 3 * ch + j, G47[xi0 + x], tap2d[..., None] + 49 * np.arange(7), tap2d >= 49)
            parts.append([a.reshape(ch.shape[0], 13, -1) for a in v])
        return tuple(np.concatenate([p[i] for p in parts], axis=2).ravel() for i in range(3))
    if name == "G":
        b, ch, xz, q, dx, ct, lane, e, cc = np.indices((cb, cin_pad // 8, 6, 2, 3, 2, 64, 2, 2))
        h, c16 = _lane(lane)
        xy = 2 * q + e
        coef = (G43[xz][..., :, None] * G23[xy][..., None, :]).reshape(xz.shape + (9,))
        tap = dx[..., None] + (9 * np.arange(3)[:, None] + 3 * np.arange(3)[None, :]).ravel()
        return _terms(c, 32 * b + 16 * ct + c16, 8 * ch + 2 * h + cc, coef, tap)
    if name == "H":
        ch, g, lane, xi = np.indices((round_up(cin_pad, 3) // 3, 37, 64, 12))
        h, c16 = _lane(lane)
        slot = 4 * g + h
        chan, tap2d = slot // 49, slot % 49
        return _terms(c, c16, 3 * ch + chan, G67[xi], tap2d[..., None] + 49 * np.arange(7), slot >= 147)
    if name == "I":
        b, ch, q, dx, ct, lane, j = np.indices((cb, cin_pad // 4, 9, 3, 2, 64, 4))
        h, c16 = _lane(lane)
        xi = 4 * q + j
        xy, xz = xi // 6, xi % 6
        coef = (G43[xz][..., :, None] * G43[xy][..., None, :]).reshape(xz.shape + (9,))
        tap = dx[..., None] + (9 * np.arange(3)[:, None] + 3 * np.arange(3)[None, :]).ravel()
        return _terms(c, 32 * b + 16 * ct + c16, 4 * ch + h, coef, tap)
    raise KeyError(name)


def pack_model(c):
    """The whole buffer of a case of tests/conv_pack_cases.py: (value, magnitude, padding, {section: (start, floats)})."""
    sizes = section_sizes(c["cout"], c["cin_pad"], c["k"], c["transposed"])
    vals, mags, pads, where, at = [], [], [], {}, 0
    for name, n in sizes.items():
        v, m, p = _section(c, name)
        assert v.size == n, (name, v.size, n)
        vals.append(v), mags.append(m), pads.append(p)
        where[name] = (at, n)
        at += n
    return np.concatenate(vals), np.concatenate(mags), np.concatenate(pads), where


U = 2.0 ** -24          # unit roundoff of float32


def check_packed(c, wpack, bpack):
    """What the host and the GPU test both assert of the buffers written for case c.  Bounds, in units of U times the magnitude:
    wpack 16 - the largest sum has 7 terms (7 roundings), each G constant is rounded to float32 (1), the scale multiply adds 1, the
    scale's own divide and square root at most 4: 13, rounded up to 16; bpack 4."""
    val, mag, pad, where = pack_model(c)
    wpack, bpack = np.asarray(wpack), np.asarray(bpack)
    assert wpack.dtype == np.float32 and bpack.dtype == np.float32
    assert wpack.size == val.size, f"{c['name']}: {wpack.size} floats written, the layout has {val.size}"
    assert not np.isnan(wpack).any(), f"{c['name']}: {int(np.isnan(wpack).sum())} elements of wpack were never written"
    assert not np.isnan(bpack).any(), f"{c['name']}: {int(np.isnan(bpack).sum())} elements of bpack were never written"
    assert np.all(wpack[pad] == 0.0), f"{c['name']}: {int((wpack[pad] != 0).sum())} padding elements are not zero"
    err = np.abs(wpack.astype(np.float64) - val)
    for name, (at, n) in where.items():
        e, m = err[at:at + n], mag[at:at + n]
        worst = float((e[m > 0] / (U * m[m > 0])).max()) if (m > 0).any() else 0.0
        print(f"{c['name']} section {name}: {n} floats, {int(pad[at:at + n].sum())} padding, worst error {worst:.2f} U x magnitude")
    assert np.all(err <= 16 * U * mag), f"{c['name']}: {int((err > 16 * U * mag).sum())} elements of wpack are off by more than 16 U x magnitude"
    bval, bmag = bias_model(c)
    assert bpack.size == bval.size
    berr = np.abs(bpack.astype(np.float64) - bval)
    worst = float((berr[bmag > 0] / (U * bmag[bmag > 0])).max()) if (bmag > 0).any() else 0.0
    print(f"{c['name']} bpack: worst error {worst:.2f} U x magnitude")
    assert np.all(bpack[c["cout"]:] == 0.0), f"{c['name']}: bpack is not zero beyond cout"
    assert np.all(berr <= 4 * U * bmag), f"{c['name']}: {int((berr > 4 * U * bmag).sum())} elements of bpack are off by more than 4 U x magnitude"
