"""The hand-built JPEG files of the decoder tests, named once and shared by tests/test_jpeg_craft_host.py (model against PIL, no
GPU) and tests/test_gpu_jpeg_craft.py (kernels against PIL).  Every file comes from tests/jpeg_craft.py and a seeded generator.

A case says what must happen to it:
  path     "device": the parser takes it for the device; "host": the parser sends it to PIL, ``why`` is a piece of the reason
  pil      PIL decodes it (else PIL raises and so must the decoder, naming the file)
  status   None: the device decode reports nothing; 2 / 3 / 4: the status it reports, after which PIL decodes the file again on the
           host (``DecodeStatus.redecoded``).  Only such a file may be decoded again: that keeps the fall-back from hiding a wrong kernel.
  classes  group 7 only: {block index in MCU order: first failing class "a" / "b" / "c"} of tests/jpeg_model.py plain_classes

Unless a case is about amplitudes its blocks are plain: |DC| <= 300 with DC steps of 2 or 3, |AC| <= 40 at a density of 0.25 with
steps 2..9 (the host test asserts it with the model's predicate).
"""
from __future__ import annotations

import functools

import numpy as np

import jpeg_craft as C

H0, W0 = 40, 56                                    # the common size: 4:2:0 gives 4 x 3 MCUs
YCC = {"444": [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)], "422": [(1, 2, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)],
       "420": [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]}
GRAY = [(1, 1, 1, 0)]


class Case:
    def __init__(self, name, group, data, path="device", why="", pil=True, status=None, classes=None):
        self.name, self.group, self.data, self.path, self.why, self.pil, self.status = name, group, data, path, why, pil, status
        self.classes = classes or {}
        self.H, self.W = int.from_bytes(_sof(data)[3:5], "big"), int.from_bytes(_sof(data)[5:7], "big")

    def __repr__(self):
        return self.name


def _sof(data):
    pos = 2
    while True:
        while data[pos + 1] == 0xFF:
            pos += 1
        m, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if m in (0xC0, 0xC1):
            return data[pos + 2:pos + 2 + n]
        pos += 2 + n


def grid(H, W, comps):
    """[(block rows, block cols)] per component of the padded MCU grid."""
    if len(comps) == 1:
        return [(-(-H // 8), -(-W // 8))]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    return [(my * c[2], mx * c[1]) for c in comps]


def rand_coefs(rng, H, W, comps, dc=300, ac=40, density=0.25):
    out = []
    for r, c in grid(H, W, comps):
        a = rng.integers(-ac, ac + 1, (r, c, 64)) * (rng.random((r, c, 64)) < density)
        a[:, :, 0] = rng.integers(-dc, dc + 1, (r, c))
        out.append(a.astype(np.int64))
    return out


def rand_quant(rng, ids, lo=2, hi=9, wide=False):
    out = {}
    for t in ids:
        q = rng.integers(lo, hi + 1, 64)
        q[0] = rng.integers(2, 4)
        out[t] = (q, wide)
    return out


def plain_file(seed, H=H0, W=W0, comps=None, **kw):
    rng = np.random.default_rng(seed)
    comps = YCC["420"] if comps is None else comps
    quant = kw.pop("quant", None) or rand_quant(rng, sorted({c[3] for c in comps}))
    coefs = kw.pop("coefs", None) or rand_coefs(rng, H, W, comps)
    return C.write_jpeg(H, W, comps, coefs, quant, **kw)


DC16 = C.canonical_table(range(16), 1)                       # sixteen 5-bit codes: DC categories 0..15
DC12_LONG = C.canonical_table(range(12), 12)                 # twelve 12-bit codes
AC10 = C.canonical_table(C.AC_SYMBOLS, 10)                   # 162 ten-bit codes: every code misses the 9-bit lookahead
AC16 = C.canonical_table(C.AC_SYMBOLS, 16)                   # 162 sixteen-bit codes
AC_SPREAD = C.canonical_table(C.AC_SYMBOLS, 10, spread=True)  # lengths 10..16
DC_SPREAD = C.canonical_table(range(12), 10, spread=True)
LONG_TABLES = [((0, 0), DC12_LONG), ((1, 0), AC10), ((0, 1), DC12_LONG), ((1, 1), AC10)]


def _ids(comps, ids):
    return [(i,) + c[1:] for i, c in zip(ids, comps)]


def _group1():
    out = []
    for name, comps in (("444", YCC["444"]), ("422", YCC["422"]), ("420", YCC["420"]), ("gray", GRAY)):
        out.append(Case(f"g1_{name}_19x37", 1, plain_file(100 + len(out), 19, 37, comps)))
    for name in ("422", "420"):
        for H, W in ((5, 3), (7, 4), (3, 5), (9, 2), (33, 6), (19, 4), (35, 3)):     # the last two: 2 chroma columns, several MCU rows
            out.append(Case(f"g1_{name}_{H}x{W}", 1, plain_file(120 + len(out), H, W, YCC[name])))
    return out


def _group2():
    c = YCC["420"]
    rows = [("nojfif", dict(jfif=False), c, "device", ""),
            ("ids012_nojfif", dict(jfif=False), _ids(c, (0, 1, 2)), "device", ""),
            ("idsRGB_jfif", dict(jfif=True), _ids(c, (82, 71, 66)), "device", ""),
            ("idsrgb_nojfif", dict(jfif=False), _ids(c, (114, 103, 98)), "device", ""),
            ("adobe2", dict(jfif=False, adobe=2), c, "device", ""),
            ("jfif_adobe0", dict(jfif=True, adobe=0), c, "device", ""),
            ("adobe0", dict(jfif=False, adobe=0), c, "host", "RGB")]
    return [Case(f"g2_{n}", 2, plain_file(200 + i, comps=comps, **kw), path=path, why=why)
            for i, (n, kw, comps, path, why) in enumerate(rows)]


def _group3():
    rng = np.random.default_rng(300)
    out = [Case("g3_long_codes", 3, plain_file(301, dht=LONG_TABLES)),
           Case("g3_ac16", 3, plain_file(302, dht=[((0, 0), C.std_table(0, 0)), ((1, 0), AC16), ((0, 1), C.std_table(0, 1)), ((1, 1), AC16)])),
           Case("g3_spread", 3, plain_file(303, dht=[((0, 0), DC_SPREAD), ((1, 0), AC_SPREAD), ((0, 1), C.std_table(0, 1)),
                                                     ((1, 1), AC_SPREAD)])),
           Case("g3_ids23", 3, plain_file(304, comps=YCC["444"], scan=[(0, 2, 3), (1, 3, 2), (2, 3, 3)],
                                          dht=[((0, 2), C.std_table(0, 0)), ((0, 3), DC16), ((1, 3), C.std_table(1, 1)), ((1, 2), AC10)])),
           # the first definitions of DC 0 and AC 0 are other tables than the ones the data is coded with
           Case("g3_redefined", 3, plain_file(305, dht=[((0, 0), DC12_LONG), ((1, 0), C.std_table(1, 1)), ((0, 1), C.std_table(0, 1)),
                                                        ((1, 1), C.std_table(1, 1)), ((1, 0), AC10), ((0, 0), C.std_table(0, 0))])),
           Case("g3_quant23", 3, plain_file(306, comps=[(1, 2, 2, 2), (2, 1, 1, 3), (3, 1, 1, 2)]))]
    q = {}
    for t in (0, 1):
        v = rng.integers(256, 401, 64)
        v[0] = 256 + 20 * t
        q[t] = (v, True)
    coefs = rand_coefs(rng, H0, W0, YCC["420"], dc=2, ac=1, density=0.05)
    out.append(Case("g3_dqt16_sof1", 3, C.write_jpeg(H0, W0, YCC["420"], coefs, q, sof=0xC1)))
    return out


def _dc_wrap(W):
    """4:2:0, one MCU row of 8 pixel rows: the lower two luma blocks of every MCU are padding.  In the first MCU they carry DC
    differences of +32767 each, so from the second MCU on the predictor is beyond 65536 while every block that holds samples stores a
    small DC; a later MCU's padding blocks bring it back down, the one after takes it below -65536, the next back up."""
    rng = np.random.default_rng(450 + W)
    comps = YCC["420"]
    coefs = rand_coefs(rng, 8, W, comps, dc=200)
    n = grid(8, W, comps)[0][1] // 2
    raw = {}
    for mcu, step in ((0, 32767), (n // 3, -32767), (n // 3 + 1, -32767), (2 * n // 3 + 1, 32767)):
        raw[(0, 1, 2 * mcu)] = C.Raw(step, [C.EOB])
        raw[(0, 1, 2 * mcu + 1)] = C.Raw(step, [(0, 7 if step > 0 else -7), C.EOB])
    dht = [((0, 0), DC16), ((1, 0), C.std_table(1, 0)), ((0, 1), C.std_table(0, 1)), ((1, 1), C.std_table(1, 1))]
    return C.write_jpeg(8, W, comps, coefs, rand_quant(rng, (0, 1)), dht=dht, raw=raw)


def _group4():
    rng = np.random.default_rng(400)
    out = []
    comps = YCC["420"]
    dense = [rng.choice([-3, -2, -1, 1, 2, 3], (r, c, 64)) for r, c in grid(H0, W0, comps)]
    out.append(Case("g4_no_eob", 4, plain_file(401, coefs=dense, quant=rand_quant(rng, (0, 1), 2, 4))))
    sparse = []
    for r, c in grid(H0, W0, comps):
        a = np.zeros((r, c, 64), dtype=np.int64)
        zz = np.zeros((r, c, 64), dtype=np.int64)
        zz[:, :, 0] = rng.integers(-300, 301, (r, c))
        for k in (20, 41, 63):
            zz[:, :, k] = rng.integers(1, 30, (r, c)) * rng.choice([-1, 1], (r, c))
        zz[::2, :, 63] = 0                           # half the blocks end in an EOB after their ZRLs' coefficient
        zz[:, ::3, 20] = 0                           # a run of 40 zeros: two ZRLs in a row
        a[:, :, C.ZIGZAG] = zz
        sparse.append(a)
    out.append(Case("g4_zrl", 4, plain_file(402, coefs=sparse)))
    big = []
    for r, c in grid(H0, W0, comps):
        a = np.zeros((r, c, 64), dtype=np.int64)
        a[:, :, 0] = 700 * (1 - 2 * ((np.arange(r)[:, None] + np.arange(c)[None, :]) & 1))      # differences of 1400: category 11
        pos = rng.integers(1, 64, (r, c))
        np.put_along_axis(a, pos[:, :, None], (rng.integers(512, 700, (r, c)) * rng.choice([-1, 1], (r, c)))[:, :, None], axis=2)
        big.append(a)
    flat1 = {0: (np.ones(64, dtype=np.int64), False), 1: (np.ones(64, dtype=np.int64), False)}
    out.append(Case("g4_cat11_cat10", 4, plain_file(403, coefs=big, quant=flat1)))
    # the largest values a plain block can hold: pass-2 values of exactly 511 and -512 (DC 4088 and -4096 at a step of 1)
    edge = [np.zeros((r, c, 64), dtype=np.int64) for r, c in grid(H0, W0, comps)]
    for e in edge:
        e[:, :, 0] = np.where((np.arange(e.shape[0])[:, None] + np.arange(e.shape[1])[None, :]) & 1, -4096, 4088)
    dht16 = [((0, 0), DC16), ((1, 0), C.std_table(1, 0)), ((0, 1), DC16), ((1, 1), C.std_table(1, 1))]
    out.append(Case("g4_inside_c", 4, plain_file(404, coefs=edge, quant=flat1, dht=dht16)))
    # runs past coefficient 63 (gray, 5 x 7 blocks; the raw blocks sit among ordinary ones)
    coefs = rand_coefs(rng, H0, W0, GRAY)
    raw = {(0, 0, 1): C.Raw(5, [C.ZRL, C.ZRL, C.ZRL, (15, 7)]),                       # lands at k = 64
           (0, 1, 3): C.Raw(-3, [C.ZRL, C.ZRL, C.ZRL, (10, 3), (10, -9)]),            # the second lands at k = 70
           (0, 2, 0): C.Raw(2, [(0, 5), C.ZRL, C.ZRL, C.ZRL, C.ZRL]),                 # a coefficient, then four ZRLs
           (0, 4, 6): C.Raw(-1, [C.ZRL, C.ZRL, C.ZRL, (15, -4)])}                     # the file's last block
    out.append(Case("g4_overrun", 4, plain_file(405, comps=GRAY, coefs=coefs, raw=raw)))
    out.append(Case("g4_dc_wrap_thread", 4, _dc_wrap(56)))           # 4 MCUs: 16 luma blocks in the segment, one thread per run
    out.append(Case("g4_dc_wrap_workgroup", 4, _dc_wrap(280)))       # 18 MCUs: 72 luma blocks, one workgroup per run
    return out


def _group5():
    out = [Case(f"g5_dri{n}", 5, plain_file(500 + i, restart=n)) for i, n in enumerate((1, 2, 5, 11, 12, 13, 65535))]
    out.append(Case("g5_dri2_fill_zero_pad", 5, plain_file(510, restart=2, rst_fill=3, pad_ones=False)))
    out.append(Case("g5_gray_dri1", 5, plain_file(511, comps=GRAY, restart=1, coefs=rand_coefs(np.random.default_rng(511), H0, W0, GRAY,
                                                                                                dc=20, ac=2, density=0.03))))
    out.append(Case("g5_header_fill", 5, plain_file(512, restart=5, extra=C.com(b"made by hand") + C.appn(3, b"xyz\0" * 5) + b"\xff\xff\xff")))
    return out


def _group6():
    rng = np.random.default_rng(600)
    a = rng.integers(-3, 4, (16, 16, 64)) * (rng.random((16, 16, 64)) < 0.7)
    a[:, :, 0] = rng.integers(-300, 301, (16, 16))
    return [Case("g6_long_segment", 6, C.write_jpeg(128, 128, GRAY, [a], rand_quant(rng, (0,), 2, 4), dht=LONG_TABLES[:2]))]


def _group7():
    """Gray files of 5 x 7 blocks, quantisation step 1 except where stated, plain blocks around the marked ones."""
    out = []
    dht = [((0, 0), DC16), ((1, 0), C.canonical_table([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 16)], 9))]

    def build(seed, marks, q=None, comps=GRAY, comp=0):
        rng = np.random.default_rng(seed)
        coefs = rand_coefs(rng, H0, W0, comps, dc=200, ac=20, density=0.2)
        for (by, bx), vals in marks.items():
            coefs[comp][by, bx] = 0
            for k, v in vals.items():
                coefs[comp][by, bx, k] = v
        quant = {c[3]: (np.ones(64, dtype=np.int64) if q is None else np.asarray(q), False) for c in comps}
        d = dht if len(comps) == 1 else dht + [((0, 1), DC16), ((1, 1), dht[1][1])]
        return C.write_jpeg(H0, W0, comps, coefs, quant, dht=d)

    q64 = np.ones(64, dtype=np.int64)
    q64[9] = 64
    # a: 600 * 64 = 38400 leaves int16; the block at (3, 3) is just inside c (pass-2 values of 511)
    out.append(Case("g7_a", 7, build(701, {(1, 2): {0: 10, 9: 600}, (3, 3): {0: 4088}}, q64), status=4, classes={1 * 7 + 2: "a"}))
    # b: DC 9000 is an int16, its workspace value 36000 is not; (2, 5) is just inside a (32767) and fails b as well
    out.append(Case("g7_b", 7, build(702, {(0, 4): {0: 9000}, (2, 5): {0: 32767}, (4, 0): {0: -4096}}), status=4,
                    classes={4: "b", 2 * 7 + 5: "b"}))
    # c: DC 5000: workspace 20000, pass-2 value 625; (3, 1) is just inside b (workspace 32764) and fails c; (1, 1): -513
    out.append(Case("g7_c", 7, build(703, {(4, 6): {0: 5000}, (3, 1): {0: 8191}, (1, 1): {0: -4104}, (0, 0): {0: 4088}}), status=4,
                    classes={4 * 7 + 6: "c", 3 * 7 + 1: "c", 1 * 7 + 1: "c"}))
    # c through AC coefficients alone
    out.append(Case("g7_c_ac", 7, build(704, {(2, 2): {0: 0, 1: 3000, 8: -3000}}), status=4, classes={2 * 7 + 2: "c"}))
    # mixed, 4:2:0: a in luma, b in Cb, c in Cr (MCU order: 6 blocks per MCU, 4 MCUs per row)
    rng = np.random.default_rng(705)
    comps = YCC["420"]
    coefs = rand_coefs(rng, H0, W0, comps, dc=200, ac=20, density=0.2)
    coefs[0][3, 5] = 0
    coefs[0][3, 5, 9] = 600
    coefs[1][2, 1] = 0
    coefs[1][2, 1, 0] = -9000
    coefs[2][0, 3] = 0
    coefs[2][0, 3, 0] = 5000
    quant = {0: (q64, False), 1: (np.ones(64, dtype=np.int64), False)}
    d = dht + [((0, 1), DC16), ((1, 1), dht[1][1])]
    out.append(Case("g7_mixed_420", 7, C.write_jpeg(H0, W0, comps, coefs, quant, dht=d), status=4,
                    classes={(1 * 4 + 2) * 6 + 3: "a", (2 * 4 + 1) * 6 + 4: "b", (0 * 4 + 3) * 6 + 5: "c"}))
    return out


def _group8():
    out = []
    info = {}
    base = plain_file(800, restart=2, info=info)
    a, b = info["segments"][2]
    out.append(Case("g8_short_segment", 8, base[:b - 6] + base[b:], status=3))
    n = (b - a) // 2
    out.append(Case("g8_all_ones_segment", 8, base[:a] + b"\xff\x00" * n + base[a + 2 * n:], status=2))
    out.append(Case("g8_junk_after_segment", 8, base[:b] + b"\x12\x34\x56" + base[b:]))
    out.append(Case("g8_scan_order", 8, plain_file(801, comps=YCC["444"], scan=[(1, 1, 1), (0, 0, 0), (2, 1, 1)]), path="host",
                    why="scan order", pil=False))
    whole = plain_file(802)
    out.append(Case("g8_no_eoi", 8, whole[:-2], path="host", why="without a marker", pil=False))
    sos = base.index(b"\xff\xda")
    out.append(Case("g8_cut_in_half", 8, base[:sos + (len(base) - sos) // 2], path="host", why="without a marker", pil=False))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _group1() + _group2() + _group3() + _group4() + _group5() + _group6() + _group7() + _group8()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)
