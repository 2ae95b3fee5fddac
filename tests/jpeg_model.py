"""A small numpy model of the integer stages of csrc/jpeg.hip, for the CPU tests: sequential Huffman decode (one step per codeword,
exactly as the device steps), DC prediction, libjpeg's ISLOW IDCT (jidctint.c), libjpeg v6b fancy upsampling (jdsample.c h2v1 /
h2v2 with jdmainct.c's edge rows) and jdcolor.c's YCbCr -> RGB, plus the speculative / synchronisation rounds of the parallel decode
with a free lane size, and the predicate of the blocks on which that IDCT equals libjpeg-turbo's SIMD one (``plain_blocks``).  It works on ``sceneego_amd.jpeg_device.JpegFile`` and is meant for small images (pure Python per codeword).
"""
from __future__ import annotations

import numpy as np

from sceneego_amd.jpeg_device import ZIGZAG

NATURAL = np.concatenate([ZIGZAG, np.full(16, 63)])        # jpeg_natural_order with its 16 trailing guard entries
ERR, END = 1 << 16, 1 << 17                                 # flags of a stopped state


class Stream:
    """One segment's unstuffed bits, read MSB first; bits past the end read as 0."""

    def __init__(self, data):
        self.nbits = 8 * len(data)
        self.v = int.from_bytes(data + b"\0\0\0\0", "big")
        self.total = 8 * (len(data) + 4)

    def peek(self, p, n):
        return (self.v >> (self.total - p - n)) & ((1 << n) - 1)


def decode_symbol(tab, st, p):
    """(length, symbol) of the code at bit p, or None when no code matches."""
    from sceneego_amd.jpeg_device import LOOKAHEAD
    e = int(tab.lut[st.peek(p, LOOKAHEAD)])
    if e:
        return e >> 8, e & 255
    code = st.peek(p, 16)
    ln = LOOKAHEAD + 1
    while ln <= 16 and (code >> (16 - ln)) > tab.maxcode[ln]:
        ln += 1
    if ln > 16:
        return None
    return ln, tab.vals[int((code >> (16 - ln)) + tab.valoff[ln])]


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def step(f, st, state, write=None):
    """One codeword (code + its extra bits) from state (p, k, z) -> (p, k, z) or a stopped state (p | ERR or END flag)."""
    p, k, z = state
    fi = f.block_comp[k]
    td, ta = [(t[1], t[2]) for t in f.scan if t[0] == fi][0]
    tab = f.huff[(0, td)] if z == 0 else f.huff[(1, ta)]
    r = decode_symbol(tab, st, p)
    if r is None:
        return (p, k, z, ERR)
    ln, sym = r
    s = sym if z == 0 else sym & 15
    if p + ln + s > st.nbits:
        return (p, k, z, END)
    v = extend(st.peek(p + ln, s), s) if s else 0
    p += ln + s
    if z == 0:
        if write is not None:
            write(0, v, True)
        z = 1
    else:
        run = sym >> 4
        if s:
            z += run
            if write is not None:
                write(int(NATURAL[z]), v, False)
            z += 1
        elif run == 15:
            z += 16
        else:
            z = 64
    if z >= 64:
        k += 1
        z = 0
        if k == f.blocks_per_mcu:
            k = 0
    return (p, k, z)


def run_lane(f, st, entry, end):
    """Decode from ``entry`` while the position is before ``end`` -> (exit state, DC codes decoded)."""
    if len(entry) == 4:
        return (-1, 0, 0, ERR), 0
    s, n = entry, 0
    while s[0] < end:
        if s[2] == 0:
            n += 1
        t = step(f, st, s)
        if len(t) == 4:
            return t, n - (1 if s[2] == 0 else 0)
        s = t
    return s, n


def decode_segment(f, data, n_blocks):
    """Sequential decode -> (int32 [n_blocks, 64] natural order with DC differences, {bit offset: (k, z)} of every boundary)."""
    st = Stream(data)
    coef = np.zeros((n_blocks, 64), dtype=np.int32)
    states = {}
    s, nb = (0, 0, 0), 0

    def write(pos, v, dc):
        coef[nb - 1 if not dc else nb, pos] = v

    while not (s[2] == 0 and nb == n_blocks):
        states[s[0]] = (s[1], s[2])
        t = step(f, st, s, write)
        if len(t) == 4:
            raise ValueError(f"segment stops at bit {t[0]} ({'no code' if t[3] == ERR else 'end'}) after {nb} of {n_blocks}")
        if s[2] == 0:
            nb += 1
        s = t
    states[s[0]] = (s[1], s[2])
    return coef, states


def sync_lanes(f, data, lane_bits, wg=4, rounds=1):
    """The device's lane scheme on one segment: speculative pass, rounds inside workgroups of ``wg`` lanes, ``rounds`` Jacobi
    rounds across workgroups, then the sequential repair.  Returns the entry state of every lane."""
    st = Stream(data)
    nl = max(1, -(-st.nbits // lane_bits))
    ends = [min((j + 1) * lane_bits, st.nbits) for j in range(nl)]
    entry = [(0, 0, 0) if j == 0 else (j * lane_bits, 0, 0) for j in range(nl)]
    res = [run_lane(f, st, entry[j], ends[j]) for j in range(nl)]
    exits = [r[0] for r in res]

    def chain(lo, hi):
        while True:
            need = [j for j in range(max(lo, 1), hi) if j > lo and entry[j] != exits[j - 1]]
            if not need:
                return
            for j in need:
                entry[j] = exits[j - 1]
            for j in need:
                exits[j] = run_lane(f, st, entry[j], ends[j])[0]

    groups = [(g, min(g + wg, nl)) for g in range(0, nl, wg)]
    for lo, hi in groups:
        chain(lo, hi)
    for _ in range(rounds):
        snap = list(exits)
        for lo, hi in groups:
            if lo == 0 or entry[lo] == snap[lo - 1]:
                continue
            entry[lo] = snap[lo - 1]
            exits[lo] = run_lane(f, st, entry[lo], ends[lo])[0]
            chain(lo, hi)
    for lo, hi in groups[1:]:
        e = exits[lo - 1]
        for j in range(lo, hi):
            if entry[j] == e:
                break
            entry[j] = e
            x = run_lane(f, st, e, ends[j])[0]
            if x == exits[j]:
                break
            exits[j] = e = x
    return entry, [run_lane(f, st, entry[j], ends[j])[1] for j in range(nl)]


# ---------------------------------------------------------------------------------------------------------------- integer stages
CONST_BITS, PASS1_BITS = 13, 2


def _fix(x):
    return int(x * (1 << CONST_BITS) + 0.5)


F = {n: _fix(v) for n, v in (("0_298631336", 0.298631336), ("0_390180644", 0.390180644), ("0_541196100", 0.541196100),
                             ("0_765366865", 0.765366865), ("0_899976223", 0.899976223), ("1_175875602", 1.175875602),
                             ("1_501321110", 1.501321110), ("1_847759065", 1.847759065), ("1_961570560", 1.961570560),
                             ("2_053119869", 2.053119869), ("2_562915447", 2.562915447), ("3_072711026", 3.072711026))}


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(v0, v1, v2, v3, v4, v5, v6, v7):
    z2, z3 = v2, v6
    z1 = (z2 + z3) * F["0_541196100"]
    tmp2 = z1 + z3 * (-F["1_847759065"])
    tmp3 = z1 + z2 * F["0_765366865"]
    tmp0 = (v0 + v4) << CONST_BITS
    tmp1 = (v0 - v4) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v7, v5, v3, v1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F["1_175875602"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F["0_298631336"], tmp1 * F["2_053119869"], tmp2 * F["3_072711026"], tmp3 * F["1_501321110"]
    z1, z2 = z1 * (-F["0_899976223"]), z2 * (-F["2_562915447"])
    z3, z4 = z3 * (-F["1_961570560"]) + z5, z4 * (-F["0_390180644"]) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3)


def range_limit(v):
    """range_limit[v & RANGE_MASK] of jidctint.c (range_limit = sample_range_limit + CENTERJSAMPLE)."""
    i = v & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.uint8)


def idct_islow(coef, quant):
    """int [n, 64] natural-order coefficients, int quantisation (as ISLOW_MULT_TYPE) -> uint8 [n, 8, 8]."""
    c = coef.astype(np.int64).reshape(-1, 8, 8)
    q = quant.astype(np.int64).reshape(8, 8)
    dq = (c * q).astype(np.int32).astype(np.int64)             # DEQUANTIZE: int arithmetic
    cols = _idct_1d(*[dq[:, r, :] for r in range(8)])          # pass 1 on columns
    ws = np.stack([_descale(x, CONST_BITS - PASS1_BITS).astype(np.int32).astype(np.int64) for x in cols], axis=1)
    rows = _idct_1d(*[ws[:, :, i] for i in range(8)])          # pass 2 on rows
    out = np.stack([range_limit(_descale(x, CONST_BITS + PASS1_BITS + 3)) for x in rows], axis=2)
    return out


def plain_blocks(coef, quant):
    """bool [n]: the blocks (int [n, 64] natural-order coefficients, quantisation as ISLOW_MULT_TYPE) on which jidctint.c's C code,
    which ``idct_islow`` and csrc/jpeg.hip follow, and libjpeg-turbo's SIMD ISLOW IDCT (jidctint-sse2 / -avx2, what PIL runs) give
    the same samples.  A block is plain when
      (a) every dequantised coefficient fits int16,
      (b) every pass-1 workspace value (after its descale by 11 bits) fits int16,
      (c) every pass-2 value after its descale by 18 bits, before the +128, lies in [-512, 511].

    Why these three suffice.  The SIMD code differs from the C code in four ways only: it multiplies coefficient and quantisation
    value in int16 lanes (low 16 bits of the product), forms a few sums of two inputs in int16 lanes (in0 +- in4, in7 + in3,
    in5 + in1), sums the int16 x constant products in 32 bits where the C code has 64, and narrows with saturating packs (to int16
    after pass 1; to int16, then to int8, then +128 after pass 2) where the C code stores an int and reads
    range_limit[x & 1023].  (a) makes the int16 product the true product.  The 1-D transform is linear; its even part is
    (in0 +- in4) << 13 plus terms of in2, in6, and its odd part is 8192 * 2 * Q with Q orthogonal (the rows are sqrt(2) cos((2x+1)
    u pi / 16), u odd, and sum of cos^2 over the four odd u is 2).  (b) bounds all eight outputs of a column below 2^15 * 2^11 =
    2^26 in magnitude, so every true 32-bit sum fits (and wrapping partial sums leave the true result), the half sums and half
    differences of mirrored outputs bound |in0 +- in4| by 2^13 and the odd inputs' 2-norm by 2^13 (a sum of two of them by
    sqrt(2) 2^13): no int16 lane wraps, and the saturating pack to int16 passes the value through.  In pass 2 (c) bounds the outputs
    below 2^9 * 2^18 = 2^27 and gives the same with 2^14 and sqrt(2) 2^14 < 2^15; the two saturating packs and the +128 then are
    min(max(x, -128), 127) + 128, which is what range_limit[x & 1023] holds for x in [-512, 511] and for no other x in general
    (the table wraps at 1024).  The zero-AC shortcut of both codes is the general formula's value.  Outside (a), (b) or (c) some lane
    may wrap or saturate where the C code does neither: tests/test_jpeg_craft_host.py counts how many such blocks differ."""
    a, b, c = plain_classes(coef, quant)
    return a & b & c


def plain_classes(coef, quant):
    """(a, b, c) of ``plain_blocks`` as three bool [n] arrays (True: the condition holds)."""
    c = coef.astype(np.int64).reshape(-1, 8, 8)
    q = quant.astype(np.int64).reshape(8, 8)
    true = c * q
    a = ((true >= -32768) & (true <= 32767)).all(axis=(1, 2))
    dq = true.astype(np.int32).astype(np.int64)
    ws = np.stack([_descale(x, CONST_BITS - PASS1_BITS) for x in _idct_1d(*[dq[:, r, :] for r in range(8)])], axis=1)
    b = ((ws >= -32768) & (ws <= 32767)).all(axis=(1, 2))
    ws = ws.astype(np.int32).astype(np.int64)
    out = np.stack([_descale(x, CONST_BITS + PASS1_BITS + 3) for x in _idct_1d(*[ws[:, :, i] for i in range(8)])], axis=2)
    return a, b, ((out >= -512) & (out <= 511)).all(axis=(1, 2))


def file_coefficients(f):
    """int32 [blocks, 64] of a device-path JpegFile in MCU order: natural order, DC predicted."""
    bpm = f.blocks_per_mcu
    rows, nbs = [], []
    for _, mc, data in f.segments:
        rows.append(decode_segment(f, data, mc * bpm)[0])
        nbs.append(mc * bpm)
    return dc_predict(np.concatenate(rows), f, nbs)


def file_real(f):
    """bool per block (MCU order): the block holds at least one sample of its component (the others pad the MCU grid: they reach
    no pixel and libjpeg never transforms them)."""
    bpm = f.blocks_per_mcu
    k0, first = 0, {}
    for fi, _, _ in f.scan:
        h, v = f.comp_hv(fi)
        first[fi] = k0
        k0 += h * v
    out = np.zeros(f.mcus_x * f.mcus_y * bpm, dtype=bool)
    for i in range(len(out)):
        m, k = divmod(i, bpm)
        fi = f.block_comp[k]
        h, v = f.comp_hv(fi)
        kk = k - first[fi]
        bx, by = (m % f.mcus_x) * h + kk % h, (m // f.mcus_x) * v + kk // h
        out[i] = 8 * bx < -(-f.W * h // f.hmax) and 8 * by < -(-f.H * v // f.vmax)
    return out


def file_classes(f):
    """(a, b, c) of ``plain_classes`` per block (MCU order) of a device-path JpegFile."""
    coef = file_coefficients(f)
    comp = np.array([f.block_comp[i % f.blocks_per_mcu] for i in range(len(coef))])
    out = [np.ones(len(coef), dtype=bool) for _ in range(3)]
    for fi in set(f.block_comp):
        for o, x in zip(out, plain_classes(coef[comp == fi], f.quant[fi].astype(np.uint16).view(np.int16))):
            o[comp == fi] = x
    return out


def file_plain(f):
    """bool per block (MCU order) of a device-path JpegFile: plain, or a padding block."""
    a, b, c = file_classes(f)
    return (a & b & c) | ~file_real(f)


def dc_predict(coef, f, seg_blocks):
    """Running sum of the DC differences per component, reset at every segment (coef rows in MCU order, all segments)."""
    out = coef.copy()
    bpm = f.blocks_per_mcu
    row = 0
    for nb in seg_blocks:
        last = [0, 0, 0]
        for b in range(nb):
            fi = f.block_comp[b % bpm]
            last[fi] += int(coef[row + b, 0])
            out[row + b, 0] = np.int16(np.int64(last[fi]).astype(np.int16))
        row += nb
    return out


def planes(f, coef):
    """Per-component uint8 planes of the padded MCU grid from the dequantised IDCT of the coefficient rows (MCU order)."""
    bpm = f.blocks_per_mcu
    pix = {}
    k0 = 0
    out = []
    for fi, _, _ in f.scan:
        h, v = f.comp_hv(fi)
        pix[fi] = (k0, h, v)
        k0 += h * v
    for fi in range(len(f.comps)):
        k0, h, v = pix[fi]
        pw, ph = 8 * h * f.mcus_x, 8 * v * f.mcus_y
        pl = np.zeros((ph, pw), dtype=np.uint8)
        ids = [(m * bpm + k0 + yy * h + xx, (m // f.mcus_x) * v + yy, (m % f.mcus_x) * h + xx)
               for m in range(f.mcus_x * f.mcus_y) for yy in range(v) for xx in range(h)]
        blocks = idct_islow(coef[[i for i, _, _ in ids]], f.quant[fi].astype(np.uint16).view(np.int16))
        for (_, by, bx), blk in zip(ids, blocks):
            pl[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = blk
        out.append(pl)
    return out


def _fancy_cols(c, wc, W, rnd_even, rnd_odd, shift):
    """Horizontal triangle filter of jdsample.c on column sums c [rows, >= wc]: out[2j] uses c[j-1], out[2j+1] uses c[j+1]; the
    first / last real column repeat themselves."""
    c = c.astype(np.int64)
    j = np.arange(wc)
    left = c[:, np.maximum(j - 1, 0)]
    right = c[:, np.minimum(j + 1, wc - 1)]
    out = np.empty((c.shape[0], 2 * wc), dtype=np.int64)
    out[:, 0::2] = (3 * c[:, :wc] + left + rnd_even) >> shift
    out[:, 1::2] = (3 * c[:, :wc] + right + rnd_odd) >> shift
    return out[:, :W]


def upsample(f, pl, fi):
    h, v = f.comp_hv(fi)
    W, H = f.W, f.H
    if len(f.comps) == 1 or (h, v) == (f.hmax, f.vmax):
        return pl[:H, :W].astype(np.int64)
    wc, hc = -(-W * h // f.hmax), -(-H * v // f.vmax)
    y, x = np.arange(H), np.arange(W)
    if wc <= 2:                                                # libjpeg-turbo: no fancy upsampling below 3 columns (box filter)
        return pl[(y >> 1) if f.vmax == 2 else y][:, x >> 1].astype(np.int64)
    if f.vmax == 1:                                            # h2v1
        return _fancy_cols(pl[:H], wc, W, 1, 2, 2)
    near = y >> 1
    far = np.where(y & 1, np.minimum(near + 1, hc - 1), np.maximum(near - 1, 0))
    colsum = 3 * pl[near].astype(np.int64) + pl[far].astype(np.int64)
    return _fancy_cols(colsum, wc, W, 8, 7, 4)


def ycc_to_bgr(y, cb, cr):
    one_half = 1 << 15

    def fix(x):
        return int(x * 65536 + 0.5)

    x_cb, x_cr = cb - 128, cr - 128
    r_add = (fix(1.40200) * x_cr + one_half) >> 16
    b_add = (fix(1.77200) * x_cb + one_half) >> 16
    g_add = ((-fix(0.34414)) * x_cb + one_half + (-fix(0.71414)) * x_cr) >> 16
    return np.stack([np.clip(y + b_add, 0, 255), np.clip(y + g_add, 0, 255), np.clip(y + r_add, 0, 255)], axis=-1).astype(np.uint8)


def decode(f):
    """uint8 [H, W, 3] B, G, R of a device-path JpegFile, through the sequential decode."""
    pls = planes(f, file_coefficients(f))
    if len(f.comps) == 1:
        g = pls[0][:f.H, :f.W]
        return np.stack([g, g, g], axis=-1)
    return ycc_to_bgr(upsample(f, pls[0], 0), upsample(f, pls[1], 1), upsample(f, pls[2], 2))
