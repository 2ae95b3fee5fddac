"""Deterministic inputs (sceneego_amd.synth streams) for the volume input / output kernels at the shapes where they can go wrong and
the workload's own shape (64^3, a 1024 x 1280 table, 32 channels, cuboid side 2) cannot show it.  Used by tests/test_volume_io_host.py
(which proves on the CPU that the cases can tell a wrong evaluation from the right one) and tests/test_gpu_volume_io.py."""
import functools

import numpy as np

import volume_io_model as M
from sceneego_amd import synth

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ voxeliser
#  up * up = 576 / 1600: no multiple of the 256-thread block; 17 x 29 and 40 x 40 do not divide (or equal) every `up`; side 2.4 and 0.7
#  make G / side inexact, so that (p + side/2) * G / side depends on the order of its operations; side 2.0 keeps the workload's.
#  Both inexact sides come with G = 6 as well: with a power-of-two G the product by G is exact, and dividing first gives the same bits.
VOXEL_CASES = {
    #  name             B  dh  dw  up pad_x  G  side
    "u24_g6_s24":      (1, 17, 29, 24, 8,    6, 2.4),
    "u40_g6_s07":      (3, 40, 40, 40, 0,    6, 0.7),
    "u40_g16_s20":     (1, 17, 29, 40, 8,   16, 2.0),
    "u24_g16_s24":     (3, 40, 40, 24, 0,   16, 2.4),
    "u24_g8_s07":      (1, 17, 29, 24, 0,    8, 0.7),
    "u40_g8_s20":      (3, 40, 40, 40, 8,    8, 2.0),
}
#  se_voxelize_full_f64: no resize, no padding, a ray per depth pixel
VOXEL_FULL_CASES = {
    "full_17x29_g6_s24":  (1, 17, 29, 6, 2.4),
    "full_40x40_g16_s07": (3, 40, 40, 16, 0.7),
    "full_17x29_g8_s20":  (3, 17, 29, 8, 2.0),
}


def _rays(seed, h, w):
    """Arbitrary float64 unit vectors [h, w, 3] looking into the cuboid (z > 0)."""
    u = synth.uniform01(seed, "vio/ray", h * w * 3).reshape(h, w, 3)
    v = np.stack([2.0 * u[..., 0] - 1.0, 2.0 * u[..., 1] - 1.0, 0.25 + 0.75 * u[..., 2]], axis=-1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _is_pow2(x):
    m, _ = np.frexp(x)
    return m == 0.5


def _tie_inputs(seed, B, dh, dw, up_h, up_w, G, side):
    """(depth float32 [B, dh, dw], ray float64 [up_h, up_w, 3]).

    About half of the depth pixels are TIE depths: for the first resized pixel that reads the depth pixel, a seeded axis and an
    integer k in [-1, G - 1] (k = -1 and k = G - 1 are the two edges of the range test), d0 = ((k + 0.5) * side / G - off) / ray[axis]
    solves for the depth at which the voxel coordinate is k + 0.5, and the pixel gets float32(d0) or one of its two float32
    neighbours: within one float32 step of a rounding boundary.  k is drawn among those for which the other two axes land inside the
    grid, so that the pixel is seen.  A float32 step is ~1e8 float64 steps, so such a depth alone cannot tell two float64
    evaluation orders apart; the ray table is arbitrary, so for one sample per tie pixel the ray component is then moved (by the float32 rounding
    of the depth, a relative 1e-7, and a few float64 steps) to where the left-to-right evaluation and a wrong one (precomputed G / side, or
    division first) round to different voxels, or, for a power-of-two side where they cannot differ, to an exact float64 tie.
    The other pixels: depth 0, a depth far outside the cuboid, +inf, and random depths inside."""
    ray = _rays(seed, up_h, up_w)
    sy, sx = M.nearest_index(up_h, dh), M.nearest_index(up_w, dw)
    rep_y, rep_x = np.full(dh, -1), np.full(dw, -1)
    for y in range(up_h - 1, -1, -1):
        rep_y[sy[y]] = y
    for x in range(up_w - 1, -1, -1):
        rep_x[sx[x]] = x
    u = synth.uniform01(seed, "vio/pick", B * dh * dw * 6).reshape(B, dh, dw, 6)
    depth = (0.05 + u[..., 0] * 1.2 * side).astype(F32)
    kind = u[..., 1]
    depth[(kind >= 0.50) & (kind < 0.56)] = 0.0
    depth[(kind >= 0.56) & (kind < 0.62)] = F32(50.0 * side)
    depth[(kind >= 0.62) & (kind < 0.68)] = np.inf
    offs = (side / 2, side / 2, 0.0)
    ks = np.arange(-1, G, dtype=np.float64)
    steps = np.arange(-256, 257, dtype=np.float64)
    steps = steps[np.argsort(np.abs(steps), kind="stable")]            # nearest first
    pow2 = _is_pow2(side)
    for b in range(B):
        for j in range(dh):
            for i in range(dw):
                y, x = rep_y[j], rep_x[i]
                if kind[b, j, i] >= 0.5 or y < 0 or x < 0:
                    continue
                r = ray[y, x]
                a = int(u[b, j, i, 2] * 3)
                with np.errstate(all="ignore"):
                    d0 = ((ks + 0.5) * side / G - offs[a]) / r[a]
                    ok = np.isfinite(d0) & (d0 != 0)
                    for o in range(3):
                        if o != a:
                            qo = ((r[o] * d0 + offs[o]) * G) / side
                            ok &= (qo > -0.4) & (qo < G - 0.6)
                if not ok.any():
                    continue
                edge = ok & ((ks == -1) | (ks == G - 1))
                pool = np.flatnonzero(edge if (edge.any() and u[b, j, i, 3] < 0.35) else ok)
                pick = pool[int(u[b, j, i, 4] * len(pool))]
                k, d = ks[pick], F32(d0[pick])
                nb = int(u[b, j, i, 5] * 3)
                if nb:
                    d = np.nextafter(d, F32(np.inf) if nb == 1 else F32(-np.inf))
                depth[b, j, i] = d
                flat = j * dw + i
                if flat % B != b or d == 0 or not np.isfinite(d):
                    continue                                            # the ray of a pixel is shared by the B samples: one of them owns it
                want = None if pow2 else ("prescale", "divfirst", None)[(flat // B) % 3]
                r0 = ((k + 0.5) * side / G - offs[a]) / float(d)
                cand = r0 + steps * np.spacing(r0)
                off = None if a == 2 else offs[a]
                q = M.voxel_coordinate(cand * float(d), off, G, side)
                if want is None:
                    with np.errstate(all="ignore"):
                        t = cand * float(d) if off is None else cand * float(d) + off
                        hit = np.flatnonzero(((t * float(G)) / side) == k + 0.5)
                else:
                    hit = np.flatnonzero(q != M.voxel_coordinate(cand * float(d), off, G, side, want))
                if len(hit):
                    ray[y, x, a] = cand[hit[0]]
    return depth, np.ascontiguousarray(ray)


@functools.lru_cache(maxsize=None)
def voxel_case(name):
    B, dh, dw, up, pad_x, G, side = VOXEL_CASES[name]
    depth, ray = _tie_inputs(100 + sorted(VOXEL_CASES).index(name), B, dh, dw, up, up, G, side)
    return {"B": B, "dh": dh, "dw": dw, "up": up, "pad_x": pad_x, "G": G, "side": side, "depth": depth, "ray": ray}


@functools.lru_cache(maxsize=None)
def voxel_full_case(name):
    B, dh, dw, G, side = VOXEL_FULL_CASES[name]
    depth, ray = _tie_inputs(200 + sorted(VOXEL_FULL_CASES).index(name), B, dh, dw, dh, dw, G, side)
    return {"B": B, "dh": dh, "dw": dw, "up": (dh, dw), "pad_x": 0, "G": G, "side": side, "depth": depth, "ray": ray}


# ------------------------------------------------------------------------------------------------------------------ gather
#  channels-last:  B texels channels voxels out_stride_c out_c_offset      (channels 12: 3 quads per voxel, which 256 threads do not
#  divide, so voxels straddle workgroups and the last workgroup ends inside a voxel; out_stride_c > out_c_offset + channels everywhere)
GATHER_CL_CASES = [(1, 35, 4, 257, 16, 8), (3, 35, 12, 1000, 24, 8), (1, 1, 32, 1, 48, 0), (3, 35, 32, 257, 44, 8),
                   (1, 35, 12, 257, 16, 0), (3, 1, 4, 1000, 8, 0), (1, 35, 12, 1, 28, 8)]
#  planar:  B texels channels voxels triplets_total planes_total      (spare triplet slots: 16 -> 2 or 5, 32 -> 1 or 4, 64 -> 2; those beyond the last
#  triplet the channels reach are not the gather's to write;
#  planes_total = channels and channels + 3)
GATHER_PLANAR_CASES = [(1, 35, 16, 257, 6, 16), (3, 35, 32, 1000, 11, 35), (1, 1, 64, 1, 22, 64), (3, 35, 16, 1000, 7, 19),
                       (1, 35, 32, 257, 12, 32), (3, 1, 64, 257, 22, 67)]
#  bfloat16 octet-planar:  B texels channels voxels octs_total out_c_offset      (B = 9: the kernel walks the batch in slices of 8)
GATHER_BF16_CASES = [(1, 35, 8, 257, 3, 8), (3, 35, 32, 1000, 6, 16), (9, 35, 16, 257, 2, 0), (1, 1, 8, 1, 2, 8)]


@functools.lru_cache(maxsize=None)
def gather_table(voxels, texels):
    """(idx int32 [voxels, 4], w float32 [voxels, 4]): random taps in [-1, texels) with random weights (a -1 tap keeps a NON-zero
    weight: it is the index that marks it), and hand-made rows at both ends of the table."""
    seed = 7000 + 31 * voxels + texels
    idx = (synth.uniform01(seed, "vio/gidx", voxels * 4) * (texels + 1)).astype(np.int32).reshape(voxels, 4) - 1
    w = synth.normal(seed, "vio/gw", (voxels, 4))
    L, m = texels - 1, texels // 2
    hand = [([-1, -1, -1, -1], [0.3, -0.7, 1.1, 0.9]),        # no live tap
            ([0, -1, -1, -1], [1.0, 0.0, 0.0, 0.0]),          # one live tap, weight 1
            ([-1, L, -1, -1], [0.5, -1.25, 0.5, 0.5]),
            ([-1, -1, L, 0], [0.0, 0.0, 0.75, -0.75]),        # two, mixed sign
            ([0, L, -1, 0], [0.25, 0.5, 9.0, 0.25]),          # three
            ([L, -1, 0, L], [-1.0, 1.0, 1.0, -1.0]),
            ([0, L, L, 0], [0.1, 0.2, 0.3, 0.4]),             # four, texel 0 and texels - 1
            ([m, m, m, m], [0.25, 0.25, 0.25, 0.25]),         # all taps on one texel
            ([L, L, L, L], [1.0, -1.0, 1.0, -1.0]),           # ... cancelling
            ([0, 0, 0, 0], [0.0, 0.0, 0.0, 0.0]),             # zero weights
            ([0, m, L, m], [1.0, 1.0, 1.0, 1.0])]
    if voxels == 1:
        hand = hand[6:7]
    for t, (hi, hw) in enumerate(hand):
        for row in (t, voxels - 1 - t):
            if 0 <= row < voxels:
                idx[row], w[row] = hi, hw
    return np.ascontiguousarray(idx), np.ascontiguousarray(w.astype(F32))


@functools.lru_cache(maxsize=None)
def gather_feat(B, texels, channels):
    return synth.normal(7100 + B, "vio/feat/%d/%d" % (texels, channels), (B, texels, channels))


# ------------------------------------------------------------------------------------------------------------------ intersection
#  B voxels channels stride_c      (B * voxels * channels / 4 is no multiple of 256; stride_c > 2 * channels)
INTERSECTION_CASES = [(1, 1000, 4, 12), (3, 257, 32, 72), (3, 1, 4, 16), (1, 1000, 32, 80)]


# ------------------------------------------------------------------------------------------------------------------ soft-argmax
def sa_splits(rows):
    """Chunks per row (se_sa_splits of csrc/common.h, restated)."""
    return 32 if rows >= 120 else 64 if rows >= 60 else 128 if rows >= 30 else 256


def sa_chunk(rows, voxels):
    """Voxels per chunk: ceil(voxels / splits) rounded up to a multiple of 4.  Chunk k covers [k * chunk, min((k + 1) * chunk, voxels));
    chunks with k * chunk >= voxels are empty."""
    s = sa_splits(rows)
    return (((voxels + s - 1) // s) + 3) & ~3


SA_ROWS = (1, 15, 29, 30, 59, 60, 119, 120, 121)        # every regime of sa_splits and both sides of each threshold
SA_VOXELS = (4, 64, 216, 1000, 13824)                   # 4 .. 24^3: empty chunks, ragged last chunks
SA_BIG = (120, 64000)                                   # 40^3 in 32 chunks of 2000: more than one 1024-voxel stride of the inner loop
SA_RANDOM_CASES = [(r, n) for r in SA_ROWS for n in SA_VOXELS] + [SA_BIG]
SA_SPIKE_CASES = [(1, 13824), (15, 64), (15, 1000), (30, 13824), (60, 216), (60, 1000), (121, 13824), (29, 4), SA_BIG]
SA_NEGINF_CASES = [(1, 1000), (15, 64), (15, 13824), (30, 1000), (59, 216), (60, 13824), (120, 1000), (121, 64), SA_BIG]


@functools.lru_cache(maxsize=None)
def sa_coord(voxels):
    """[voxels, 3] float32: an irregular table with three different axes, so that no exchange of coordinates can cancel."""
    c = np.stack([synth.uniform(900, "vio/cx", (voxels,), -1.0, 1.0), synth.uniform(901, "vio/cy", (voxels,), -0.7, 1.3),
                  synth.uniform(902, "vio/cz", (voxels,), 0.0, 2.0)], axis=1)
    return np.ascontiguousarray(c.astype(F32))


@functools.lru_cache(maxsize=None)
def sa_random(rows, voxels):
    """Logits with a spread like the network's (standard deviation 6)."""
    return synth.normal(8000 + rows, "vio/lg/%d" % voxels, (rows, voxels), 6.0)


def spike_position(row, rows, voxels):
    """Where row ``row`` gets its spike: the positions walk a chunk (first voxel, last voxel, i mod 4 = 0..3 inside it), then the
    last voxel of the row and the first voxel of the last non-empty chunk."""
    chunk = sa_chunk(rows, voxels)
    n_chunks = (voxels + chunk - 1) // chunk                 # non-empty ones
    kind = (row + (7 if rows == 1 else 0)) % 8
    c0 = ((row * 37 + 5) % n_chunks) * chunk
    c1 = min(c0 + chunk, voxels)
    if kind == 0:
        return c0
    if kind == 1:
        return c1 - 1
    if kind in (2, 3, 4, 5):
        quads = (c1 - c0 + 3) // 4
        return min(c0 + 4 * ((row * 11) % quads) + (kind - 2), c1 - 1)
    if kind == 6:
        return voxels - 1
    return (n_chunks - 1) * chunk


@functools.lru_cache(maxsize=None)
def sa_spike(rows, voxels):
    """(logits, positions): non-positive background (-|N(0, 6)|) and one +80 per row: every other term of the row's sums is below
    e^-80 of the spike's."""
    lg = -np.abs(sa_random(rows, voxels))
    pos = np.array([spike_position(r, rows, voxels) for r in range(rows)])
    lg[np.arange(rows), pos] = 80.0
    return np.ascontiguousarray(lg.astype(F32)), pos


@functools.lru_cache(maxsize=None)
def sa_neginf(rows, voxels):
    """Random logits with -inf entries, by row modulo 4: scattered single entries (one in ten); one whole chunk; both; all of the
    row but one voxel.  Needs more than one non-empty chunk per row (voxels >= 8)."""
    lg = sa_random(rows, voxels).copy()
    chunk = sa_chunk(rows, voxels)
    n_chunks = (voxels + chunk - 1) // chunk
    assert n_chunks >= 2
    scatter = synth.uniform01(8100 + rows, "vio/ninf/%d" % voxels, rows * voxels).reshape(rows, voxels) < 0.1
    for r in range(rows):
        kind = r % 4
        if kind in (0, 2):
            lg[r, scatter[r]] = -np.inf
        if kind in (1, 2):
            c0 = ((r * 13 + 3) % n_chunks) * chunk
            lg[r, c0:min(c0 + chunk, voxels)] = -np.inf
        if kind == 3:
            keep = (r * 101 + 17) % voxels
            v = lg[r, keep]
            lg[r] = -np.inf
            lg[r, keep] = v
        if not np.isfinite(lg[r]).any():                     # scattered entries took the last finite one: keep one
            lg[r, (r * 7) % voxels] = 0.5
    return np.ascontiguousarray(lg)


@functools.lru_cache(maxsize=None)
def sa_nan_rows():
    """rows 15, voxels 1000 (256 chunks of 4): row 3 is -inf throughout, row 7 holds a NaN in a chunk whose other logits are -inf, row 9 a
    NaN among ordinary logits, row 12 one whole chunk of -inf; the other rows are ordinary."""
    lg = sa_random(15, 1000).copy()
    lg[3] = -np.inf
    lg[7, 400:404] = -np.inf
    lg[7, 401] = np.nan
    lg[9, 999] = np.nan
    lg[12, 0:4] = -np.inf
    return lg, (3, 7, 9)
