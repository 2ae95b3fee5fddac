"""The inputs of tests/test_gpu_scene_field.py, built on the host so that tests/test_scene_field_host.py can hold every case list to the
conditions it states (on the CPU, without the library).  Nothing here calls the code under test."""
import numpy as np

import scene_field_model as M

FRAME_H, FRAME_W = 32, 40
MIN_Z, MAX_DEPTH = 0.125, 100.0        # a dyadic min_z: s.z == min_z can be planted exactly


# ------------------------------------------------------------------------------------------------------------------ sites
# (G, side): side / (G - 1) is a power of two, so every planted coordinate and every q below is exact in float64
SITE_GRIDS = [(9, 2.0), (16, 1.875)]
SITE_DEPTH_SHAPES = [(32, 40), (16, 20)]            # the frame's own size, and a depth map smaller than the frame


def site_plants(G, side):
    """(kind, (qx, qy, qz) or None, depth value or None, ray or None, expected voxel (i, j, k) or None): what each planted pixel is
    meant to show.  q is the unrounded grid coordinate of the planted scene point."""
    m = 4.0                                         # a voxel well inside, on the other axes
    top = G - 0.5                                   # rint: half to even -> G - 1 (inside) for odd G, G (outside) for even G
    top_in = (G - 1) if (G - 1) % 2 == 0 else None
    e = 2.0 ** -10
    plants = [("centre", (m, m, m), None, None, (4, 4, 4)),
              ("half to even, down", (2.5, m, m), None, None, (2, 4, 4)), ("half to even, up", (3.5, m, m), None, None, (4, 4, 4)),
              ("half to even, y down", (m, 2.5, m), None, None, (4, 2, 4)), ("half to even, y up", (m, 3.5, m), None, None, (4, 4, 4)),
              ("half to even, z down", (m, m, 2.5), None, None, (4, 4, 2)), ("half to even, z up", (m, m, 3.5), None, None, (4, 4, 4)),
              ("minus half rounds to -0: inside", (-0.5, m, m), None, None, (0, 4, 4)),
              ("minus half, y", (m, -0.5, m), None, None, (4, 0, 4)),
              ("top half x", (top, m, m), None, None, None if top_in is None else (top_in, 4, 4)),
              ("top half y", (m, top, m), None, None, None if top_in is None else (4, top_in, 4)),
              ("top half z", (m, m, top), None, None, None if top_in is None else (4, 4, top_in)),
              ("outside low x", (-0.5 - e, m, m), None, None, None), ("outside high x", (G - 0.5 + e, m, m), None, None, None),
              ("outside low y", (m, -0.5 - e, m), None, None, None), ("outside high y", (m, G - 0.5 + e, m), None, None, None),
              ("outside high z", (m, m, G - 0.5 + e), None, None, None),
              ("far outside", (1000.0, m, m), None, None, None),
              ("last voxel", (G - 1.0, G - 1.0, G - 1.0), None, None, (G - 1, G - 1, G - 1)),
              ("depth 0", (m, m, m), 0.0, None, None), ("depth negative", (m, m, m), -1.5, None, None),
              ("depth NaN", (m, m, m), float("nan"), None, None), ("depth +inf", (m, m, m), float("inf"), None, None),
              ("depth above max_depth", (m, m, m), 150.0, None, None),
              ("z == min_z", "min_z", None, None, None), ("z below min_z", "below", None, None, None),
              ("ray NaN", None, None, (float("nan"), 0.0, 1.0), None), ("ray +inf", None, None, (0.0, float("inf"), 1.0), None),
              ("ray -inf z", None, None, (0.0, 0.0, float("-inf")), None)]
    return plants


def sites_case(G, side, dh, dw, B=2, seed=0):
    """A 32 x 40 frame with a dyadic ray table and dyadic depths, so that s = ray * d is exact, and one pixel per entry of
    site_plants.  Returns (depth [B,dh,dw] float32, ray_tab [H,W,3] float64, planted: list of (kind, b, y, x, q, expected voxel))."""
    g = np.random.default_rng(seed)
    H, W = FRAME_H, FRAME_W
    h, x0 = side / (G - 1), -side / 2.0
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ray = np.stack([(xs - W / 2) / 16.0, (ys - H / 2) / 16.0, np.ones((H, W))], axis=-1).astype(np.float64)     # not unit: not needed
    ray[..., 2] = g.choice(np.array([0.5, 0.75, 1.0, 1.25]), size=(H, W))
    depth = g.choice(np.arange(1, 17) * 0.125, size=(B, dh, dw)).astype(np.float32)
    planted = []
    slot = 0
    for kind, q, dval, r, voxel in site_plants(G, side):
        y, x = 2 * (slot // 20), 2 * (slot % 20)            # even pixels: each owns its depth pixel at both depth-map sizes
        slot += 1
        py, px = (y * dh) // H, (x * dw) // W
        v = 0.5                                             # the planted depth: a power of two, so s / v and ray * v are exact
        if r is not None:
            ray[y, x] = r
        elif isinstance(q, str):
            ray[y, x] = np.array([x0 + 4 * h, x0 + 4 * h, MIN_Z if q == "min_z" else MIN_Z / 2]) / v
        else:
            ray[y, x] = np.array([x0 + q[0] * h, x0 + q[1] * h, q[2] * h]) / v
        for b in range(B):                                  # the ray table is shared by the frames: every frame holds every plant
            depth[b, py, px] = np.float32(v if dval is None else dval)
            keep = dval is None and r is None and not isinstance(q, str)
            planted.append((kind, b, y, x, q if keep else None, voxel if keep else None))
    return depth, ray, planted


# ------------------------------------------------------------------------------------------------------------------ transform
def _flat(G, *ijk):
    return [(i * G + j) * G + k for i, j, k in ijk]


def _frames(G, *site_lists):
    out = np.zeros((len(site_lists), G ** 3), dtype=np.uint8)
    for b, s in enumerate(site_lists):
        out[b, np.asarray(s, dtype=np.int64)] = 1
    return out


def _random(G, B, density, seed):
    g = np.random.default_rng(seed)
    s = (g.random((B, G ** 3)) < density).astype(np.uint8)
    s[s == 1] = g.choice(np.array([1, 1, 255, 2], dtype=np.uint8), size=int((s == 1).sum()))      # any non-zero byte is a site
    return s


def corners(G):
    return _flat(G, *[(a, b, c) for a in (0, G - 1) for b in (0, G - 1) for c in (0, G - 1)])


def transform_cases():
    """[(name, G, sites uint8 [B, G^3])]: the cases the issue lists.  tests/test_scene_field_host.py states and checks what each is
    meant to contain."""
    cases = []
    # G = 2: all 256 patterns as one batch; bit n of the frame number is voxel n
    n = np.arange(256)[:, None]
    cases.append(("all 256 patterns", 2, ((n >> np.arange(8)[None]) & 1).astype(np.uint8)))
    for G in (3, 5, 9, 17, 33):                                             # odd grids; frame 1 sparser
        s = _random(G, 2, 0.08, seed=G)
        s[1] = _random(G, 1, 3.0 / G ** 3 * 4, seed=100 + G)[0]
        if not s[1].any():
            s[1, G ** 3 // 2] = 1
        cases.append((f"odd grid {G}", G, s))
    for G in (16, 64):                                                      # densities 0, about 1 %, 1
        s = np.zeros((3, G ** 3), dtype=np.uint8)
        s[1] = _random(G, 1, 0.01, seed=7 * G)[0]
        s[2] = 1
        cases.append((f"densities at {G}", G, s))
    for G in (127, 128):                                                    # at most 64 sites; d2 reaches 3 (G - 1)^2
        g = np.random.default_rng(G)
        extra = g.choice(G ** 3, size=56, replace=False).tolist()
        cases.append((f"corners at {G}", G, _frames(G, [0], [G ** 3 - 1], corners(G) + extra)))
    G = 9                                                                   # equidistant pairs: the lower index must win
    cases.append(("equidistant pairs", G, _frames(G, _flat(G, (4, 4, 2), (4, 4, 6)), _flat(G, (4, 2, 4), (4, 6, 4)),
                                                  _flat(G, (2, 4, 4), (6, 4, 4)), _flat(G, (0, 1, 0), (1, 0, 0), (0, 0, 1)),
                                                  _flat(G, (1, 7, 3), (7, 1, 3)),
                                                  _flat(G, (1, 7, 3), (7, 1, 3), (3, 3, 8), (5, 5, 0)))))
    G = 17                                                                  # a single plane of sites, across each axis
    idx = np.arange(G ** 3)
    cases.append(("single plane", G, _frames(G, idx[idx // (G * G) == 5], idx[(idx // G) % G == 11], idx[idx % G == 3])))
    s = _random(8, 5, 0.05, seed=8)                                         # a batch mixing empty and full frames
    s[0], s[1], s[3] = 0, 1, 0
    cases.append(("empty and full frames", 8, s))
    return cases


def transform_expected(site_bytes, G):
    """(d2, nearest) of one frame by the cheapest statement of the model that is still independent of the kernel: the trivial answers
    for an empty and a full grid, brute force over the site list up to 3e8 (voxel, site) pairs, the separable form beyond (the 64^3
    grid at 1 %: tests/test_scene_field_host.py holds the two forms to each other at that size)."""
    N = G ** 3
    count = int(np.count_nonzero(site_bytes))
    if count == 0:
        return np.full(N, M.NO_SITE, dtype=np.int32), np.full(N, -1, dtype=np.int32)
    if count == N:
        return np.zeros(N, dtype=np.int32), np.arange(N, dtype=np.int32)
    if N * count <= 3e8:
        return M.distance_brute(site_bytes, G)
    return M.distance_separable(site_bytes, G)


# ------------------------------------------------------------------------------------------------------------------ reduction
#        rows, G: the cases of tests/test_gpu_scene_constraint.py (the chunk rule of se_sa_splits), each with its radii
REDUCTION_CASES = [(1, 8, (4,)),                                            # K = 1; rows_per_frame 1
                   (15, 8, (0, 1, 4, 9, 16, 100, 147, 48387)),              # K = 8; radii2 of 0 and of 48 387
                   (30, 16, (1, 4, 9)), (60, 16, (1, 4, 9)), (120, 16, (0, 48387)),
                   (15, 24, (1, 4, 9)),
                   (15, 64, (1, 4, 9))]


def reduction_field(frames, G, seed):
    """d2 int32 [frames, G^3] of a few random sites per frame (a real field, by the formula) and a random free mask uint8; the LAST
    frame of a case with more than one frame has no site at all."""
    g = np.random.default_rng(seed)
    N = G ** 3
    n = np.arange(N, dtype=np.int64)
    ni, nj, nk = n // (G * G), (n // G) % G, n % G
    d2 = np.empty((frames, N), dtype=np.int32)
    for f in range(frames):
        if frames > 1 and f == frames - 1:
            d2[f] = M.NO_SITE
            continue
        m = g.choice(N, size=5, replace=False).astype(np.int64)
        q = (ni[:, None] - m[None] // (G * G)) ** 2 + (nj[:, None] - (m[None] // G) % G) ** 2 + (nk[:, None] - m[None] % G) ** 2
        d2[f] = q.min(axis=1)
    free = (g.random((frames, N)) < 0.5).astype(np.uint8)
    free[free == 1] = g.choice(np.array([1, 1, 1, 255, 2], dtype=np.uint8), size=int((free == 1).sum()))
    return d2, free
