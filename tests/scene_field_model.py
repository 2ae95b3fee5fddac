"""numpy restatement of the scene distance field of include/sceneego_hip.h (sites, exact Euclidean distance transform, expectation
of a distribution against the field), written from the header and independent of sceneego_amd/op.py and csrc/scene_field.hip.  The
tests feed it the SAME float32 / float64 / int32 / uint8 arrays the code under test gets.

The transform is stated twice: ``distance_brute`` is the definition itself, the minimum of the key (|n - m|^2, m) over the list of
sites in exact integers; ``distance_separable`` is the three-pass form the kernel uses, carrying the key packed as d2 * 2^32 + index
in int64 (an exact integer, compared as one).  tests/test_scene_field_host.py holds the two to each other."""
import numpy as np

NO_SITE = 0x7fffffff
_INF_KEY = (NO_SITE << 32) | 0xffffffff


def sites(depth, ray_tab, G, side, min_z, max_depth):
    """depth [B,dh,dw] float32, ray_tab [H,W,3] float64 -> uint8 [B,G^3]; float64, one operation at a time, as written."""
    B, dh, dw = depth.shape
    H, W = ray_tab.shape[:2]
    y, x = np.divmod(np.arange(H * W, dtype=np.int64), W)
    py, px = (y * dh) // H, (x * dw) // W
    ray = ray_tab.reshape(-1, 3).astype(np.float64)
    finite = np.isfinite(ray).all(axis=1)
    out = np.zeros((B, G * G * G), dtype=np.uint8)
    side, g1 = float(side), float(G - 1)
    half = side / 2.0
    for b in range(B):
        d = depth[b][py, px].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            surface = finite & (d > 0.0) & (d <= float(max_depth))                 # a NaN fails
            s = np.where(finite[:, None], ray, 0.0) * np.where(surface, d, 0.0)[:, None]
            scene = surface & (s[:, 2] > float(min_z))
            qx = np.rint(((s[:, 0] + half) * g1) / side)                           # np.rint: half to even
            qy = np.rint(((s[:, 1] + half) * g1) / side)
            qz = np.rint((s[:, 2] * g1) / side)
            inside = scene & (qx >= 0) & (qx <= g1) & (qy >= 0) & (qy <= g1) & (qz >= 0) & (qz <= g1)
        n = ((qx[inside].astype(np.int64) * G + qy[inside].astype(np.int64)) * G + qz[inside].astype(np.int64))
        out[b, n] = 1
    return out


def distance_brute(site_bytes, G, block=4096):
    """uint8 [G^3] (any non-zero byte is a site) -> (d2 int32 [G^3], nearest int32 [G^3]): the minimum of (|n - m|^2, m) over the
    list of sites m, in int64; 0x7fffffff / -1 without a site."""
    N = G * G * G
    m = np.flatnonzero(np.asarray(site_bytes).reshape(-1) != 0).astype(np.int64)       # ascending
    d2 = np.full(N, NO_SITE, dtype=np.int32)
    near = np.full(N, -1, dtype=np.int32)
    if m.size == 0:
        return d2, near
    mi, mj, mk = m // (G * G), (m // G) % G, m % G
    for n0 in range(0, N, block):
        n = np.arange(n0, min(n0 + block, N), dtype=np.int64)
        ni, nj, nk = n // (G * G), (n // G) % G, n % G
        q = (ni[:, None] - mi[None]) ** 2 + (nj[:, None] - mj[None]) ** 2 + (nk[:, None] - mk[None]) ** 2
        a = np.argmin(q, axis=1)                   # np.argmin: the first of equals, and m ascends: the lowest index
        d2[n] = q[np.arange(n.size), a]
        near[n] = m[a]
    return d2, near


def distance_separable(site_bytes, G):
    """The same result from three passes along k, j and i: each takes, per output, the minimum over the G candidates of its grid line
    of key + (offset^2 << 32), the key being d2 * 2^32 + index; a line position without a candidate holds the largest key."""
    s = np.asarray(site_bytes).reshape(G, G, G) != 0
    idx = np.arange(G * G * G, dtype=np.int64).reshape(G, G, G)
    key = np.where(s, idx, _INF_KEY)
    off = (np.arange(G, dtype=np.int64)[:, None] - np.arange(G, dtype=np.int64)[None]) ** 2 << 32      # [out, cand]
    for axis in (2, 1, 0):
        k = np.moveaxis(key, axis, -1)                                              # [a, b, cand]
        res = np.empty_like(k)
        for a in range(G):                                                          # one slab at a time: G^3 candidates in memory
            line = k[a][:, None, :]
            res[a] = np.where(line >= _INF_KEY, _INF_KEY, line + off).min(axis=-1)
        key = np.moveaxis(res, -1, axis)
    none = key >= _INF_KEY
    d2 = np.where(none, NO_SITE, key >> 32).astype(np.int32).reshape(-1)
    near = np.where(none, -1, key & 0xffffffff).astype(np.int32).reshape(-1)
    return d2, near


def expectation(prob, d2, free, radii2, rows_per_frame):
    """prob [rows,N] float32, d2 int32 and free uint8 [rows / rows_per_frame, N], radii2: K ints -> (out float64 [rows,24], mag float64
    [rows,24]: the sum of the magnitudes of each slot's terms, what a float32 summation bound is relative to).  The distance terms
    are p * sqrt(d2) in float64."""
    rows = prob.shape[0]
    K = len(radii2)
    assert 1 <= K <= 8
    out = np.zeros((rows, 24))
    mag = np.zeros((rows, 24))
    for r in range(rows):
        p = prob[r].astype(np.float64)
        if np.isnan(p).any():
            out[r] = np.nan
            continue
        f = free[r // rows_per_frame] != 0
        d = d2[r // rows_per_frame].astype(np.int64)
        has = d != NO_SITE
        t = p * np.sqrt(np.where(has, d, 0).astype(np.float64))
        terms = [p, np.where(f, 0.0, p), np.where(has, t, 0.0), np.where(has & f, t, 0.0)]
        slots = [0, 1, 2, 3]
        for k in range(K):
            within = d <= int(radii2[k])
            terms += [np.where(within, p, 0.0), np.where(within & f, p, 0.0)]
            slots += [4 + k, 12 + k]
        for slot, v in zip(slots, terms):
            out[r, slot] = v.sum()
            mag[r, slot] = np.abs(v).sum()
    return out, mag
