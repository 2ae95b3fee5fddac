"""numpy float64 restatement of se_scene_probe_f64 (include/sceneego_hip.h) in the same operation order: sums and products only,
every dot product (x x + y y) + z z, so each value has one correctly rounded answer and the kernel is compared bit for bit.
``argmin`` / ``argmax`` return the lowest index among equals, which is the kernel's tie rule."""
import numpy as np


def scene(depth, ray_tab, min_z, max_depth):
    """(d [B,N] float64, surface [B,N] bool, s [B,N,3], scene [B,N] bool, finite [N] bool) of the N = H * W pixels, n = y * W + x."""
    B, dh, dw = depth.shape
    H, W = ray_tab.shape[:2]
    ys, xs = (np.arange(H) * dh) // H, (np.arange(W) * dw) // W
    d = depth[:, ys][:, :, xs].astype(np.float64).reshape(B, H * W)
    rays = ray_tab.reshape(H * W, 3)
    finite = np.isfinite(rays).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        surface = (d > 0.0) & (d <= max_depth)                    # a NaN fails both
        s = rays[None] * d[:, :, None]
        is_scene = surface & (s[:, :, 2] > min_z) & finite[None]
    return d, surface, s, is_scene, finite


def probe(depth, ray_tab, probes, min_z, max_depth):
    """(out [B,P,8] float64, index [B,P,2] int32)."""
    B, P = probes.shape[:2]
    d, surface, s, is_scene, finite = scene(depth, ray_tab, min_z, max_depth)
    rays = ray_tab.reshape(-1, 3)
    out = np.full((B, P, 8), np.nan, dtype=np.float64)
    index = np.full((B, P, 2), -1, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for p in range(P):
                c = probes[b, p]
                if not np.isfinite(c).all():
                    continue
                out[b, p, 7] = 0.0
                e = s[b] - c[None]
                q = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                q = np.where(is_scene[b], q, np.inf)
                if is_scene[b].any():
                    # among equal q the lowest n that is a scene point (a dropped pixel holds +inf, and so may a scene point)
                    n = int(np.flatnonzero(is_scene[b] & (q == q.min()))[0])
                    out[b, p, 0] = q[n]
                    out[b, p, 1:4] = s[b, n]
                    index[b, p, 0] = n
                else:
                    out[b, p, 0] = np.inf
                out[b, p, 4] = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
                t = (rays[:, 0] * c[0] + rays[:, 1] * c[1]) + rays[:, 2] * c[2]
                t = np.where(finite, t, -np.inf)
                if finite.any():
                    n = int(np.flatnonzero(finite & (t == t.max()))[0])
                    out[b, p, 5] = t[n]
                    out[b, p, 6] = d[b, n] if surface[b, n] else np.nan
                    index[b, p, 1] = n
                else:
                    out[b, p, 5] = -np.inf
    return out, index


def bits(a):
    """The raw 64-bit patterns of a float64 array (NaN payloads and signed zeros included)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
