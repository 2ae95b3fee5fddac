"""float64 numpy restatement of the scene-constraint definitions of include/sceneego_hip.h (sight table, free mask, masked
soft-argmax reduction), written from the header and independent of sceneego_amd/op.py and csrc/scene_constraint.hip.  The tests feed it
the SAME float32 / int32 arrays the code under test gets."""
import math

import numpy as np


def sight_table(uv, centres, height, width):
    """uv [N,2] float32 projections, centres [N,3] float32 -> (pix int32 [N], rng float32 [N]); one voxel at a time, as written."""
    n = uv.shape[0]
    pix = np.full(n, -1, dtype=np.int32)
    rng = np.empty(n, dtype=np.float32)
    for i in range(n):
        u, v = float(uv[i, 0]), float(uv[i, 1])
        if math.isfinite(u) and math.isfinite(v):
            x, y = math.floor(u + 0.5), math.floor(v + 0.5)
            if 0 <= x < width and 0 <= y < height:
                pix[i] = y * width + x
        cx, cy, cz = (float(c) for c in centres[i])
        rng[i] = np.float32(math.sqrt((cx * cx + cy * cy) + cz * cz))
    return pix, rng


def free_mask(depth, pix, rng, height, width, margin, max_depth):
    """depth [B,dh,dw] float32, pix int32 [N], rng float32 [N] -> uint8 [B,N]; float64 arithmetic, one sum and one comparison."""
    B, dh, dw = depth.shape
    p = pix.astype(np.int64)
    seen = (p >= 0) & (p < height * width)
    y, x = np.where(seen, p // width, 0), np.where(seen, p % width, 0)
    py, px = (y * dh) // height, (x * dw) // width
    d = depth[:, py, px].astype(np.float64)                                    # [B,N]
    with np.errstate(invalid="ignore"):
        surface = (d > 0.0) & (d <= float(max_depth))                          # a NaN fails
        blocked = seen[None] & surface & (d + float(margin) < rng.astype(np.float64)[None])
    return np.where(blocked, 0, 1).astype(np.uint8)


def masked_reduction(prob, coord, free, rows_per_frame):
    """prob [rows,N] float32, coord [N,3] float32, free uint8 [rows / rows_per_frame, N] -> (out float64 [rows,8], peak_index int32
    [rows], mag float64 [rows,4]: sum of |terms| of slots 0..3, what a float32 summation bound is relative to)."""
    rows = prob.shape[0]
    c = coord.astype(np.float64)
    out = np.zeros((rows, 8))
    mag = np.zeros((rows, 4))
    idx = np.full(rows, -1, dtype=np.int32)
    for r in range(rows):
        p = prob[r].astype(np.float64)
        f = free[r // rows_per_frame] != 0
        if np.isnan(p).any():
            out[r] = np.nan
            continue
        pf = np.where(f, p, 0.0)
        out[r, 0] = pf.sum()
        out[r, 1:4] = pf @ c
        mag[r, 0] = np.abs(pf).sum()
        mag[r, 1:4] = np.abs(pf) @ np.abs(c)
        if not f.any():
            out[r, 5:8] = np.nan
            continue
        where = np.flatnonzero(f)
        k = where[np.argmax(prob[r][where])]                                   # np.argmax: the first, i.e. lowest free index
        idx[r] = k
        out[r, 4] = prob[r, k]
        out[r, 5:8] = coord[k]
    return out, idx, mag
