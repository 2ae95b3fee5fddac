"""The exact model of se_joint_modes_f32 (include/sceneego_hip.h): a restatement of the definition, nothing else.

Fed the SAME float32 ``prob`` and ``coord`` the kernel gets.  The mode mask is 26 shifted key comparisons, the selection a sort by
key, the window sums an explicit loop in ascending flat index in float64 with one float32 rounding at the end."""
import itertools

import numpy as np

QNAN_BITS = 0x7FC00000


def qnan():
    return np.array([QNAN_BITS], dtype=np.uint32).view(np.float32)[0]


def mode_mask(p, G, min_prob=0.0):
    """p [G,G,G] float32 -> bool [G,G,G]: p > 0, p >= min_prob and the key (p, -n) greater than that of every neighbour in the grid."""
    p = np.asarray(p, dtype=np.float32).reshape(G, G, G)
    n = np.arange(G ** 3, dtype=np.int64).reshape(G, G, G)
    pad_p = np.full((G + 2,) * 3, -np.inf, dtype=np.float32)
    pad_n = np.full((G + 2,) * 3, -1, dtype=np.int64)             # -1: the neighbour does not exist
    pad_p[1:-1, 1:-1, 1:-1] = p
    pad_n[1:-1, 1:-1, 1:-1] = n
    with np.errstate(invalid="ignore"):
        mask = (p > 0) & (p >= np.float32(min_prob))
        for di, dj, dk in itertools.product((-1, 0, 1), repeat=3):
            if (di, dj, dk) == (0, 0, 0):
                continue
            q = pad_p[1 + di:G + 1 + di, 1 + dj:G + 1 + dj, 1 + dk:G + 1 + dk]
            m = pad_n[1 + di:G + 1 + di, 1 + dj:G + 1 + dj, 1 + dk:G + 1 + dk]
            greater = (p > q) | ((p == q) & (n < m))              # key (p, -n) > key (q, -m)
            mask &= (m < 0) | greater
    return mask


def joint_modes_model(prob, coord, G, K, radius, min_prob=0.0):
    """prob [rows, G^3] float32, coord [G^3, 3] float32 -> (modes [rows,K,8] float32, index [rows,K] int32, count [rows] int32,
    total [rows] int32), as the header defines them."""
    prob = np.ascontiguousarray(prob, dtype=np.float32).reshape(-1, G ** 3)
    coord = np.ascontiguousarray(coord, dtype=np.float32).reshape(G ** 3, 3)
    rows = prob.shape[0]
    nan = qnan()
    modes = np.zeros((rows, K, 8), dtype=np.float32)
    modes[:, :, 5:] = nan
    index = np.full((rows, K), -1, dtype=np.int32)
    count = np.zeros(rows, dtype=np.int32)
    total = np.zeros(rows, dtype=np.int32)
    c64 = coord.astype(np.float64)
    for r in range(rows):
        p = prob[r]
        if np.isnan(p).any():
            modes[r] = nan
            count[r] = total[r] = -1
            continue
        idx = np.flatnonzero(mode_mask(p, G, min_prob).reshape(-1))
        total[r] = idx.size
        order = np.lexsort((idx, -p[idx].astype(np.float64)))     # p descending, then index ascending
        sel = idx[order][:K]
        count[r] = sel.size
        for s, n in enumerate(sel):
            i, j, k = n // (G * G), (n // G) % G, n % G
            mass = mx = my = mz = 0.0                             # Python floats: float64
            for a in range(max(i - radius, 0), min(i + radius, G - 1) + 1):
                for b in range(max(j - radius, 0), min(j + radius, G - 1) + 1):
                    for c in range(max(k - radius, 0), min(k + radius, G - 1) + 1):   # ascending flat index
                        m = (a * G + b) * G + c
                        pm = float(p[m])
                        mass += pm
                        mx += pm * c64[m, 0]
                        my += pm * c64[m, 1]
                        mz += pm * c64[m, 2]
            modes[r, s, 0] = p[n]
            modes[r, s, 1:5] = np.array([mass, mx, my, mz], dtype=np.float64).astype(np.float32)
            modes[r, s, 5:] = coord[n]
            index[r, s] = n
    return modes, index, count, total
