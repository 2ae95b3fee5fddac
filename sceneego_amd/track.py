"""Pick one mode per joint and frame over a sequence (host, numpy float64).

``VoxelNetwork_depth.joint_modes`` says where the peaks of a joint's distribution are in one frame; a sequence says which of them
the joint is: it was near one of them a frame ago.  ``select_modes`` is the smallest honest form of that argument.

WHAT THIS IS.  A convention, not a calibrated tracker: the mass of a mode's window is read as its likelihood, and the joint is
assumed to take an isotropic Gaussian step of sigma = 0.1 m from one frame to the next.  Neither is fitted to or validated against
annotated data, because none ships with the method; the same holds for the thresholds of the scene check and for the masking of
``constrain_to_scene``.  Treat the output as one more hypothesis beside the soft-argmax joint, not as a correction of it."""
from __future__ import annotations

import numpy as np


def select_modes(frames, sigma=0.10, fallback=None):
    """One mode per joint and frame, by dynamic programming.

    ``frames``: a list of T per-frame dicts as ``op.joint_modes_to_numpy`` returns them; ``coord`` [J,K,3], ``mass`` [J,K] and
    ``valid`` [J,K] are read (K may differ between frames).  Per joint j the path k_0 .. k_{T-1} over the VALID modes minimises

        sum_t -ln(mass[t, j, k_t])  +  sum_{t>0} |coord[t, j, k_t] - coord[t-1, j, k_{t-1}]|^2 / (2 sigma^2)

    evaluated in float64 in frame order, ((c + step) + node).  Ties are broken by the lowest mode slot, the last frame first: of
    the minimal paths the one with the lowest slot in the last frame, among those the lowest in the frame before, and so on.
    A frame in which joint j has no valid mode takes ``fallback[t, j]`` ([T,J,3]: the soft-argmax joints) as its single candidate
    with cost 0; ValueError if that happens and ``fallback`` is None.

    Returns ``joints`` [T,J,3] float32 and ``choice`` [T,J] int64: the slot taken, -1 where the fallback was.

    Mass as likelihood and a Gaussian step of ``sigma`` metres per frame are a convention, not calibrated against annotated data."""
    T = len(frames)
    if T == 0:
        raise ValueError("select_modes: no frames")
    sigma = float(sigma)
    if not sigma > 0.0:
        raise ValueError(f"select_modes: sigma = {sigma} must be positive")
    J = int(np.asarray(frames[0]["mass"]).shape[0])
    fb = None
    if fallback is not None:
        fb = np.asarray(fallback, dtype=np.float64)
        if fb.shape != (T, J, 3):
            raise ValueError(f"select_modes: fallback {fb.shape}, expected {(T, J, 3)}")
    inv = 1.0 / (2.0 * sigma * sigma)
    joints = np.empty((T, J, 3), dtype=np.float32)
    choice = np.empty((T, J), dtype=np.int64)
    for j in range(J):
        slots, pos, node = [], [], []              # per frame: candidate slots, positions [n,3], node costs [n]
        for t, f in enumerate(frames):
            valid = np.asarray(f["valid"])[j].astype(bool)
            k = np.flatnonzero(valid)              # ascending slot
            if k.size == 0:
                if fb is None:
                    raise ValueError(f"select_modes: joint {j} has no valid mode in frame {t} and no fallback was given")
                slots.append(np.array([-1], dtype=np.int64))
                pos.append(fb[t, j][None, :])
                node.append(np.zeros(1))
            else:
                slots.append(k.astype(np.int64))
                pos.append(np.asarray(f["coord"], dtype=np.float64)[j, k])
                node.append(-np.log(np.asarray(f["mass"], dtype=np.float64)[j, k]))
        cost = node[0]
        back = []
        for t in range(1, T):
            d = pos[t][None, :, :] - pos[t - 1][:, None, :]                       # [prev, cur, 3]
            step = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * inv
            through = cost[:, None] + step                                         # [prev, cur]
            b = np.argmin(through, axis=0)                                         # the first minimum: the lowest slot
            back.append(b)
            cost = through[b, np.arange(through.shape[1])] + node[t]
        n = int(np.argmin(cost))
        for t in range(T - 1, -1, -1):
            choice[t, j] = slots[t][n]
            joints[t, j] = pos[t][n]
            if t > 0:
                n = int(back[t - 1][n])
    return joints, choice
