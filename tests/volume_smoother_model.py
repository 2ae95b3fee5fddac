"""Float64 numpy model of the filter's backward pass (include/sceneego_hip.h: se_volume_smooth_f32; csrc/volume_filter.hip).

It takes the float32 inputs the kernel takes (volumes, filtered beliefs, restart flags, coordinates, taps, state) and restates the
definition; the beliefs may also be the float64 ones of tests/volume_filter_model.py.  Walking the frames from last to first with a backward belief r per row:

    linked_t   = t is not the last frame and not restarted[t + 1]          (the call's last frame: have_link)
    not linked:  gamma_t = b_t and r_t = p_t bit for bit, smoothed = false, agreement NaN
    linked:      u = (1 - floor) blur3T(r_{t+1}) + floor / N               blur3T = blur3 with the taps reversed; floor rounded to
                 g = b_t u,  S = sum g,  gamma_t = g / S                   float32 first, the value the kernel is given
                 a = p_t u,  s = sum a,  r_t = a / s
                 S not a finite number > 0: gamma_t = b_t, smoothed = false;   s not a finite number > 0: r_t = p_t

r is carried from frame to frame in float64: the model is the exact recursion on the float32 inputs, not an emulation of the kernel's
roundings.
"""
import numpy as np

from volume_filter_model import blur3


def volume_smoother_model(prob, belief, restarted, coord, taps, G, floor, state=None, have_link=None):
    """``prob`` [T, rows, N] float32 and ``belief`` [T, rows, N] float32 (what the kernel takes) or float64 (the filter model's own
    beliefs, unrounded: for the properties of the recursion itself, which hold beyond float32's rounding), ``restarted`` [T, rows]
    (bool or int), ``coord`` [N, 3] float32, ``taps`` [2R+1] float32 (the filter's: reversed here), ``state`` None or [rows, N] (r of the frame behind the last one: float32 or the float64 a
    previous call returned), ``have_link`` None (the last frame is linked to nothing) or bool [rows].  Returns a dict: ``gamma`` and
    ``r`` [T, rows, N] float64, ``joints`` [T, rows, 3], ``agreement`` and ``s`` [T, rows] (NaN where not linked), ``smoothed`` and
    ``linked`` [T, rows] bool; ``r[0]`` is the state for the call over the frames before these."""
    prob, belief = np.asarray(prob), np.asarray(belief)
    assert prob.dtype == np.float32 and belief.dtype in (np.float32, np.float64) and prob.ndim == 3 and prob.shape == belief.shape
    T, rows, N = prob.shape
    assert N == G ** 3 and np.asarray(taps).dtype == np.float32 and len(taps) % 2 == 1
    restarted = np.asarray(restarted) != 0
    assert restarted.shape == (T, rows)
    c = np.asarray(coord, dtype=np.float64).reshape(N, 3)
    eps = float(np.float32(floor))
    rev = np.asarray(taps)[::-1]
    link_last = np.zeros(rows, dtype=bool) if have_link is None else np.asarray(have_link) != 0
    r = np.zeros((rows, N)) if state is None else np.asarray(state, dtype=np.float64).copy()
    out = {"gamma": np.empty((T, rows, N)), "r": np.empty((T, rows, N)), "joints": np.empty((T, rows, 3)),
           "agreement": np.full((T, rows), np.nan), "s": np.full((T, rows), np.nan), "smoothed": np.zeros((T, rows), dtype=bool),
           "linked": np.zeros((T, rows), dtype=bool)}
    for t in range(T - 1, -1, -1):
        p, b = prob[t].astype(np.float64), belief[t].astype(np.float64)
        linked = link_last if t == T - 1 else ~restarted[t + 1]
        gamma, new_r = b.copy(), p.copy()
        idx = np.flatnonzero(linked)
        if idx.size:
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                u = (1.0 - eps) * blur3(r[idx], rev, G) + eps / N
                g, a = b[idx] * u, p[idx] * u
                S, s = g.sum(axis=1), a.sum(axis=1)
                okS, oks = np.isfinite(S) & (S > 0), np.isfinite(s) & (s > 0)
                gamma[idx[okS]] = g[okS] / S[okS, None]
                new_r[idx[oks]] = a[oks] / s[oks, None]
            out["agreement"][t, idx], out["s"][t, idx] = S, s
            out["smoothed"][t, idx[okS]] = True
        out["linked"][t] = linked
        r = new_r
        out["gamma"][t], out["r"][t] = gamma, r
        with np.errstate(invalid="ignore", over="ignore"):
            out["joints"][t] = gamma @ c
    return out
