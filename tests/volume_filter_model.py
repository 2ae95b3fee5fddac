"""Float64 numpy model of the grid Bayes filter (include/sceneego_hip.h: se_volume_filter_f32; csrc/volume_filter.hip).

It takes the float32 inputs the kernel takes (probabilities, coordinates, taps, state) and restates the definition:

    q = blur3(b)                     separable, taps w[-R..R], along k, then j, then i; zero-padded
    u = (1 - floor) q + floor / N    (floor rounded to float32 first: the value the kernel is given)
    a = p u,  Z = sum a,  b' = a / Z
    restart (b' = p bit for bit) where the row has no prior or Z is not a finite number > 0

The belief is carried from frame to frame in float64: the model is the exact recursion on the float32 inputs, not an emulation of
the kernel's roundings.
"""
import numpy as np


def blur_axis(x, w, axis):
    """Zero-padded correlation of ``x`` with the symmetric-or-not taps ``w`` [2R+1] along ``axis``: out[n] = sum_d w[d] x[n + d]."""
    R = (len(w) - 1) // 2
    n = x.shape[axis]
    out = np.zeros_like(x)
    for d in range(-R, R + 1):
        lo, hi = max(0, -d), min(n, n - d)          # the outputs whose tap d stays inside
        if lo >= hi or w[d + R] == 0.0:
            continue
        dst = [slice(None)] * x.ndim
        src = [slice(None)] * x.ndim
        dst[axis] = slice(lo, hi)
        src[axis] = slice(lo + d, hi + d)
        out[tuple(dst)] += w[d + R] * x[tuple(src)]
    return out


def blur3(b, taps, G):
    """``b`` [..., G^3] float64 -> blur3(b), the same shape: along k, then j, then i."""
    w = np.asarray(taps, dtype=np.float64)
    v = b.reshape(b.shape[:-1] + (G, G, G))
    nd = v.ndim
    for axis in (nd - 1, nd - 2, nd - 3):
        v = blur_axis(v, w, axis)
    return v.reshape(b.shape)


def volume_filter_model(prob, coord, taps, G, floor, state=None, have_prior=None):
    """``prob`` [T, rows, N] float32, ``coord`` [N, 3] float32, ``taps`` [2R+1] float32, ``state`` None or [rows, N] (the belief
    before frame 0: float32 or the float64 a previous call returned), ``have_prior`` None (no row has one) or bool [rows].
    Returns (belief [T, rows, N] float64, joints [T, rows, 3] float64, evidence [T, rows] float64, restarted [T, rows] bool)."""
    prob = np.asarray(prob)
    assert prob.dtype == np.float32 and prob.ndim == 3
    T, rows, N = prob.shape
    assert N == G ** 3 and np.asarray(taps).dtype == np.float32 and len(taps) % 2 == 1
    c = np.asarray(coord, dtype=np.float64).reshape(N, 3)
    eps = float(np.float32(floor))
    prior = np.zeros(rows, dtype=bool) if have_prior is None else np.asarray(have_prior, dtype=bool).copy()
    b = np.zeros((rows, N)) if state is None else np.asarray(state, dtype=np.float64).copy()
    belief = np.empty((T, rows, N))
    joints = np.empty((T, rows, 3))
    evidence = np.full((T, rows), np.nan)
    restarted = np.zeros((T, rows), dtype=bool)
    for t in range(T):
        p = prob[t].astype(np.float64)
        new = p.copy()                                   # a restart: exactly p
        restarted[t] = True
        idx = np.flatnonzero(prior)
        if idx.size:
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                u = (1.0 - eps) * blur3(b[idx], taps, G) + eps / N
                a = p[idx] * u
                Z = a.sum(axis=1)
                evidence[t, idx] = Z
                ok = np.isfinite(Z) & (Z > 0)
                new[idx[ok]] = a[ok] / Z[ok, None]
            restarted[t, idx[ok]] = False
        b = new
        belief[t] = b
        with np.errstate(invalid="ignore", over="ignore"):
            joints[t] = b @ c
        prior[:] = True
    return belief, joints, evidence, restarted
