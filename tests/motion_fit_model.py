"""Float64 numpy model of the transition statistics (include/sceneego_hip.h: se_volume_transition_stats_f32; csrc/volume_filter.hip)
and of the whole EM loop of sceneego_amd/motion_fit.py, built on tests/volume_filter_model.py and tests/volume_smoother_model.py.

It takes the float32 inputs the kernel takes (volumes, filtered beliefs, restart flags, taps, state) and restates the definition.
With w' the taps reversed and m'[d] = d d w'[d] (exact here; the kernel rounds the product to float32 once), walking the frames from
last to first with the backward belief r of the smoother's model:

    linked:      q0 = blur3(r_{t+1}; w', w', w')
                 q2 = blur3(r_{t+1}; m', w', w') + blur3(r_{t+1}; w', m', w') + blur3(r_{t+1}; w', w', m')
                 u = (1 - floor) q0 + floor / N,  a = p_t u,  s = sum a,  r_t = a / s   (s not a finite number > 0: r_t = p_t)
                 stats = { S = sum b_t u,  s,  A0 = sum b_t q0,  A2 = sum b_t q2,  Bsum = sum b_t,  Rsum = sum r_{t+1} }
    not linked:  r_t = p_t bit for bit, the six stats NaN

r is carried in float64: the exact recursion on the float32 inputs, not an emulation of the kernel's roundings.
"""
import numpy as np

from sceneego_amd import motion_fit
from sceneego_amd.volume_filter import gaussian_taps
from volume_filter_model import blur_axis, volume_filter_model


def blur3_per_axis(x, wk, wj, wi, G):
    """``x`` [..., G^3] float64 -> the separable correlation along k with ``wk``, then j with ``wj``, then i with ``wi``."""
    v = x.reshape(x.shape[:-1] + (G, G, G))
    nd = v.ndim
    for axis, w in ((nd - 1, wk), (nd - 2, wj), (nd - 3, wi)):
        v = blur_axis(v, np.asarray(w, dtype=np.float64), axis)
    return v.reshape(x.shape)


def squared_taps(taps):
    """(w', m'): the float32 taps reversed and m'[d] = d d w'[d], exact in float64 (the kernel rounds the product to float32 once:
    that rounding is the kernel's, and the GPU test's bound has a term for it)."""
    rev = np.asarray(taps, dtype=np.float32)[::-1].astype(np.float64)
    R = (len(rev) - 1) // 2
    d = np.arange(-R, R + 1, dtype=np.float64)
    return rev, d * d * rev


def transition_stats_model(prob, belief, restarted, taps, G, floor, state=None, have_link=None):
    """``prob`` [T, rows, N] float32, ``belief`` [T, rows, N] float32 (what the kernel takes) or float64 (the filter model's own),
    ``restarted`` [T, rows], ``taps`` [2R+1] float32 (the filter's), ``state`` None or [rows, N] (r of the frame behind the last one),
    ``have_link`` None or bool [rows].  Returns a dict: ``stats`` [T, rows, 6] float64 (NaN where not linked), ``linked`` [T, rows]
    bool, ``r`` [T, rows, N] float64 (``r[0]`` is the state for the call over the frames before these), ``q0`` and ``q2`` [T, rows, N]
    (zeros where not linked)."""
    prob, belief = np.asarray(prob), np.asarray(belief)
    assert prob.dtype == np.float32 and belief.dtype in (np.float32, np.float64) and prob.ndim == 3 and prob.shape == belief.shape
    T, rows, N = prob.shape
    assert N == G ** 3 and np.asarray(taps).dtype == np.float32 and len(taps) % 2 == 1
    restarted = np.asarray(restarted) != 0
    eps = float(np.float32(floor))
    w, m = squared_taps(taps)
    link_last = np.zeros(rows, dtype=bool) if have_link is None else np.asarray(have_link) != 0
    r = np.zeros((rows, N)) if state is None else np.asarray(state, dtype=np.float64).copy()
    out = {"stats": np.full((T, rows, 6), np.nan), "linked": np.zeros((T, rows), dtype=bool), "r": np.empty((T, rows, N)),
           "q0": np.zeros((T, rows, N)), "q2": np.zeros((T, rows, N))}
    for t in range(T - 1, -1, -1):
        p, b = prob[t].astype(np.float64), belief[t].astype(np.float64)
        linked = link_last if t == T - 1 else ~restarted[t + 1]
        new_r = p.copy()
        idx = np.flatnonzero(linked)
        if idx.size:
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                q0 = blur3_per_axis(r[idx], w, w, w, G)
                q2 = blur3_per_axis(r[idx], m, w, w, G) + blur3_per_axis(r[idx], w, m, w, G) + blur3_per_axis(r[idx], w, w, m, G)
                u = (1.0 - eps) * q0 + eps / N
                a = p[idx] * u
                s = a.sum(axis=1)
                ok = np.isfinite(s) & (s > 0)
                new_r[idx[ok]] = a[ok] / s[ok, None]
                out["stats"][t, idx] = np.stack([(b[idx] * u).sum(axis=1), s, (b[idx] * q0).sum(axis=1), (b[idx] * q2).sum(axis=1),
                                                 b[idx].sum(axis=1), r[idx].sum(axis=1)], axis=1)
            out["q0"][t, idx], out["q2"][t, idx] = q0, q2
        out["linked"][t] = linked
        r = new_r
        out["r"][t] = r
    return out


def fit_model(prob, coord, G, side, sigma, radius, floor, iterations=8, tol=0.0, fit_sigma=True, fit_floor=True,
              floor_bounds=(1e-6, 0.5)):
    """The EM loop of ``MotionModelFit.fit`` over the float64 models: ``prob`` [T, rows, N] float32 is one track pushed whole.  The
    loop, the stop test and the M-step are the package's own (``motion_fit.em_loop``); the forward pass and the statistics are the
    models.  Returns the dict of ``fit`` with ``stats`` and ``linked`` of the last E-step added."""
    h = float(side) / G
    iterations, tol, floor_bounds = motion_fit.check_fit_args(iterations, tol, floor_bounds)
    last = {}

    def e_step(sigma, floor, want_stats):
        taps = gaussian_taps(sigma, radius, h)
        belief, _, evidence, restarted = volume_filter_model(prob, coord, taps, G, floor)
        if not want_stats:
            return evidence, restarted, None, None
        m = transition_stats_model(prob, belief, restarted, taps, G, floor)
        last["stats"], last["linked"] = m["stats"], m["linked"]
        return evidence, restarted, m["stats"], m["linked"]

    result = motion_fit.em_loop(e_step, float(sigma), float(floor), G, int(radius), h, iterations, tol, fit_sigma, fit_floor, floor_bounds)
    result.update(last)
    return result
