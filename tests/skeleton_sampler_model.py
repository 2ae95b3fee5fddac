"""Numpy model of the pose sampler (include/sceneego_hip.h: se_skeleton_upward_f32, se_skeleton_sample_f32; csrc/skeleton_sample.hip):
ancestral sampling from the posterior of the coupling's own model, restated so that it has one right answer.

    posterior   prod_j p_j(x_j) prod_c F_c(x_parent(c), x_c), normalised;  F_c(x, y) = (1 - floor) w_c(y - x) + floor / N for y inside
                the grid: CORRELATE's orientation (skeleton_prior_model.corr_direct), the child is y = x + d with weight taps[c][d], no
                tap reversal
    upward      A_j = p_j prod_{c in ch(j)} U_c,  s_j = sum A_j (also j = 0),  U_j = (1 - floor) corr(A_j, w_j) / s_j + floor / N
    draws       x_0 ~ A_0;  x_c ~ A_c(y) F_c(x_parent(c), y) for c = 1..J-1 ascending

``upward_model`` is the exact recursion in float64 on the float32 inputs, as skeleton_prior_model is.  ``skeleton_sample_model`` takes
the float32 ``A`` the sampler takes and is compared with the kernel BIT FOR BIT: everything is float64 with one rounding per operation
and every sum is SEQUENTIAL in ascending index (``np.cumsum``, never ``np.sum``, whose pairwise order is numpy's own).  Philox, the
uniforms, the categorical draw and the three levels of sums of a volume are volume_sampler_model's, imported, not restated.
"""
import numpy as np

from skeleton_prior_model import children, corr_direct
from volume_sampler_model import (FRESH, JUMP, STEP, Frame, constants, global_law, last_positive, mass_ok, masses, uniforms,
                                  window_draw)

__all__ = ["STEP", "JUMP", "FRESH", "upward_model", "skeleton_sample_model", "conditional_masses", "edge_factor", "edge_constants",
           "Volume", "window"]


def _radius(taps):
    W = round(taps.shape[-1] ** (1.0 / 3.0))
    assert W ** 3 == taps.shape[-1] and W % 2 == 1
    return (W - 1) // 2


def edge_constants(floor, N, wide=False):
    """keep and uniform of the edge factor.  The definition's: 1 - floor and floor / N formed in float32, as the coupling's kernels
    form them (volume_sampler_model.constants).  ``wide``: the same two of the float32 floor formed in float64, as
    skeleton_prior_model carries them; the two differ by a rounding of float32, 6e-8, so a comparison to 1e-12 with that model
    (the marginals of the joint law) takes its constants on both sides."""
    if not wide:
        return constants(floor, N)
    eps = float(np.float32(floor))
    return 1.0 - eps, eps / N


# ------------------------------------------------------------------------------------------------------------------ the upward pass
def upward_model(prob, taps, parents, G, floor, wide=False):
    """``prob`` [F, J, N] float32, ``taps`` [J, (2R+1)^3] float32 -> (A [F, J, N] float64, s [F, J] float64 with s_0 = sum A_0, valid [F]
    bool: every s_j a finite number > 0).  floor is rounded to float32 first: the value the kernel is given; ``wide``: edge_constants."""
    prob, taps = np.asarray(prob), np.asarray(taps)
    assert prob.dtype == np.float32 and prob.ndim == 3 and taps.dtype == np.float32
    F, J, N = prob.shape
    assert N == G ** 3 and len(parents) == J and taps.shape[0] == J
    assert parents[0] == 0 and all(0 <= parents[j] < j for j in range(1, J))
    R = _radius(taps)
    ch = children(parents)
    keep, uniform = edge_constants(floor, N, wide)
    A = np.empty((F, J, N))
    s = np.empty((F, J))
    for f in range(F):
        p = prob[f].astype(np.float64)
        U = [None] * J
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for j in range(J - 1, -1, -1):
                a = p[j].copy()
                for k in ch[j]:
                    a = a * U[k]
                A[f, j] = a
                s[f, j] = np.cumsum(a)[-1]
                if j:
                    U[j] = keep * corr_direct(a, taps[j], G, R) / s[f, j] + uniform
    return A, s, (np.isfinite(s) & (s > 0)).all(axis=1)


# ------------------------------------------------------------------------------------------------------------------ one volume
class Volume(Frame):
    """``Frame``'s three levels of sums of one volume A_j [G^3].  float32: the sampler's input, ``Frame`` itself.  float64: the same
    sums of an unrounded A_j, for the tests of the law that must not carry the rounding of A_j to float32."""

    def __init__(self, a, G):
        a = np.asarray(a)
        if a.dtype == np.float32:
            super().__init__(a, G)
            return
        assert a.dtype == np.float64 and a.shape == (G ** 3,)
        self.G = G
        self.b = a.reshape(G, G, G)
        self.ck = np.cumsum(self.b, axis=2)
        self.Rs = self.ck[:, :, -1]
        self.cj = np.cumsum(self.Rs, axis=1)
        self.P = self.cj[:, -1]
        self.ci = np.cumsum(self.P)
        self.total = self.ci[-1]
        self.last_k, self.last_j, self.last_i = last_positive(self.b), last_positive(self.Rs), last_positive(self.P)


def window(vol, x, w3, R):
    """The window sums of child volume ``vol`` given the parent's voxel ``x`` with the child's taps ``w3`` [2R+1, 2R+1, 2R+1] float64:
    y = x + d, clipped to the grid; v(d) = A(x + d) w(d), exactly 0 where the tap is 0 whatever A holds there; r[di][dj] = sum_dk v,
    q[di] = sum_dj r, Wsum = sum_di q.  The keys are those of volume_sampler_model's window, so its ``masses`` and ``window_draw``
    take it: ti = q, tj = r, tk = v and their running sums."""
    G = vol.G
    xi, xj, xk = x // (G * G), (x // G) % G, x % G
    lo = [max(-R, -c) for c in (xi, xj, xk)]
    n = [min(R, G - 1 - c) - l + 1 for c, l in zip((xi, xj, xk), lo)]
    sub = vol.b[xi + lo[0]:xi + lo[0] + n[0], xj + lo[1]:xj + lo[1] + n[1], xk + lo[2]:xk + lo[2] + n[2]]
    ws = w3[lo[0] + R:lo[0] + R + n[0], lo[1] + R:lo[1] + R + n[1], lo[2] + R:lo[2] + R + n[2]]
    with np.errstate(invalid="ignore", over="ignore"):
        tk = np.where(ws == 0.0, 0.0, sub * ws)
        ck = np.cumsum(tk, axis=2)
        tj = ck[:, :, -1]
        cj = np.cumsum(tj, axis=1)
        ti = cj[:, -1]
        ci = np.cumsum(ti)
    return {"base": (xi + lo[0], xj + lo[1], xk + lo[2]), "n": n, "tk": tk, "ck": ck, "tj": tj, "cj": cj, "ti": ti, "ci": ci,
            "Wsum": ci[-1]}


# ------------------------------------------------------------------------------------------------------------------ the chain
def skeleton_sample_model(A, valid, taps, parents, G, R, floor, samples, first_sample=0, first_frame=0, seed=0):
    """``A`` [F, J, N] float32 (the upward products), ``valid`` None or [F], ``taps`` [J, (2R+1)^3] float32.  Returns a dict: ``index``
    and ``kind`` [samples, F, J] int32.  Vectorised over the samples of a (frame, joint): the sums of a volume are shared by its
    samples, and samples whose parent stands on the same voxel share one window."""
    A, taps = np.asarray(A), np.asarray(taps)
    assert A.dtype == np.float32 and A.ndim == 3 and taps.dtype == np.float32
    F, J, N = A.shape
    assert N == G ** 3 and len(parents) == J and taps.shape == (J, (2 * R + 1) ** 3)
    keep, uniform = constants(floor, N)
    S = int(samples)
    W = 2 * R + 1
    index = np.full((S, F, J), -1, dtype=np.int32)
    kind = np.full((S, F, J), FRESH, dtype=np.int32)
    gs = np.arange(first_sample, first_sample + S)
    for f in range(F):
        if valid is not None and not valid[f]:
            continue                                           # -1 and kind 2 for every joint and sample; nothing of A is read
        for j in range(J):
            vol = Volume(A[f, j], G)
            w3 = taps[j].astype(np.float64).reshape(W, W, W)
            u0, u1, u2, u3 = uniforms(seed, gs, first_frame + f, j)
            x = index[:, f, parents[j]].astype(np.int64) if j else np.full(S, -1, dtype=np.int64)
            mode = np.full(S, FRESH, dtype=np.int32)
            y = np.full(S, -1, dtype=np.int64)
            for xv in np.unique(x[x >= 0]):
                grp = np.flatnonzero(x == xv)
                win = window(vol, int(xv), w3, R)
                step, jump, mass = masses(vol, win, keep, uniform)
                if not mass_ok(mass):
                    continue                                   # drawn as an unlinked joint
                jumps = u0[grp] * mass >= step
                mode[grp] = np.where(jumps, JUMP, STEP)
                st = grp[~jumps]
                y[st] = window_draw(win, G, u1[st], u2[st], u3[st])
            glob = np.flatnonzero(mode != STEP)
            y[glob] = vol.global_draw(u1[glob], u2[glob], u3[glob])
            index[:, f, j], kind[:, f, j] = y, mode
    return {"index": index, "kind": kind}


# ------------------------------------------------------------------------------------------------------------------ the law
def edge_factor(w, G, R, floor, wide=False):
    """The dense edge factor F[x, y] = keep w(y - x) + uniform over all pairs of voxels, from the taps ``w`` [(2R+1)^3] float32; keep and
    uniform as the definition forms them (float32, then float64), or ``wide`` (edge_constants)."""
    N, W = G ** 3, 2 * R + 1
    w3 = np.asarray(w).astype(np.float64).reshape(W, W, W)
    keep, uniform = edge_constants(floor, N, wide)
    c = np.stack(np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij"), axis=-1).reshape(N, 3)
    d = c[None, :, :] - c[:, None, :]                          # [x, y]: y - x
    inside = (np.abs(d) <= R).all(axis=-1)
    dd = np.clip(d + R, 0, W - 1)
    return keep * np.where(inside, w3[dd[..., 0], dd[..., 1], dd[..., 2]], 0.0) + uniform


def conditional_masses(a_c, x, w, G, R, floor, wide=False):
    """What the model's own sums imply for child volume ``a_c`` [N] (float32, or float64 for the law tests) given the parent's voxel
    ``x`` (None: a global draw, the root's): a dict of ``step``, ``jump``, ``mass``, the probabilities ``window`` [N] of a step's draw
    (the three window levels; 0 outside the window), ``global`` [N] of a global draw (the three levels of the volume) and ``law`` [N],
    the probability of every voxel: (step / mass) window + (jump / mass) global.  ``wide``: edge_constants."""
    N, W = G ** 3, 2 * R + 1
    vol = Volume(a_c, G)
    glob = global_law(vol)
    if x is None:
        return {"step": 0.0, "jump": vol.total, "mass": vol.total, "window": np.zeros(N), "global": glob, "law": glob}
    win = window(vol, int(x), np.asarray(w).astype(np.float64).reshape(W, W, W), R)
    keep, uniform = edge_constants(floor, N, wide)
    step, jump, mass = masses(vol, win, keep, uniform)
    with np.errstate(invalid="ignore", divide="ignore"):
        pa = win["ti"] / win["Wsum"] if win["Wsum"] > 0 else np.zeros_like(win["ti"])
        pc = np.where(win["ti"][:, None] > 0, win["tj"] / win["ti"][:, None], 0.0)
        pm = np.where(win["tj"][:, :, None] > 0, win["tk"] / win["tj"][:, :, None], 0.0)
    i0, j0, k0 = win["base"]
    n = win["n"]
    inside = np.zeros((G, G, G))
    inside[i0:i0 + n[0], j0:j0 + n[1], k0:k0 + n[2]] = pa[:, None, None] * pc[:, :, None] * pm
    inside = inside.reshape(-1)
    return {"step": step, "jump": jump, "mass": mass, "window": inside, "global": glob,
            "law": (step / mass) * inside + (jump / mass) * glob}
