"""Float64 numpy model of the skeleton model's edge statistics (include/sceneego_hip.h: se_skeleton_edge_stats_f32,
se_shell_moments_f32; csrc/skeleton_prior.hip) and of the fit around them (sceneego_amd/skeleton_fit.py).

The recursion is tests/skeleton_prior_model.py's, on its ``corr_direct`` (or ``corr_fft`` for the shapes the direct form is too slow
for), kept to the point where both A_c and E_c of an edge exist:

    S0 = sum_x E_c(x) corr(A_c, w_c)(x)    S1 = sum_x E_c(x) corr(A_c, w1_c)(x)    S2 = sum_x E_c(x) corr(A_c, w2_c)(x)
    SJ = (floor / N) t_c s_c                a tap with w_c(d) == 0 is skipped in all three blocks

(floor rounded to float32 first: the value the kernel is given).  The tap blocks may be float32, as the kernels take them, or float64,
for the identities that hold exactly only with unrounded blocks.  Everything is carried in float64.

``fit_model`` runs ``skeleton_fit.em_loop`` - the loop ``SkeletonModelFit.fit`` runs - over this model instead of the device pass.
"""
import numpy as np

from sceneego_amd import skeleton_fit
from skeleton_prior_model import children, corr_direct, corr_fft


def shell_moments_model(e, a, w, w1, w2, G, R, method="direct", cache=None, key=None):
    """(S0, S1, S2) of one pair of volumes ``e``, ``a`` [G^3] with the blocks ``w``, ``w1``, ``w2`` [(2R+1)^3].  ``cache`` / ``key``:
    as for ``corr_fft``."""
    w = np.asarray(w, dtype=np.float64)
    keep = w != 0
    out = []
    for k, blk in enumerate((w, w1, w2)):
        blk = np.where(keep, np.asarray(blk, dtype=np.float64), 0.0)
        c = corr_fft(a, blk, G, R, cache, (key, k)) if method == "fft" else corr_direct(a, blk, G, R)
        out.append(float((e * c).sum()))
    return out


def edge_stats_model(prob, taps, taps_r, taps_r2, parents, G, floor, method="direct"):
    """``prob`` [F, J, N] float32, the three tap blocks [J, (2R+1)^3], ``parents`` the tree.  Returns ``stats`` [F, J, 4] float64 (row
    0 zero), ``norms`` [F, J, 3] (s, t, Z; s_0 and t_0 NaN) and ``valid`` [F] bool."""
    prob = np.asarray(prob)
    taps = np.asarray(taps)
    assert prob.dtype == np.float32 and prob.ndim == 3
    F, J, N = prob.shape
    assert N == G ** 3 and len(parents) == J and taps.shape[0] == J
    W = round(taps.shape[1] ** (1.0 / 3.0))
    assert W ** 3 == taps.shape[1] and W % 2 == 1
    R = (W - 1) // 2
    ch = children(parents)
    eps = float(np.float32(floor))
    cache = {}

    def corr(a, j):
        return corr_fft(a, taps[j], G, R, cache, j) if method == "fft" else corr_direct(a, taps[j], G, R)

    stats = np.zeros((F, J, 4))
    norms = np.full((F, J, 3), np.nan)
    valid = np.ones(F, dtype=bool)
    for f in range(F):
        p = prob[f].astype(np.float64)
        A, U, D = [None] * J, [None] * J, [None] * J
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for j in range(J - 1, 0, -1):
                A[j] = p[j].copy()
                for k in ch[j]:
                    A[j] = A[j] * U[k]
                norms[f, j, 0] = A[j].sum()
                U[j] = (1.0 - eps) * corr(A[j], j) / norms[f, j, 0] + eps / N
            for j in range(J):
                base = p[j] if j == 0 else p[j] * D[j]
                T = base.copy()
                for k in ch[j]:
                    T = T * U[k]
                norms[f, j, 2] = T.sum()
                for k in ch[j]:
                    E = base.copy()
                    for k2 in ch[j]:
                        if k2 != k:
                            E = E * U[k2]
                    norms[f, k, 1] = E.sum()
                    D[k] = (1.0 - eps) * corr(E, k) / norms[f, k, 1] + eps / N
                    stats[f, k, :3] = shell_moments_model(E, A[k], taps[k], taps_r[k], taps_r2[k], G, R, method, cache, ("m", k))
                    stats[f, k, 3] = (eps / N) * norms[f, k, 1] * norms[f, k, 0]
            check = np.concatenate([norms[f, 1:, 0], norms[f, 1:, 1], norms[f, :, 2]])
            valid[f] = bool(np.all(np.isfinite(check) & (check > 0)))
    return stats, norms, valid


def fit_model(prob, parents, G, side, lengths, tau, floor, iterations=6, tol=0.0, fit_lengths=True, fit_tau=True, fit_floor=True,
              floor_bounds=(1e-6, 0.5), tau_bounds=None, method="direct"):
    """``SkeletonModelFit.fit`` with the float64 model as its E-step: the same support, the same float32 taps, the same loop."""
    support = skeleton_fit.cut_support(lengths, tau, side / G)

    def e_step(taps, fl):
        return edge_stats_model(prob, taps[0], taps[1], taps[2], parents, G, fl, method)

    return skeleton_fit.em_loop(e_step, support, floor, iterations, tol, fit_lengths, fit_tau, fit_floor, floor_bounds, tau_bounds)
