"""Numpy restatement of the runner-up poses (include/sceneego_hip.h: se_skeleton_alternatives_f32; csrc/skeleton_pose.hip), operation by
operation: the max-marginals of the max-product pass over the tree and what follows from them.

``dtype`` = float32 is the definition and the kernels must equal it bit for bit; ``dtype`` = float64 is the same recursion for the host
checks (against a brute force over all poses).  Every maximum is the ROW MAX of tests/skeleton_pose_model.py: from 0, a strictly greater
value wins, the lowest index among equals, a NaN never.

    upward     se_skeleton_pose_f32's, unchanged: A_j, M_j at peak_j, e_j, s_j = ldexp(A_j, -e_j), m_j, the pose x*, solved
    downward   joints by depth level, shallowest first (here: j ascending, every parent before its children); d_0 is absent
               mu_0 = s_0;  mu_j = s_j d_j                                              the max-marginal, scaled
               per child c of j:  E_c = p_j [times d_j if j > 0] times m_c' for the other children c' of j ascending
                                  G_c = max E_c at epeak_c, q_c = ilogb(G_c), t_c = ldexp(E_c, -q_c), tbest_c = ldexp(G_c, -q_c)
                                  e3(y) = max over the non-zero taps d with y + d inside of t_c(y + d) w_c(d), lowest tap
                                  step = keep e3(y), jump = uniform tbest_c;  d_c(y) = jump > step ? jump : step
                                  the parent voxel behind d_c(y): epeak_c for a jump, otherwise y + d*
    exponents  Esub_j = e_j + sum over the children of Esub_c;  F_0 = 0, F_c = F_parent + q_c + sum over the siblings c' of Esub_c'
               ln of the max-marginal of j at x = ln mu_j(x) + ln 2 (Esub_j + F_j)
    records    mm_best_a at mm_peak_a: the row max of mu_a;  pose_value_a = mu_a(x*_a);
               alt_value_a at alt_index_a: the row max of mu_a over the voxels whose Chebyshev distance from x*_a is > separation
    walk       anchor a with alt_index_a >= 0: x_a = alt_index_a; up to the root along the parent voxels behind d_u(x_u); then
               j = 1..J-1 ascending and not yet set: the predecessor of upward edge j at x_parent(j), as in the pose's back-walk
    fallback   a frame that is not solved, or with some G_c not a finite number > 0: complete False, the fills of the header
"""
import numpy as np

from skeleton_pose_model import radius_of, shell_max, tap_voxel
from skeleton_prior_model import children
from volume_viterbi_model import row_max


def _scaled(row, dtype):
    """(max, peak, exponent, best, alive, the row scaled by 2^-exponent)."""
    M, pk = row_max(row[None])
    M, pk = M[0], int(pk[0])
    alive = bool(np.isfinite(M) and M > 0)
    e = int(np.frexp(M)[1] - 1) if alive else 0
    best = np.ldexp(M, -e) if alive else dtype(np.nan)
    return M, pk, e, dtype(best), alive, np.ldexp(row, -e).astype(dtype)


def _edge(row, w, G, R, keep, uniform, dtype):
    """The message of ``row`` through the shell ``w`` and what the walks need of it."""
    M, pk, e, best, alive, s = _scaled(row, dtype)
    e3, arg = shell_max(s, w, G, R, dtype)
    step = keep * e3
    jump = uniform * best
    take = jump > step                                               # a NaN jump never takes it
    return {"M": M, "peak": pk, "e": e, "best": best, "alive": alive, "s": s, "arg": arg, "take": take,
            "out": np.where(take, jump, step).astype(dtype)}


def _behind(edge, x, G, R):
    """(the voxel behind the message ``edge`` at x, jumped)."""
    if edge["take"][x]:
        return edge["peak"], True
    if edge["arg"][x] >= 0:
        return int(tap_voxel(x, int(edge["arg"][x]), G, R)), False
    return edge["peak"], False                                       # step = jump = 0: not reached from a value > 0


def exponent_sums(parents, exponent, down_exponent):
    """(Esub [..., J], F [..., J]) int64 from the exponents the device returns."""
    e, q = np.asarray(exponent, dtype=np.int64), np.asarray(down_exponent, dtype=np.int64)
    J = len(parents)
    ch = children(parents)
    Esub = e.copy()
    for j in range(J - 1, 0, -1):
        Esub[..., parents[j]] += Esub[..., j]
    F = np.zeros_like(e)
    for c in range(1, J):
        j = parents[c]
        F[..., c] = F[..., j] + q[..., c] + sum(Esub[..., o] for o in ch[j] if o != c)
    return Esub, F


def window_mask(x, G, separation):
    """[N] bool: the voxels whose Chebyshev distance in voxel indices from the voxel ``x`` is > separation."""
    n = np.arange(G ** 3)
    far = np.maximum(np.maximum(np.abs(n // (G * G) - x // (G * G)), np.abs(n // G % G - x // G % G)), np.abs(n % G - x % G))
    return far > separation


def skeleton_alternatives_model(prob, taps, parents, G, floor, separation, dtype=np.float32):
    """``prob`` [F, J, N] float32, ``taps`` [J, (2R+1)^3] float32.  Returns a dict of what the device returns - ``index``, ``jumped``,
    ``exponent`` [F, J], ``best_root``, ``solved`` [F] (the pose's), ``down_exponent``, ``mm_peak``, ``alt_index`` [F, J] int32,
    ``mm_best``, ``pose_value``, ``alt_value`` [F, J] ``dtype``, ``alt_pose``, ``alt_jumped`` [F, J, J] int32, ``complete`` [F] bool,
    ``max_marginals`` [F, J, N] ``dtype`` - and of what the caller derives in float64: ``log_score`` [F], ``log_mm_best``,
    ``alt_log_score``, ``margin`` [F, J], ``log_max_marginals`` [F, J, N]."""
    dtype = np.dtype(dtype).type
    prob, taps = np.asarray(prob), np.asarray(taps)
    assert prob.dtype == np.float32 and prob.ndim == 3 and taps.dtype == np.float32
    F, J, N = prob.shape
    assert N == G ** 3 and len(parents) == J and taps.shape[0] == J and int(separation) == separation and separation >= 0
    assert parents[0] == 0 and all(0 <= parents[j] < j for j in range(1, J))
    R = radius_of(taps)
    ch = children(parents)
    fl = dtype(np.float32(floor))
    keep, uniform = dtype(1.0) - fl, fl / dtype(N)
    nan = dtype(np.nan)
    out = {"index": np.empty((F, J), dtype=np.int32), "jumped": np.zeros((F, J), dtype=np.int32),
           "exponent": np.zeros((F, J), dtype=np.int32), "best_root": np.full(F, nan, dtype=dtype), "solved": np.zeros(F, dtype=bool),
           "down_exponent": np.zeros((F, J), dtype=np.int32), "mm_best": np.full((F, J), nan, dtype=dtype),
           "pose_value": np.full((F, J), nan, dtype=dtype), "alt_value": np.full((F, J), nan, dtype=dtype),
           "mm_peak": np.full((F, J), -1, dtype=np.int32), "alt_index": np.full((F, J), -1, dtype=np.int32),
           "alt_pose": np.full((F, J, J), -1, dtype=np.int32), "alt_jumped": np.zeros((F, J, J), dtype=np.int32),
           "complete": np.zeros(F, dtype=bool), "max_marginals": prob.astype(dtype)}
    for f in range(F):
        p = prob[f].astype(dtype)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            # upward
            up = [None] * J
            for j in range(J - 1, -1, -1):
                A = p[j].copy()
                for c in ch[j]:
                    A = A * up[c]["out"]
                if j > 0:
                    up[j] = _edge(A, taps[j], G, R, keep, uniform, dtype)
                else:
                    M, pk, e, best, alive, s = _scaled(A, dtype)
                    up[0] = {"M": M, "peak": pk, "e": e, "best": best, "alive": alive, "s": s}
            if not all(u["alive"] for u in up):
                out["index"][f] = row_max(p)[1]
                continue
            x = np.empty(J, dtype=np.int64)
            x[0] = up[0]["peak"]
            for j in range(1, J):
                x[j], out["jumped"][f, j] = _behind(up[j], int(x[parents[j]]), G, R)
            out["index"][f], out["exponent"][f] = x, [u["e"] for u in up]
            out["best_root"][f], out["solved"][f] = up[0]["best"], True
            # downward
            down, mu = [None] * J, [None] * J
            mu[0] = up[0]["s"]
            for j in range(J):
                if j > 0:
                    mu[j] = up[j]["s"] * down[j]["out"]
                for c in ch[j]:
                    E = p[j].copy()
                    if j > 0:
                        E = E * down[j]["out"]
                    for o in ch[j]:
                        if o != c:
                            E = E * up[o]["out"]
                    down[c] = _edge(E, taps[c], G, R, keep, uniform, dtype)
        if not all(down[c]["alive"] for c in range(1, J)):
            continue
        out["complete"][f] = True
        out["down_exponent"][f, 1:] = [down[c]["e"] for c in range(1, J)]
        out["max_marginals"][f] = np.stack(mu)
        for a in range(J):
            best, peak = row_max(mu[a][None])
            out["mm_best"][f, a], out["mm_peak"][f, a] = best[0], peak[0]
            out["pose_value"][f, a] = mu[a][x[a]]
            with np.errstate(invalid="ignore"):
                masked = np.where(window_mask(int(x[a]), G, separation), mu[a], dtype(0))
            value, at = row_max(masked[None])
            out["alt_value"][f, a], out["alt_index"][f, a] = value[0], at[0]
            if at[0] < 0:
                continue
            y = np.full(J, -1, dtype=np.int64)
            y[a] = at[0]
            u = a
            while u > 0:
                y[parents[u]], out["alt_jumped"][f, a, u] = _behind(down[u], int(y[u]), G, R)
                u = parents[u]
            for j in range(1, J):
                if y[j] < 0:
                    y[j], out["alt_jumped"][f, a, j] = _behind(up[j], int(y[parents[j]]), G, R)
            out["alt_pose"][f, a] = y
    out.update(derive(out, parents))
    return out


def derive(out, parents):
    """float64, from the device's outputs: ``log_score`` [F], ``log_mm_best``, ``alt_log_score``, ``margin`` [F, J] (+inf where a
    complete frame has no alternative, NaN where not complete) and, with ``max_marginals`` present, ``log_max_marginals`` [F, J, N]."""
    ln2 = np.log(2.0)
    Esub, Fd = exponent_sums(parents, out["exponent"], out["down_exponent"])
    shift = ln2 * (Esub + Fd).astype(np.float64)
    complete = np.asarray(out["complete"]).astype(bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = {"log_score": np.log(np.asarray(out["best_root"], dtype=np.float64)) + ln2 * np.asarray(out["exponent"], dtype=np.float64).sum(axis=1),
               "log_mm_best": np.log(np.asarray(out["mm_best"], dtype=np.float64)) + shift}
        has = np.asarray(out["alt_index"]) >= 0
        alt = np.log(np.asarray(out["alt_value"], dtype=np.float64))
        res["alt_log_score"] = np.where(has, alt + shift, np.where(complete[:, None], -np.inf, np.nan))
        res["margin"] = np.where(has, np.log(np.asarray(out["mm_best"], dtype=np.float64)) - alt,
                                 np.where(complete[:, None], np.inf, np.nan))
        if "max_marginals" in out:
            res["log_max_marginals"] = np.log(np.asarray(out["max_marginals"], dtype=np.float64)) + shift[..., None]
    return res
