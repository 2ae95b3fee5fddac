"""Float64 numpy model of the skeleton-coupled joints (include/sceneego_hip.h: se_skeleton_couple_f32, se_shell_correlate_f32;
csrc/skeleton_prior.hip).

It takes the float32 inputs the kernels take (probabilities, coordinates, taps) and restates the definition:

    tree      J joints, parent[j] < j, parent[0] = 0; ch(j) the children of j in ascending order
    corr(a, w)(x) = sum over d with w(d) != 0 and x + d inside the grid of w(d) a(x + d)        zero-padded, exact zeros skipped
    upward    j = J-1 .. 1:   A_j = p_j prod_c U_c,  s_j = sum A_j,  U_j = (1 - floor) corr(A_j, w_j) / s_j + floor / N
    downward  j = 0 .. J-1:   T_j = p_j D_j prod_c U_c (D_0 absent),  Z_j = sum T_j,  b_j = T_j / Z_j,  joints_j = (sum T_j coord) / Z_j
              per child c:    E = p_j D_j prod_{c' != c} U_c',  t_c = sum E,  D_c = (1 - floor) corr(E, w_c) / t_c + floor / N
    fallback  a frame one of whose s_j, t_c, Z_j is not a finite number > 0: b = p exactly, joints = sum p coord, coupled = False;
              the evidence keeps the Z_j as computed

(floor rounded to float32 first: the value the kernel is given).  Everything is carried in float64: the model is the exact recursion on
the float32 inputs, not an emulation of the kernel's roundings.

``method="direct"`` adds one shifted slice per non-zero tap.  ``method="fft"`` computes the same linear correlation through a
zero-padded FFT of size G + 2R and clips negatives to 0: its absolute error is a few 1e-16 of the largest value of ``a``, which is
only harmless with floor > 0, where every message is at least floor / N (it must stay far below that); with floor = 0 a message that
should be exactly 0 would come out as noise.  It is there for the shapes the direct form is too slow for.
"""
import numpy as np


def children(parents):
    return [[c for c in range(1, len(parents)) if parents[c] == j] for j in range(len(parents))]


def corr_direct(a, w, G, R):
    """``a`` [..., G^3] float64, ``w`` [(2R+1)^3] -> corr(a, w), the same shape."""
    W = 2 * R + 1
    v = a.reshape(a.shape[:-1] + (G, G, G))
    out = np.zeros_like(v)
    w3 = np.asarray(w, dtype=np.float64).reshape(W, W, W)
    for di, dj, dk in zip(*np.nonzero(w3)):
        d = (di - R, dj - R, dk - R)
        dst, src = [Ellipsis], [Ellipsis]
        empty = False
        for e in d:
            lo, hi = max(0, -e), min(G, G - e)          # the outputs whose tap stays inside
            if lo >= hi:
                empty = True
            dst.append(slice(lo, hi))
            src.append(slice(lo + e, hi + e))
        if not empty:
            out[tuple(dst)] += w3[di, dj, dk] * v[tuple(src)]
    return out.reshape(a.shape)


def corr_fft(a, w, G, R, cache=None, key=None):
    """The same through a zero-padded FFT (size G + 2R per axis), negatives clipped to 0.  ``cache`` / ``key``: a dict that keeps the
    transformed taps."""
    W, S = 2 * R + 1, G + 2 * R
    K = None if cache is None else cache.get(key)
    if K is None:
        flipped = np.asarray(w, dtype=np.float64).reshape(W, W, W)[::-1, ::-1, ::-1]
        K = np.fft.rfftn(flipped, s=(S, S, S), axes=(0, 1, 2))
        if cache is not None:
            cache[key] = K
    v = a.reshape(a.shape[:-1] + (G, G, G))
    full = np.fft.irfftn(np.fft.rfftn(v, s=(S, S, S), axes=(-3, -2, -1)) * K, s=(S, S, S), axes=(-3, -2, -1))
    out = full[..., R:R + G, R:R + G, R:R + G]           # conv(a, flipped w)(x + R) = sum_d w(d) a(x + d)
    return np.maximum(out, 0.0).reshape(a.shape)


def skeleton_couple_model(prob, coord, taps, parents, G, floor, method="direct"):
    """``prob`` [F, J, N] float32, ``coord`` [N, 3] float32, ``taps`` [J, (2R+1)^3] float32, ``parents`` the tree.
    Returns (beliefs [F, J, N] float64, joints [F, J, 3] float64, evidence [F, J] float64, coupled [F] bool, norms): ``norms`` is a
    dict of the normalisers ``s`` [F, J], ``t`` [F, J] (entry 0 of both NaN: the root sends and receives nothing) and ``Z`` [F, J]."""
    prob = np.asarray(prob)
    taps = np.asarray(taps)
    assert prob.dtype == np.float32 and prob.ndim == 3 and taps.dtype == np.float32
    F, J, N = prob.shape
    assert N == G ** 3 and len(parents) == J and taps.shape[0] == J
    W = round(taps.shape[1] ** (1.0 / 3.0))
    assert W ** 3 == taps.shape[1] and W % 2 == 1
    R = (W - 1) // 2
    assert parents[0] == 0 and all(0 <= parents[j] < j for j in range(1, J))
    ch = children(parents)
    c = np.asarray(coord, dtype=np.float64).reshape(N, 3)
    eps = float(np.float32(floor))
    cache = {}

    def corr(a, j):
        if method == "fft":
            return corr_fft(a, taps[j], G, R, cache, j)
        assert method == "direct"
        return corr_direct(a, taps[j], G, R)

    beliefs = np.empty((F, J, N))
    joints = np.empty((F, J, 3))
    evidence = np.empty((F, J))
    coupled = np.ones(F, dtype=bool)
    s = np.full((F, J), np.nan)
    t = np.full((F, J), np.nan)
    for f in range(F):
        p = prob[f].astype(np.float64)
        U = [None] * J
        D = [None] * J
        T = [None] * J
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for j in range(J - 1, 0, -1):
                A = p[j].copy()
                for k in ch[j]:
                    A = A * U[k]
                s[f, j] = A.sum()
                U[j] = (1.0 - eps) * corr(A, j) / s[f, j] + eps / N
            for j in range(J):
                base = p[j] if j == 0 else p[j] * D[j]
                T[j] = base.copy()
                for k in ch[j]:
                    T[j] = T[j] * U[k]
                evidence[f, j] = T[j].sum()
                for k in ch[j]:
                    E = base.copy()
                    for k2 in ch[j]:
                        if k2 != k:
                            E = E * U[k2]
                    t[f, k] = E.sum()
                    D[k] = (1.0 - eps) * corr(E, k) / t[f, k] + eps / N
            norms = np.concatenate([s[f, 1:], t[f, 1:], evidence[f]])
            ok = bool(np.all(np.isfinite(norms) & (norms > 0)))
            coupled[f] = ok
            for j in range(J):
                beliefs[f, j] = T[j] / evidence[f, j] if ok else p[j]
                joints[f, j] = beliefs[f, j] @ c
    return beliefs, joints, evidence, coupled, {"s": s, "t": t, "Z": evidence.copy()}
