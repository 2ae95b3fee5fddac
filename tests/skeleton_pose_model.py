"""Numpy restatement of the most probable pose (include/sceneego_hip.h: se_skeleton_pose_f32, se_shell_maxcorr_f32,
se_shell_argmax_i32; csrc/skeleton_pose.hip), operation by operation.

``dtype`` = float32 is the definition: every product is one float32 rounding, numpy keeps float32 gradual underflow, and the kernel
must equal it bit for bit.  ``dtype`` = float64 is the same recursion for the host checks (against a dense max-product over N x N
transition matrices and a brute force, and that the float32 pose is the float64 pose on the test inputs).

    joints by depth level, deepest first (here: j = J-1 .. 0, every child before its parent; the order inside a level is free)
    product    A_j = p_j, then times m_c for each child c ascending, one rounding per factor
    row max    M_j = max A_j from 0, strictly greater wins: lowest index, NaN never; peak_j its index
    rescale    e_j = ilogb(M_j), s_j = ldexp(A_j, -e_j), best_j = ldexp(M_j, -e_j)
    message    e3_j(x) = max over the non-zero taps d with x + d inside of s_j(x + d) w_j(d), from 0, cand > best takes it, the taps in
               ascending index: the argument is the lowest tap index that attains it, -1 where e3_j(x) = 0
               step = keep e3_j(x), jump = uniform best_j; jump > step: m_j(x) = jump, predecessor peak_j with the jump mark;
               otherwise m_j(x) = step, predecessor x + d*
    back-walk  x_0 = peak_0; j = 1..J-1 ascending: x_j = the predecessor of edge j at x_parent(j)
    fallback   some M_j not a finite number > 0: every joint the peak of its own p_j (-1: none), jumped False, exponent 0, best_root and
               log_score NaN, solved False
"""
import numpy as np

from skeleton_prior_model import children
from volume_viterbi_model import row_max


def radius_of(taps):
    W = round(np.asarray(taps).shape[-1] ** (1.0 / 3.0))
    assert W ** 3 == np.asarray(taps).shape[-1] and W % 2 == 1
    return (W - 1) // 2


def shell_max(s, w, G, R, dtype=np.float32):
    """``s`` [..., G^3], ``w`` [(2R+1)^3] float32 -> (e3 [..., G^3] ``dtype``, arg [..., G^3] int32: the lowest tap index that attains
    e3, -1 where e3 = 0)."""
    dtype = np.dtype(dtype).type
    W = 2 * R + 1
    v = np.asarray(s).astype(dtype).reshape(s.shape[:-1] + (G, G, G))
    best = np.zeros(v.shape, dtype=dtype)
    arg = np.full(v.shape, -1, dtype=np.int32)
    wf = np.asarray(w).reshape(-1)
    for tap in np.flatnonzero(wf != 0):                  # ascending tap index: di, then dj, then dk
        d = (tap // (W * W) - R, tap // W % W - R, tap % W - R)
        dst, src = [Ellipsis], [Ellipsis]
        empty = False
        for e in d:
            lo, hi = max(0, -e), min(G, G - e)           # the outputs whose tap stays inside
            empty |= lo >= hi
            dst.append(slice(lo, hi))
            src.append(slice(lo + e, hi + e))
        if empty:
            continue
        dst, src = tuple(dst), tuple(src)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            cand = v[src] * dtype(wf[tap])
            take = cand > best[dst]                      # a NaN never wins; equal candidates keep the lower tap
        np.copyto(best[dst], cand, where=take)           # (views: the copies land in best and arg)
        np.copyto(arg[dst], np.int32(tap), where=take)
    return best.reshape(s.shape), arg.reshape(s.shape)


def shell_max_at(s, w, G, R, voxels, dtype=np.float32):
    """The same at the flat ``voxels`` only, for shapes whose whole volume is too slow: a gather over the non-zero taps.
    Returns (e3 [V] ``dtype``, arg [V] int32)."""
    dtype = np.dtype(dtype).type
    S, W = G + 2 * R, 2 * R + 1
    pad = np.zeros((S, S, S), dtype=dtype)
    pad[R:R + G, R:R + G, R:R + G] = np.asarray(s).astype(dtype).reshape(G, G, G)        # zeros outside: 0 w is never > best
    pad = pad.reshape(-1)
    wf = np.asarray(w).reshape(-1)
    taps = np.flatnonzero(wf != 0)
    off = (taps // (W * W) * S + taps // W % W) * S + taps % W
    wv = wf[taps].astype(dtype)
    voxels = np.asarray(voxels)
    base = (voxels // (G * G) * S + voxels // G % G) * S + voxels % G
    e3 = np.zeros(len(voxels), dtype=dtype)
    arg = np.full(len(voxels), -1, dtype=np.int32)
    for lo in range(0, len(voxels), 64):
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            cand = pad[base[lo:lo + 64, None] + off[None, :]] * wv[None, :]
            cand = np.where(cand > 0, cand, dtype(0))
        first = cand.argmax(axis=1)                      # the first of the equal maxima: the lowest tap
        e3[lo:lo + 64] = cand[np.arange(len(first)), first]
        arg[lo:lo + 64] = np.where(e3[lo:lo + 64] > 0, taps[first], -1)
    return e3, arg


def tap_voxel(x, tap, G, R):
    """The voxel x + d of tap index ``tap``."""
    W = 2 * R + 1
    return ((x // (G * G) + tap // (W * W) - R) * G + (x // G % G + tap // W % W - R)) * G + (x % G + tap % W - R)


def skeleton_pose_model(prob, taps, parents, G, floor, dtype=np.float32):
    """``prob`` [F, J, N] float32, ``taps`` [J, (2R+1)^3] float32, ``parents`` the tree.  Returns a dict: ``index`` [F, J] int32,
    ``jumped`` [F, J] bool, ``exponent`` [F, J] int32, ``best_root`` [F] ``dtype``, ``solved`` [F] bool, ``log_score`` [F] float64, and
    per frame the lists ``s`` and ``m`` of the scaled scores and the messages [J][N] (``m[f][0]`` is None), ``arg`` of the message
    arguments and ``M`` [F, J] of the row maxima."""
    dtype = np.dtype(dtype).type
    prob, taps = np.asarray(prob), np.asarray(taps)
    assert prob.dtype == np.float32 and prob.ndim == 3 and taps.dtype == np.float32
    F, J, N = prob.shape
    assert N == G ** 3 and len(parents) == J and taps.shape[0] == J
    assert parents[0] == 0 and all(0 <= parents[j] < j for j in range(1, J))
    R = radius_of(taps)
    ch = children(parents)
    fl = dtype(np.float32(floor))
    keep, uniform = dtype(1.0) - fl, fl / dtype(N)
    out = {"index": np.empty((F, J), dtype=np.int32), "jumped": np.zeros((F, J), dtype=bool), "exponent": np.zeros((F, J), dtype=np.int32),
           "best_root": np.full(F, np.nan, dtype=dtype), "solved": np.zeros(F, dtype=bool), "log_score": np.full(F, np.nan),
           "M": np.empty((F, J), dtype=dtype), "s": [], "m": [], "arg": []}
    for f in range(F):
        p = prob[f].astype(dtype)
        s, m, arg, take = [None] * J, [None] * J, [None] * J, [None] * J
        peak, e, best = np.empty(J, dtype=np.int32), np.zeros(J, dtype=np.int32), np.full(J, np.nan, dtype=dtype)
        alive = np.zeros(J, dtype=bool)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for j in range(J - 1, -1, -1):
                A = p[j].copy()
                for c in ch[j]:
                    A = A * m[c]
                Mj, pk = row_max(A[None])
                Mj, peak[j] = Mj[0], pk[0]
                out["M"][f, j] = Mj
                alive[j] = np.isfinite(Mj) and Mj > 0
                if alive[j]:
                    e[j] = np.frexp(Mj)[1] - 1                           # ilogb
                    best[j] = np.ldexp(Mj, -int(e[j]))
                s[j] = np.ldexp(A, -int(e[j])).astype(dtype)             # e = 0: the copy
                if j > 0:
                    e3, arg[j] = shell_max(s[j], taps[j], G, R, dtype)
                    step = keep * e3
                    jump = uniform * best[j]
                    take[j] = jump > step                                # a NaN jump never takes it
                    m[j] = np.where(take[j], jump, step).astype(dtype)
        out["s"].append(s)
        out["m"].append(m)
        out["arg"].append(arg)
        if not alive.all():
            out["index"][f] = row_max(p)[1]
            continue
        x = np.empty(J, dtype=np.int64)
        x[0] = peak[0]
        for j in range(1, J):
            xp = int(x[parents[j]])
            if take[j][xp]:
                x[j], out["jumped"][f, j] = peak[j], True
            elif arg[j][xp] >= 0:
                x[j] = tap_voxel(xp, int(arg[j][xp]), G, R)
            else:                                                        # step = jump = 0: not reached in a solved frame
                x[j] = peak[j]
        out["index"][f], out["exponent"][f], out["best_root"][f], out["solved"][f] = x, e, best[0], True
        out["log_score"][f] = np.log(np.float64(best[0])) + np.log(2.0) * float(e.astype(np.float64).sum())
    return out


def transition(w, G, R, floor):
    """float64 [N, N]: the score max(keep w(y - x), uniform) of the child at y under the parent at x; w = 0 beyond the radius."""
    N, W = G ** 3, 2 * R + 1
    fl = float(np.float32(floor))
    idx = np.arange(N)
    c = np.stack([idx // (G * G), idx // G % G, idx % G], axis=-1)
    d = c[None, :, :] - c[:, None, :]                                    # d[x, y] = y - x
    inside = (np.abs(d) <= R).all(axis=-1)
    tap = ((np.clip(d[..., 0], -R, R) + R) * W + np.clip(d[..., 1], -R, R) + R) * W + np.clip(d[..., 2], -R, R) + R
    Wm = np.where(inside, np.asarray(w, dtype=np.float64).reshape(-1)[tap], 0.0)
    return np.maximum((1.0 - fl) * Wm, fl / N)


def dense_pose(prob, taps, parents, G, floor):
    """float64, for G small: max-product over the tree with dense N x N transition matrices, every score vector normalised by its
    maximum.  ``prob`` [J, N].  Returns (log score of the best pose, the pose [J], the smallest relative margin by which the pose won a
    choice: the root's voxel over the runner-up, and per edge the chosen child voxel over the second-best one)."""
    J, N = prob.shape
    R = radius_of(taps)
    ch = children(parents)
    m, cands = [None] * J, [None] * J
    logz = 0.0
    for j in range(J - 1, -1, -1):
        A = prob[j].astype(np.float64)
        for c in ch[j]:
            A = A * m[c]
        z = A.max()
        A, logz = A / z, logz + np.log(z)
        if j > 0:
            cands[j] = transition(taps[j], G, R, floor) * A[None, :]
            m[j] = cands[j].max(axis=1)

    def margin(v):
        top = np.sort(v)[-2:]
        return (top[1] - top[0]) / top[1]

    x = np.empty(J, dtype=np.int64)
    x[0], gap = int(A.argmax()), margin(A)
    for j in range(1, J):
        row = cands[j][x[parents[j]]]
        x[j], gap = int(row.argmax()), min(gap, margin(row))
    return logz, x, gap


def pose_log_score(prob, taps, parents, G, floor, pose):
    """float64: the log score of one pose under the model (the brute force sums these)."""
    R = radius_of(taps)
    W = 2 * R + 1
    fl = float(np.float32(floor))
    N = G ** 3
    total = 0.0
    for j, x in enumerate(pose):
        total += np.log(float(prob[j, x]))
        if j > 0:
            xp = pose[parents[j]]
            d = (x // (G * G) - xp // (G * G), x // G % G - xp // G % G, x % G - xp % G)
            w = float(taps[j][((d[0] + R) * W + d[1] + R) * W + d[2] + R]) if max(abs(v) for v in d) <= R else 0.0
            with np.errstate(divide="ignore"):
                total += np.log(max((1.0 - fl) * w, fl / N))                 # -inf: floor 0 and no tap
    return total
