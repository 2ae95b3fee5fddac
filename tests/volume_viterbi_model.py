"""Numpy restatement of the max-product pass (include/sceneego_hip.h: se_volume_viterbi_f32, se_volume_viterbi_path_i32,
se_volume_viterbi_refine_f32; csrc/volume_viterbi.hip), operation by operation.

``dtype`` = float32 is the definition: every product is one float32 rounding, numpy keeps float32 gradual underflow, and the kernel
must equal it bit for bit.  ``dtype`` = float64 is the same recursion for the host checks (against a dense Viterbi, and that the
float32 path is the float64 path on the test inputs).

    stage      best = 0, offset 0; for d = -R..R ascending, skipping taps that leave the grid: cand = v[n + d] * w[d]; cand > best takes
    e3         stage along k, then j, then i, each on the values of the stage before; the offsets compose into y(x):
               i' = i + di(x), j' = j + dj(i', j, k), k' = k + dk(i', j', k)
    step/jump  step = keep * e3, jump = uniform * best_prev; jump > step: m = jump, predecessor peak_prev with the jump bit
    update     a = p * m; M = max a (from 0, strictly greater wins: lowest index, NaN never), e = ilogb(M), s = ldexp(a, -e)
    restart    no prior, or M not a finite number > 0: a = p, back = -1; p without a finite positive maximum: s = p, peak -1, best NaN, e 0
"""
import numpy as np

JUMP = 1 << 30


def stage(v, w, R, axis, dtype):
    """``v`` [rows, G, G, G]: (best, offset) of the stage along ``axis`` (1 = i, 2 = j, 3 = k)."""
    G = v.shape[axis]
    best = np.zeros(v.shape, dtype=dtype)
    off = np.zeros(v.shape, dtype=np.int8)
    for d in range(-R, R + 1):
        dst = [slice(None)] * 4
        src = [slice(None)] * 4
        dst[axis] = slice(max(0, -d), G - max(0, d))
        src[axis] = slice(max(0, d), G + min(0, d))
        dst, src = tuple(dst), tuple(src)
        cand = v[src] * dtype(w[d + R])
        with np.errstate(invalid="ignore"):
            take = cand > best[dst]
        np.copyto(best[dst], cand, where=take)          # (views: the copies land in best and off)
        np.copyto(off[dst], np.int8(d), where=take)
    return best, off


def row_max(a):
    """(M, peak) [rows] of ``a`` [rows, N]: the greatest value > 0 and its lowest index; (0, -1) where there is none."""
    with np.errstate(invalid="ignore"):
        pos = np.where(a > 0, a, a.dtype.type(0))
    M = pos.max(axis=1)
    peak = pos.argmax(axis=1).astype(np.int32)
    return M, np.where(M > 0, peak, -1).astype(np.int32)


def volume_viterbi_model(prob, taps, G, floor, dtype=np.float32, state=None, peak_state=None, best_state=None, have_prior=None):
    """``prob`` [T, rows, N] float32, ``taps`` [2R+1] float32, ``state`` / ``peak_state`` / ``best_state`` / ``have_prior``: what a
    previous call returned as ``state[-1]``, ``peak[-1]``, ``best[-1]`` and an all-true flag (None: the track starts here).  Returns a
    dict: ``state`` [T, rows, N] (the scaled scores after every frame, ``dtype``), ``back`` [T, rows, N] int32, ``peak``, ``exponent``
    [T, rows] int32, ``best`` [T, rows] ``dtype``, ``restarted`` [T, rows] bool, ``tied`` [T, rows] bool (the frame's maximum is
    attained more than once: the input condition the GPU test asserts against) and ``jump_bits`` [T, rows] (back-pointers with the
    jump bit)."""
    dtype = np.dtype(dtype).type
    prob = np.asarray(prob)
    assert prob.dtype == np.float32 and prob.ndim == 3
    T, rows, N = prob.shape
    taps = np.asarray(taps)
    assert N == G ** 3 and taps.dtype == np.float32 and len(taps) % 2 == 1
    R = len(taps) // 2
    w = taps.astype(dtype)
    fl = dtype(np.float32(floor))
    keep, uniform = dtype(1.0) - fl, fl / dtype(N)
    prior = np.zeros(rows, dtype=bool) if have_prior is None else np.asarray(have_prior) != 0
    s = np.zeros((rows, N), dtype=dtype) if state is None else np.asarray(state).astype(dtype)
    peak_prev = np.full(rows, -1, dtype=np.int32) if peak_state is None else np.asarray(peak_state).astype(np.int32)
    best_prev = np.full(rows, np.nan, dtype=dtype) if best_state is None else np.asarray(best_state).astype(dtype)
    out = {"state": np.empty((T, rows, N), dtype=dtype), "back": np.empty((T, rows, N), dtype=np.int32),
           "peak": np.empty((T, rows), dtype=np.int32), "best": np.empty((T, rows), dtype=dtype),
           "exponent": np.empty((T, rows), dtype=np.int32), "restarted": np.empty((T, rows), dtype=bool),
           "tied": np.empty((T, rows), dtype=bool), "jump_bits": np.empty((T, rows), dtype=np.int64)}
    ii, jj, kk = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    rr = np.arange(rows)[:, None, None, None]
    for t in range(T):
        p = prob[t].astype(dtype)
        prior = prior & (peak_prev >= 0)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            if prior.any():
                e1, dk = stage(s.reshape(rows, G, G, G), w, R, 3, dtype)
                e2, dj = stage(e1, w, R, 2, dtype)
                e3, di = stage(e2, w, R, 1, dtype)
                ip = ii[None] + di
                jp = jj[None] + dj[rr, ip, jj[None], kk[None]]
                kp = kk[None] + dk[rr, ip, jp, kk[None]]
                y = ((ip * G + jp) * G + kp).reshape(rows, N).astype(np.int32)
                step = keep * e3.reshape(rows, N)
                jump = (uniform * best_prev)[:, None]
                take = jump > step
                m = np.where(take, jump, step).astype(dtype)
                back = np.where(take, (peak_prev | JUMP)[:, None], y).astype(np.int32)
                a = p * m
            else:                                        # every row restarts: nothing of the recursion is used
                a, back = p, np.full((rows, N), -1, dtype=np.int32)
            M, peak = row_max(a)
            ok = prior & np.isfinite(M) & (M > 0)
            a = np.where(ok[:, None], a, p)
            back = np.where(ok[:, None], back, -1).astype(np.int32)
            Mp, peak_p = row_max(p)
            M, peak = np.where(ok, M, Mp), np.where(ok, peak, peak_p)
            alive = np.isfinite(M) & (M > 0)
            e = np.where(alive, np.frexp(np.where(alive, M, dtype(1)))[1] - 1, 0).astype(np.int32)       # ilogb
            sc = np.ldexp(a, -e[:, None]).astype(dtype)                                                 # e = 0: the copy
            best = np.where(alive, np.ldexp(M, -e), dtype(np.nan)).astype(dtype)
            peak = np.where(alive, peak, -1).astype(np.int32)
            tied = (a == M[:, None]).sum(axis=1) > 1
        out["state"][t], out["back"][t], out["peak"][t], out["best"][t] = sc, back, peak, best
        out["exponent"][t], out["restarted"][t], out["tied"][t] = e, ~ok, tied & alive
        out["jump_bits"][t] = ((back >= 0) & ((back & JUMP) != 0)).sum(axis=1)
        s, peak_prev, best_prev, prior = sc, peak, best, np.ones(rows, dtype=bool)
    return out


def viterbi_path(back, peak, restarted):
    """The back-walk: ``back`` [T, rows, N] int32, ``peak`` [T, rows], ``restarted`` [T, rows] -> (index [T, rows] int32, jumped [T, rows]
    bool).  x of the last frame is its peak; x_{t-1} = back_t[x_t] & (2^30 - 1); at a segment start x_{t-1} = peak_{t-1}."""
    T, rows, _ = back.shape
    index = np.empty((T, rows), dtype=np.int32)
    jumped = np.zeros((T, rows), dtype=bool)
    for r in range(rows):
        x = -1
        for t in range(T - 1, -1, -1):
            if x < 0:
                x = int(peak[t, r])
            b = int(back[t, r, x]) if x >= 0 and not restarted[t, r] else -1
            index[t, r] = x
            jumped[t, r] = b >= 0 and bool(b & JUMP)
            x = (b & (JUMP - 1)) if b >= 0 else -1
    return index, jumped


def refine_model(prob, coord, index, G, refine):
    """joints [T, rows, 3] float32: the centroid of ``prob`` [T, rows, N] float32 over the window of ``refine`` voxels around ``index``,
    clipped to the grid: float64 sums in ascending flat index, one rounding each, NaN cells passed over, the quotient rounded once to
    float32; the voxel centre where the sum is not a finite number > 0 or ``refine`` = 0; NaN for index -1."""
    T, rows = index.shape
    c = np.asarray(coord, dtype=np.float32).reshape(G ** 3, 3)
    out = np.full((T, rows, 3), np.nan, dtype=np.float32)
    for t in range(T):
        for r in range(rows):
            x = int(index[t, r])
            if x < 0:
                continue
            out[t, r] = c[x]
            if refine == 0:
                continue
            ci, cj, ck = x // (G * G), (x // G) % G, x % G
            m, sx = 0.0, [0.0, 0.0, 0.0]
            for i in range(max(ci - refine, 0), min(ci + refine, G - 1) + 1):
                for j in range(max(cj - refine, 0), min(cj + refine, G - 1) + 1):
                    for k in range(max(ck - refine, 0), min(ck + refine, G - 1) + 1):
                        n = (i * G + j) * G + k
                        pv = float(prob[t, r, n])
                        if pv != pv:
                            continue
                        m += pv
                        for a in range(3):
                            sx[a] += pv * float(c[n, a])
            if m > 0.0 and np.isfinite(m):
                out[t, r] = [np.float32(sx[a] / m) for a in range(3)]
    return out


def dense_viterbi(prob, taps, G, floor):
    """float64, for G small: the Viterbi recursion over all N^2 transitions with score max(keep W(d), uniform), W the product of the
    three taps (0 beyond the radius), normalised per frame by its maximum.  Returns (log score of the best path, the path [T], the
    smallest relative margin by which the best path won a choice: its end voxel over the runner-up, and at every step back along it
    the chosen predecessor over the second-best one)."""
    T, N = prob.shape
    R = len(taps) // 2
    w = np.asarray(taps, dtype=np.float64)
    fl = float(np.float32(floor))
    keep, uniform = 1.0 - fl, fl / N
    idx = np.arange(N)
    ci, cj, ck = idx // (G * G), (idx // G) % G, idx % G

    def axis(c):
        d = c[None, :] - c[:, None]                      # d[x, y] = y - x: the predecessor y = x + d
        return np.where(np.abs(d) <= R, w[np.clip(d + R, 0, 2 * R)], 0.0)

    # the product in the order the stages take it: ((s w_k) w_j) w_i
    tr = np.maximum(keep * ((axis(ck) * axis(cj)) * axis(ci)), uniform)           # tr[x, y]: from y to x
    s = prob[0].astype(np.float64)
    logz = 0.0
    cands = []
    for t in range(1, T):
        cand = tr * s[None, :]
        cands.append(cand)
        s = prob[t].astype(np.float64) * cand.max(axis=1)
        z = s.max()
        s, logz = s / z, logz + np.log(z)

    def margin(v):
        top = np.sort(v)[-2:]
        return (top[1] - top[0]) / top[1]

    x = int(s.argmax())
    path, gap = [x], margin(s)
    for cand in reversed(cands):
        gap = min(gap, margin(cand[x]))
        x = int(cand[x].argmax())
        path.append(x)
    return logz + np.log(s.max()), np.array(path[::-1]), gap
