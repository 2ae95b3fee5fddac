"""Numpy restatement of the backward max-product pass and the branch walk (include/sceneego_hip.h: se_volume_viterbi_back_f32,
se_volume_viterbi_branch_i32; csrc/volume_viterbi.hip), operation by operation, on top of tests/volume_viterbi_model.py.

``dtype`` = float32 is the definition the kernel must equal bit for bit; float64 is the same recursion for the host checks (against
the brute force over every trajectory).

    link       frame t is linked to t + 1 when t + 1 exists, the forward pass did not restart there and r_{t+1} has a finite positive
               maximum (``link`` = its lowest index, -1 otherwise)
    unlinked   r = p, mm = s, successor pointers -1, complete = 1
    linked     e3 = the three stages (k, j, i) of the forward pass on the scaled r_{t+1} with the taps REVERSED; the offsets compose
               into the successor z(x) as the forward pass composes the predecessor; step = keep * e3, jump = uniform * best_r;
               jump > step: m = jump, successor peak_r with the jump bit; r = p * m, mm = s * m, complete = complete_{t+1}
    death      linked, but r has no finite positive maximum: r = p, successor pointers -1, mm NaN, complete = 0; the frame reports
               no max-marginal (as a frame without a path voxel: -1 / NaN)
    rescaling  as the forward pass: M = max r (from 0, strictly greater, lowest index, a NaN never), e = ilogb(M), r <- ldexp(r, -e)
    outputs    mm_best / mm_peak: the maximum of mm; path_value = mm(x*); alt_value / alt_index: the maximum of mm over the voxels at
               Chebyshev distance > separation from x*; -1 / NaN where nothing is > 0
"""
import numpy as np

from volume_viterbi_model import JUMP, row_max, stage


def reversed_taps(taps):
    return np.ascontiguousarray(np.asarray(taps)[::-1])


def backward_model(prob, fwd, index, taps, G, floor, separation, dtype=np.float32, carry=None, reverse=True):
    """``prob`` [T, rows, N] float32; ``fwd``: what ``volume_viterbi_model`` returned for these frames (``state`` = the scaled scores s,
    ``restarted``), run with the same ``dtype``; ``index`` [T, rows]: the path (``viterbi_path``); ``carry``: what a call over the
    chunk BEHIND this one returned as ``carry`` (None: the chunk's last frame ends the track).  ``reverse`` = False takes the taps as
    they are: the wrong direction, for the test that pins it.  Returns a dict over the T frames: ``mm`` [T, rows, N], ``succ`` [T,
    rows, N] int32, ``r`` [T, rows, N] (scaled), ``mm_best``, ``path_value``, ``alt_value``, ``r_best`` [T, rows] ``dtype``,
    ``mm_peak``, ``alt_index``, ``r_exponent``, ``complete``, ``linked``, ``death`` [T, rows], ``tied`` [T, rows] bool (a gated
    maximum - of r, of mm, of mm outside the window - is attained twice) and ``carry``."""
    dtype = np.dtype(dtype).type
    prob = np.asarray(prob)
    T, rows, N = prob.shape
    taps = np.asarray(taps)
    assert N == G ** 3 and prob.dtype == np.float32 and taps.dtype == np.float32 and separation >= 0
    R = len(taps) // 2
    w = (reversed_taps(taps) if reverse else taps).astype(dtype)
    fl = dtype(np.float32(floor))
    keep, uniform = dtype(1.0) - fl, fl / dtype(N)
    if carry is None:
        r = np.zeros((rows, N), dtype=dtype)
        link = np.full(rows, -1, dtype=np.int32)
        best_next = np.full(rows, np.nan, dtype=dtype)
        complete_next = np.ones(rows, dtype=np.int32)
    else:
        r, link, best_next, complete_next = (np.asarray(carry[key]) for key in ("r", "link", "best", "complete"))
        r = r.astype(dtype)
    nan = dtype(np.nan)
    out = {"mm": np.empty((T, rows, N), dtype=dtype), "succ": np.empty((T, rows, N), dtype=np.int32),
           "r": np.empty((T, rows, N), dtype=dtype)}
    for key in ("mm_best", "path_value", "alt_value", "r_best"):
        out[key] = np.empty((T, rows), dtype=dtype)
    for key in ("mm_peak", "alt_index", "r_exponent", "complete"):
        out[key] = np.empty((T, rows), dtype=np.int32)
    for key in ("linked", "death", "tied"):
        out[key] = np.empty((T, rows), dtype=bool)
    ii, jj, kk = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    rr = np.arange(rows)[:, None, None, None]
    flat_i, flat_j, flat_k = ii.reshape(-1), jj.reshape(-1), kk.reshape(-1)
    for t in range(T - 1, -1, -1):
        p = prob[t].astype(dtype)
        s = np.asarray(fwd["state"][t]).astype(dtype)
        linked = link >= 0
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            if linked.any():
                e1, dk = stage(r.reshape(rows, G, G, G), w, R, 3, dtype)
                e2, dj = stage(e1, w, R, 2, dtype)
                e3, di = stage(e2, w, R, 1, dtype)
                ip = ii[None] + di
                jp = jj[None] + dj[rr, ip, jj[None], kk[None]]
                kp = kk[None] + dk[rr, ip, jp, kk[None]]
                z = ((ip * G + jp) * G + kp).reshape(rows, N).astype(np.int32)
                step = keep * e3.reshape(rows, N)
                jump = (uniform * best_next)[:, None]
                take = jump > step
                m = np.where(take, jump, step).astype(dtype)
                succ = np.where(take, (link | JUMP)[:, None], z).astype(np.int32)
                raw, mm = p * m, s * m
            else:
                raw, mm, succ = p, s, np.full((rows, N), -1, dtype=np.int32)
            M, peak = row_max(raw)
            ok = linked & np.isfinite(M) & (M > 0)
            death = linked & ~ok
            raw = np.where(ok[:, None], raw, p)
            mm = np.where(ok[:, None], mm, np.where(death[:, None], nan, s)).astype(dtype)
            succ = np.where(ok[:, None], succ, -1).astype(np.int32)
            Mp, peak_p = row_max(p)
            M, peak = np.where(ok, M, Mp), np.where(ok, peak, peak_p)
            alive = np.isfinite(M) & (M > 0)
            e = np.where(alive, np.frexp(np.where(alive, M, dtype(1)))[1] - 1, 0).astype(np.int32)
            r = np.ldexp(raw, -e[:, None]).astype(dtype)
            best = np.where(alive, np.ldexp(M, -e), nan).astype(dtype)
            peak = np.where(alive, peak, -1).astype(np.int32)
            complete = np.where(ok, complete_next, np.where(death, 0, 1)).astype(np.int32)
            xs = np.asarray(index[t]).astype(np.int64)
            have = (xs >= 0) & ~death
            x0 = np.clip(xs, 0, N - 1)
            Mm, mm_peak = row_max(mm)
            far = np.maximum(np.maximum(np.abs(flat_i[None] - flat_i[x0][:, None]), np.abs(flat_j[None] - flat_j[x0][:, None])),
                             np.abs(flat_k[None] - flat_k[x0][:, None])) > separation
            outside = np.where(far, mm, dtype(0)).astype(dtype)
            Ma, alt = row_max(outside)
            some, other = have & (Mm > 0), have & (Ma > 0)
            tied = (alive & ((raw == M[:, None]).sum(axis=1) > 1)) | (some & ((mm == Mm[:, None]).sum(axis=1) > 1)) \
                | (other & ((outside == Ma[:, None]).sum(axis=1) > 1))
        out["mm"][t], out["succ"][t], out["r"][t] = mm, succ, r
        out["mm_best"][t], out["mm_peak"][t] = np.where(some, Mm, nan), np.where(some, mm_peak, -1)
        out["path_value"][t] = np.where(have, mm[np.arange(rows), x0], nan)
        out["alt_value"][t], out["alt_index"][t] = np.where(other, Ma, nan), np.where(other, alt, -1)
        out["r_best"][t], out["r_exponent"][t], out["complete"][t] = best, e, complete
        out["linked"][t], out["death"][t], out["tied"][t] = linked, death, tied
        link = np.where(alive & ~np.asarray(fwd["restarted"][t]), peak, -1).astype(np.int32)
        best_next, complete_next = best, complete
    out["carry"] = {"r": r, "link": link, "best": best_next, "complete": complete_next}
    return out


def branch_walk(back, succ, restarted, anchor):
    """``anchor`` [T, rows] int32: a voxel at the anchor frames, -1 elsewhere.  From every anchor back through ``back`` to its
    segment's start and on through ``succ`` to its end: (index [T, rows] int32, -1 where no branch passes; jumped [T, rows] bool)."""
    T, rows, N = back.shape
    index = np.full((T, rows), -1, dtype=np.int32)
    jumped = np.zeros((T, rows), dtype=bool)
    for r in range(rows):
        x = -1
        for t in range(T - 1, -1, -1):
            if anchor[t, r] >= 0:
                x = int(anchor[t, r])
            if x < 0 or x >= N:
                x = -1
            b = int(back[t, r, x]) if x >= 0 and not restarted[t, r] else -1
            index[t, r] = x
            jumped[t, r] = b >= 0 and bool(b & JUMP)
            x = (b & (JUMP - 1)) if b >= 0 else -1
        sp = -1
        for t in range(T):
            x = (sp & (JUMP - 1)) if sp >= 0 else -1
            a = int(anchor[t, r])
            if a >= 0:
                x = a
            if x >= N:
                x = -1
            if a < 0 and x >= 0:
                index[t, r] = x
                jumped[t, r] = bool(sp & JUMP)
            sp = int(succ[t, r, x]) if x >= 0 else -1
    return index, jumped


def margins(path_value, alt_value, alt_index, index):
    """[T, rows] float64: ln path_value - ln alt_value from the float32 values; +inf where the window leaves nothing; NaN where the
    frame has no path voxel or no max-marginal."""
    pv, av = np.asarray(path_value, dtype=np.float64), np.asarray(alt_value, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.log(pv) - np.log(av)
    m = np.where(np.asarray(alt_index) < 0, np.inf, m)
    return np.where((np.asarray(index) < 0) | np.isnan(pv), np.nan, m)


def segments(restarted):
    """[(row, t0, t1)] of every segment of ``restarted`` [T, rows] bool: frames t0 .. t1 - 1."""
    T, rows = restarted.shape
    out = []
    for r in range(rows):
        starts = [t for t in range(T) if restarted[t, r] or t == 0] + [T]
        out += [(r, a, b) for a, b in zip(starts[:-1], starts[1:])]
    return out


def runner_up_anchors(margin, alt_index, restarted):
    """Per segment the anchor frame: the smallest finite margin, the lowest frame among equals.  ``anchor`` [T, rows] int32 (alt_index
    at the anchor frames, -1 elsewhere) and ``runner_up_margin`` [T, rows] float64 (broadcast over the segment; NaN without an
    anchor)."""
    T, rows = margin.shape
    anchor = np.full((T, rows), -1, dtype=np.int32)
    broadcast = np.full((T, rows), np.nan)
    for r, a, b in segments(np.asarray(restarted) != 0):
        m = np.where(np.isfinite(margin[a:b, r]) & (alt_index[a:b, r] >= 0), margin[a:b, r], np.inf)
        if np.isfinite(m).any():
            t = a + int(np.argmin(m))
            anchor[t, r] = alt_index[t, r]
            broadcast[a:b, r] = m[t - a]
    return anchor, broadcast


def brute_force_max_marginals(prob, taps, G, floor):
    """float64, one row, N^T small: (mm [T, N], arg [T, N, T]) by enumeration of every trajectory of ``prob`` [T, N]; the transition
    score from x to z is max(keep W(x - z), uniform), W = ((w_k) w_j) w_i as the stages take it.  mm is normalised by its maximum."""
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

    tr = np.maximum(keep * ((axis(ck) * axis(cj)) * axis(ci)), uniform)           # tr[x, y]: from y to x
    p = prob.astype(np.float64)
    score = p[0].copy()                                  # [N^1], [N^2], ... the last axis is the latest frame
    for t in range(1, T):
        score = score[..., :, None] * tr.T[(None,) * (t - 1)] * p[t][(None,) * t]
    mm = np.empty((T, N))
    arg = np.empty((T, N, T), dtype=np.int64)
    for t in range(T):
        moved = np.moveaxis(score, t, 0).reshape(N, -1)
        mm[t] = moved.max(axis=1)
        best = moved.argmax(axis=1)
        shape = tuple(N for _ in range(T - 1))
        others = np.stack(np.unravel_index(best, shape), axis=1) if T > 1 else np.zeros((N, 0), dtype=np.int64)
        arg[t] = np.insert(others, t, idx, axis=1)
    return mm / mm.max(), arg, score
