"""Numpy model of the trajectory sampler (include/sceneego_hip.h: se_volume_sample_f32; csrc/volume_sample.hip, csrc/categorical_draw.h):
forward-filter backward-sampling on the filter's own model, restated so that it has one right answer.

Everything is float64 with one rounding per operation and every sum is SEQUENTIAL in ascending index: ``np.cumsum`` /
``np.add.accumulate`` (never ``np.sum``, whose pairwise order is numpy's own).  The random numbers are Philox4x32-10 in pure integer
arithmetic.  So the kernel's ``index``, ``kind`` and ``next`` are compared with this model bit for bit.

    transition x (frame t) -> y (frame t + 1):  (1 - floor) W(x -> y) + floor / N,  W as blur3 has it: q(y) = sum_d w[d] b(y + d), so
    the window of y is x = y + d with weight w[di] w[dj] w[dk], no tap reversal, taps that leave the grid skipped
    x_T ~ b_T;   x_t ~ b_t(x) [(1 - floor) W(x -> x_{t+1}) + floor / N] where t is linked to t + 1;   x_t ~ b_t where it is not
    linked: t is not the last frame of the track, restarted[t + 1] is clear and the draw of t + 1 was valid

The model is vectorised over the samples of a (frame, row): the running sums of a frame are shared by its samples, and samples that
stand on the same voxel y share one window.  ``draw`` is the scalar definition, kept for the tests of the vectorised searches.
"""
import numpy as np

STEP, JUMP, FRESH = 0, 1, 2
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------ random numbers
def philox4x32_10(counter, key):
    """``counter`` [..., 4] and ``key`` [..., 2] (broadcast against each other), any unsigned integers below 2^32 -> [..., 4] uint32:
    ten rounds of Philox4x32 (Salmon et al., SC'11), the key bumped by the Weyl constants between rounds."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., n].copy() for n in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2               # 32 x 32 -> 64 bits: exact in uint64
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n1 = p1 & np.uint64(MASK)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        n3 = p0 & np.uint64(MASK)
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK), (k1 + np.uint64(W1)) & np.uint64(MASK)
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def uniform53(hi, lo):
    """(double)((hi << 32 | lo) >> 11) 2^-53: exact."""
    x = (np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def uniforms(seed, samples, frame, row):
    """u0, u1, u2, u3 [len(samples)] of the GLOBAL sample indices ``samples`` at the global frame index ``frame`` and ``row``: key
    (seed_lo, seed_hi), counter (sample, frame, row, block); block 0 gives u0, u1 and block 1 u2, u3."""
    samples = np.asarray(samples, dtype=np.uint64)
    key = np.array([int(seed) & MASK, (int(seed) >> 32) & MASK], dtype=np.uint64)
    out = []
    for block in (0, 1):
        ctr = np.stack([samples, np.full_like(samples, frame), np.full_like(samples, row), np.full_like(samples, block)], axis=-1)
        x = philox4x32_10(ctr, key)
        out += [uniform53(x[:, 0], x[:, 1]), uniform53(x[:, 2], x[:, 3])]
    return out


# ------------------------------------------------------------------------------------------------------------------ the draw
def mass_ok(total):
    return np.isfinite(total) & (total > 0)


def draw(v, u):
    """THE CATEGORICAL DRAW, as the definition words it: non-negative ``v`` [n], ``u`` in [0, 1).  -1: no draw."""
    v = np.asarray(v, dtype=np.float64)
    c = np.cumsum(v)
    total = c[-1]
    if not mass_ok(total):
        return -1
    thr = u * total
    for m in range(len(v)):
        if c[m] > thr:
            return m
    return int(np.flatnonzero(v > 0)[-1])


def last_positive(v):
    """The last m with v[..., m] > 0 along the last axis, -1 where there is none."""
    pos = v > 0
    n = v.shape[-1]
    return np.where(pos.any(axis=-1), n - 1 - np.argmax(pos[..., ::-1], axis=-1), -1)


def search(c, last, u):
    """The draw of every row of the running sums ``c`` [S, n] (``last`` [S]: last_positive of the values) with ``u`` [S]."""
    total = c[:, -1]
    with np.errstate(invalid="ignore", over="ignore"):
        hit = c > (u * total)[:, None]
    m = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last)
    return np.where(mass_ok(total), m, -1)


# ------------------------------------------------------------------------------------------------------------------ one frame
class Frame:
    """The three levels of sums of one belief ``b`` [G^3] float32: Rs[i][j] = sum_k b, P[i] = sum_j Rs[i][j], total = sum_i P[i]."""

    def __init__(self, b, G):
        b = np.asarray(b)
        assert b.dtype == np.float32 and b.shape == (G ** 3,)
        self.G = G
        self.b = b.astype(np.float64).reshape(G, G, G)
        with np.errstate(invalid="ignore", over="ignore"):
            self.ck = np.cumsum(self.b, axis=2)
            self.Rs = self.ck[:, :, -1]
            self.cj = np.cumsum(self.Rs, axis=1)
            self.P = self.cj[:, -1]
            self.ci = np.cumsum(self.P)
        self.total = self.ci[-1]
        self.last_k, self.last_j, self.last_i = last_positive(self.b), last_positive(self.Rs), last_positive(self.P)

    def global_draw(self, u1, u2, u3):
        """The voxel of every sample from (u1, u2, u3) [S]; -1: invalid."""
        S, G = len(u1), self.G
        out = np.full(S, -1, dtype=np.int64)
        if not mass_ok(self.total):
            return out
        i = search(np.broadcast_to(self.ci, (S, G)), np.full(S, self.last_i), u1)
        ok = i >= 0
        j = np.full(S, -1, dtype=np.int64)
        j[ok] = search(self.cj[i[ok]], self.last_j[i[ok]], u2[ok])
        ok &= j >= 0
        k = np.full(S, -1, dtype=np.int64)
        k[ok] = search(self.ck[i[ok], j[ok]], self.last_k[i[ok], j[ok]], u3[ok])
        ok &= k >= 0
        out[ok] = (i[ok] * G + j[ok]) * G + k[ok]
        return out

    def window(self, y, w, R):
        """The window sums of voxel ``y`` with the float64 taps ``w`` [2R+1]: x = y + d, clipped to the grid."""
        G = self.G
        yi, yj, yk = y // (G * G), (y // G) % G, y % G
        lo = [max(-R, -c) for c in (yi, yj, yk)]
        n = [min(R, G - 1 - c) - l + 1 for c, l in zip((yi, yj, yk), lo)]
        sub = self.b[yi + lo[0]:yi + lo[0] + n[0], yj + lo[1]:yj + lo[1] + n[1], yk + lo[2]:yk + lo[2] + n[2]]
        wi, wj, wk = (w[l + R:l + R + m] for l, m in zip(lo, n))
        with np.errstate(invalid="ignore", over="ignore"):
            tk = sub * wk[None, None, :]                  # b(y + d) w[dk]
            ck = np.cumsum(tk, axis=2)
            r = ck[:, :, -1]
            tj = r * wj[None, :]                          # r[di][dj] w[dj]
            cj = np.cumsum(tj, axis=1)
            q = cj[:, -1]
            ti = q * wi                                   # q[di] w[di]
            ci = np.cumsum(ti)
        return {"base": (yi + lo[0], yj + lo[1], yk + lo[2]), "n": n, "tk": tk, "ck": ck, "tj": tj, "cj": cj, "ti": ti, "ci": ci,
                "Wsum": ci[-1]}


def masses(frame, win, keep, uniform):
    with np.errstate(invalid="ignore", over="ignore"):
        step = keep * win["Wsum"]
        jump = uniform * frame.total
        return step, jump, step + jump


def window_draw(win, G, u1, u2, u3):
    """The step's voxel of every sample: di, then dj, then dk."""
    S = len(u1)
    out = np.full(S, -1, dtype=np.int64)
    a = search(np.broadcast_to(win["ci"], (S, len(win["ci"]))), np.full(S, last_positive(win["ti"])), u1)
    ok = a >= 0
    c = np.full(S, -1, dtype=np.int64)
    c[ok] = search(win["cj"][a[ok]], last_positive(win["tj"])[a[ok]], u2[ok])
    ok &= c >= 0
    m = np.full(S, -1, dtype=np.int64)
    m[ok] = search(win["ck"][a[ok], c[ok]], last_positive(win["tk"])[a[ok], c[ok]], u3[ok])
    ok &= m >= 0
    i0, j0, k0 = win["base"]
    out[ok] = ((i0 + a[ok]) * G + (j0 + c[ok])) * G + k0 + m[ok]
    return out


def constants(floor, N):
    """keep and uniform: float32 as the filter's kernels form them, then float64."""
    f = np.float32(floor)
    return float(np.float32(1.0) - f), float(f / np.float32(N))


# ------------------------------------------------------------------------------------------------------------------ the chain
def volume_sampler_model(belief, restarted, taps, G, floor, samples, seed=0, first_sample=0, first_frame=0, next_voxel=None,
                         have_link=None):
    """``belief`` [T, rows, N] float32, ``restarted`` [T, rows], ``taps`` [2R+1] float32; ``next_voxel`` None or [samples, rows] (the
    voxel of the frame behind the last one), ``have_link`` None or bool [rows].  Returns a dict: ``index`` and ``kind`` [samples, T,
    rows] int32 and ``next`` [samples, rows] int32 (the voxel of frame 0: what the call over the frames before these takes)."""
    belief = np.asarray(belief)
    assert belief.dtype == np.float32 and belief.ndim == 3
    T, rows, N = belief.shape
    taps = np.asarray(taps)
    assert N == G ** 3 and taps.dtype == np.float32 and len(taps) % 2 == 1
    R = (len(taps) - 1) // 2
    w = taps.astype(np.float64)
    restarted = np.asarray(restarted) != 0
    keep, uniform = constants(floor, N)
    S = int(samples)
    index = np.full((S, T, rows), -1, dtype=np.int32)
    kind = np.full((S, T, rows), -1, dtype=np.int32)
    nxt = np.full((S, rows), -1, dtype=np.int32)
    gs = np.arange(first_sample, first_sample + S)
    for row in range(rows):
        y = np.full(S, -1, dtype=np.int64)
        if have_link is not None and have_link[row]:
            y = np.asarray(next_voxel)[:, row].astype(np.int64)
            y = np.where((y < 0) | (y >= N), -1, y)
        for t in range(T - 1, -1, -1):
            if t < T - 1 and restarted[t + 1, row]:
                y[:] = -1
            fr = Frame(belief[t, row], G)
            u0, u1, u2, u3 = uniforms(seed, gs, first_frame + t, row)
            mode = np.full(S, FRESH, dtype=np.int32)
            x = np.full(S, -1, dtype=np.int64)
            for yv in np.unique(y[y >= 0]):
                grp = np.flatnonzero(y == yv)
                win = fr.window(int(yv), w, R)
                step, jump, mass = masses(fr, win, keep, uniform)
                if not mass_ok(mass):
                    continue                                   # drawn as an unlinked frame
                jumps = u0[grp] * mass >= step
                mode[grp] = np.where(jumps, JUMP, STEP)
                st = grp[~jumps]
                x[st] = window_draw(win, G, u1[st], u2[st], u3[st])
            glob = np.flatnonzero(mode != STEP)
            x[glob] = fr.global_draw(u1[glob], u2[glob], u3[glob])
            index[:, t, row], kind[:, t, row] = x, mode
            y = x.copy()
        nxt[:, row] = y
    return {"index": index, "kind": kind, "next": nxt}


def sample_in_chunks(belief, restarted, taps, G, floor, samples, cuts, seed=0, first_sample=0):
    """The chain over calls of ``cuts`` frames each (in frame order; issued last chunk first, ``next`` and ``have_link`` carried)."""
    T = belief.shape[0]
    assert sum(cuts) == T
    starts = np.concatenate([[0], np.cumsum(cuts)]).tolist()
    restarted = np.asarray(restarted) != 0
    parts, nxt, link = [], None, None
    for i in range(len(cuts) - 1, -1, -1):
        t0, t1 = starts[i], starts[i + 1]
        if t1 < T:
            link = ~restarted[t1]
        got = volume_sampler_model(belief[t0:t1], restarted[t0:t1], taps, G, floor, samples, seed=seed, first_sample=first_sample,
                                   first_frame=t0, next_voxel=nxt, have_link=link)
        nxt = got["next"]
        parts.insert(0, got)
    return {"index": np.concatenate([p["index"] for p in parts], axis=1), "kind": np.concatenate([p["kind"] for p in parts], axis=1),
            "next": nxt}


# ------------------------------------------------------------------------------------------------------------------ the law
def global_law(fr):
    """The probability of every voxel under the global draw, from the model's own sums: (P/total)(Rs/P)(b/Rs)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        pi = fr.P / fr.total
        pj = np.where(fr.P[:, None] > 0, fr.Rs / fr.P[:, None], 0.0)
        pk = np.where(fr.Rs[:, :, None] > 0, fr.b / fr.Rs[:, :, None], 0.0)
    return (pi[:, None, None] * pj[:, :, None] * pk).reshape(-1)


def conditional_law(b_t, y, taps, G, floor):
    """The full N-vector of the probabilities of x_t given x_{t+1} = ``y`` that the model's own masses imply: the step's share times
    the three window levels plus the jump's share times the global law.  ``b_t`` [N] float32."""
    taps = np.asarray(taps)
    R = (len(taps) - 1) // 2
    N = G ** 3
    fr = Frame(np.asarray(b_t, dtype=np.float32), G)
    win = fr.window(int(y), taps.astype(np.float64), R)
    keep, uniform = constants(floor, N)
    step, jump, mass = masses(fr, win, keep, uniform)
    law = (jump / mass) * global_law(fr).reshape(G, G, G)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = win["cj"][:, -1]
        r = win["ck"][:, :, -1]
        pa = win["ti"] / win["Wsum"] if win["Wsum"] > 0 else np.zeros_like(win["ti"])
        pc = np.where(q[:, None] > 0, win["tj"] / q[:, None], 0.0)
        pm = np.where(r[:, :, None] > 0, win["tk"] / r[:, :, None], 0.0)
    i0, j0, k0 = win["base"]
    n = win["n"]
    law[i0:i0 + n[0], j0:j0 + n[1], k0:k0 + n[2]] += (step / mass) * pa[:, None, None] * pc[:, :, None] * pm
    return law.reshape(-1)
