"""numpy float64 model of csrc/render_volume.hip: a literal restatement of the arithmetic include/sceneego_hip.h states for
se_render_volume_view_f64 / se_render_volume_overlay_f64, operation by operation (numpy rounds every product, sum and quotient
separately, as the unfused kernel does).

``march``      -> per pixel: hit flag, the 15 maxima m_j (already multiplied by the scale), and the ``ambiguous`` mask: pixels where a
                  decision of the slab test, of the cell walk or of the range lies within 1e-9 (relative) / 1e-6 (against the scene)
                  of flipping.  The GPU tests compare every other pixel exactly and cap the ambiguous share, so the mask cannot hide
                  a failure.
``composite``  -> the picture and the pixels where the clamp at 1 or the final rounding could flip.
``view`` / ``overlay`` -> the two entry points on a batch.
``brute_maxima`` -> an independent formulation used by tests/test_volume_render_host.py: every cell's own slab interval.
"""
import numpy as np

from sceneego_amd import _lib

JOINTS = 15
PALETTE = np.array(_lib.render_volume_palette(), dtype=np.float64)         # [15, 3], the table of include/sceneego_hip.h
REL, ABS_S, ABS_C = 1e-9, 1e-6, 1e-6
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
ALL = (1 << JOINTS) - 1


def grid(G, S):
    """pos [3], h of op.build_coord_volume(G, S)."""
    return np.array([-(S / 2.0), -(S / 2.0), 0.0]), S / float(G - 1)


def bnd(pos_a, h, k):
    return pos_a + (np.asarray(k, dtype=np.float64) - 0.5) * h


def view_rays(rays, view):
    """pinhole table [h,w,3], view [12] -> origin [3], directions [h,w,3] in the camera frame."""
    v = np.asarray(view, dtype=np.float64)
    o = np.array([-((v[i] * v[9] + v[3 + i] * v[10]) + v[6 + i] * v[11]) for i in range(3)])
    d = np.stack([(v[i] * rays[..., 0] + v[3 + i] * rays[..., 1]) + v[6 + i] * rays[..., 2] for i in range(3)], axis=-1)
    return o, d


def _near(a, b):
    """|a - b| within the relative margin (two infinities of one sign are not 'near': nothing can flip there)."""
    with np.errstate(all="ignore"):
        return np.abs(a - b) <= REL * np.maximum(1.0, np.maximum(np.abs(a), np.abs(b)))


def _range(o, d, G, S, near, limit):
    """The slab test: miss, s0, s1, inv [3][...], ambiguous."""
    pos, h = grid(G, S)
    shape = d.shape[:-1]
    fin = np.isfinite(d).all(axis=-1) & ~np.isnan(limit)
    miss = ~fin
    amb = np.zeros(shape, dtype=bool)
    s0 = np.full(shape, float(near))
    s1 = np.where(np.isnan(limit), np.inf, limit).astype(np.float64)
    inv = []
    with np.errstate(all="ignore"):
        for a in range(3):
            lo, hi = float(bnd(pos[a], h, 0)), float(bnd(pos[a], h, G))
            da = np.where(fin, d[..., a], 1.0)
            zero = da == 0.0
            inside = (o[a] >= lo) and (o[a] < hi)
            miss |= zero & (not inside)
            amb |= zero & bool(_near(o[a], lo) | _near(o[a], hi))
            # a direction within the margin of zero: whether the axis is walked at all could flip
            amb |= ~zero & (np.abs(da) <= REL)
            ia = 1.0 / np.where(zero, 1.0, da)
            ta, tb = (lo - o[a]) * ia, (hi - o[a]) * ia
            tn, tf = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            s0 = np.where(~zero & (tn > s0), tn, s0)
            s1 = np.where(~zero & (tf < s1), tf, s1)
            inv.append(np.where(zero, 0.0, ia))
        miss |= ~(s0 < s1)
        amb |= fin & (_near(s0, s1) | ((np.abs(s0 - s1) < ABS_S) & (s1 == limit)))
    return miss, s0, s1, inv, amb


def march(o, d, vol, scale, G, S, near, limit, live):
    """o [3], d [...,3], vol [15,G,G,G] float32, scale [15], limit [...] (+inf: none; NaN: nothing shows), live: bit mask of the
    joints that are not off -> hit bool [...], m float64 [..., 15], ambiguous bool [...]."""
    pos, h = grid(G, S)
    shape = d.shape[:-1]
    miss, s0, s1, inv, amb = _range(o, d, G, S, near, limit)
    m = np.zeros(shape + (JOINTS,))
    if live == 0:
        return np.zeros(shape, dtype=bool), m, np.zeros(shape, dtype=bool)
    cells = vol.reshape(JOINTS, G * G * G).astype(np.float64)
    with np.errstate(all="ignore"):
        dd = [np.where(miss, 0.0, d[..., a]) for a in range(3)]
        idx, step, nxt = [], [], []
        for a in range(3):
            u = ((o[a] + s0 * dd[a]) - pos[a]) / h + 0.5
            i = np.where(u >= 0.0, np.where(u < float(G), np.floor(u), float(G - 1)), 0.0)
            i = np.where(np.isnan(i), 0.0, i).astype(np.int64)
            # the start index could flip where u is within the margin of an integer that the clamp does not absorb
            lo_i = np.clip(np.floor(u - REL * np.maximum(1.0, np.abs(u))), 0, G - 1)
            hi_i = np.clip(np.floor(u + REL * np.maximum(1.0, np.abs(u))), 0, G - 1)
            amb |= ~miss & (lo_i != hi_i)
            st = np.where(dd[a] > 0.0, 1, np.where(dd[a] < 0.0, -1, 0)).astype(np.int64)
            idx.append(i)
            step.append(st)
            nxt.append(np.where(st != 0, (bnd(pos[a], h, i + (st > 0)) - o[a]) * inv[a], np.inf))
        active = ~miss
        for _ in range(3 * G + 1):
            if not active.any():
                break
            flat = (idx[0] * G + idx[1]) * G + idx[2]
            for j in range(JOINTS):
                if not (live >> j) & 1:
                    continue
                v = cells[j][flat] * scale[j]
                take = active & (v > m[..., j])
                m[..., j] = np.where(take, v, m[..., j])
            a = np.zeros(shape, dtype=np.int64)
            t = nxt[0]
            pick = nxt[1] < t
            a, t = np.where(pick, 1, a), np.where(pick, nxt[1], t)
            pick = nxt[2] < t
            a, t = np.where(pick, 2, a), np.where(pick, nxt[2], t)
            # a choice between two faces within the margin, and the entry parameter against the end of the range
            srt = np.sort(np.stack(nxt, axis=-1), axis=-1)
            amb |= active & np.isfinite(srt[..., 1]) & _near(srt[..., 0], srt[..., 1])
            # (a step that leaves the grid ends the walk whichever way its comparison falls: the exit face of the box is such a step)
            stays = np.zeros(shape, dtype=bool)
            for k in range(3):
                stays |= (a == k) & (idx[k] + step[k] >= 0) & (idx[k] + step[k] < G)
            amb |= active & stays & np.isfinite(t) & np.isfinite(s1) & (_near(t, s1) | (np.abs(t - s1) < ABS_S) & (s1 == limit))
            active = active & (t < s1)
            for k in range(3):
                mv = active & (a == k)
                idx[k] = np.where(mv, idx[k] + step[k], idx[k])
            out = (idx[0] < 0) | (idx[0] >= G) | (idx[1] < 0) | (idx[1] >= G) | (idx[2] < 0) | (idx[2] >= G)
            active = active & ~out
            for k in range(3):
                idx[k] = np.clip(idx[k], 0, G - 1)
                mv = active & (a == k)
                nxt[k] = np.where(mv, (bnd(pos[k], h, idx[k] + (step[k] > 0)) - o[k]) * inv[k], nxt[k])
        assert not active.any(), "the walk did not end within 3 G steps"
    return ~miss, m, amb & np.isfinite(d).all(axis=-1)


def composite(base_rgb, hit, m, live, gain, opacity):
    """base_rgb uint8 [...,3], m [...,15] -> out uint8 [...,3], ambiguous [...]."""
    c = base_rgb.astype(np.float64)
    amb = np.zeros(hit.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(JOINTS):
            if not (live >> j) & 1:
                continue
            g = gain * m[..., j]
            amb |= hit & (np.abs(g - 1.0) <= REL)
            a = np.where(g < 1.0, g, 1.0) * opacity
            a = np.where(hit, a, 0.0)
            for k in range(3):
                c[..., k] = c[..., k] + a * (PALETTE[j][k] - c[..., k])
        v = c + 0.5
        amb |= hit & (np.abs(v - np.rint(v)) <= ABS_C).any(axis=-1)
        out = np.clip(np.floor(v), 0, 255).astype(np.uint8)
    return out, amb


def live_mask(scale, joint_mask):
    live = 0
    for j in range(JOINTS):
        if (joint_mask >> j) & 1 and np.isfinite(scale[j]) and scale[j] > 0.0:
            live |= 1 << j
    return live


def view(rays, view12, zbuf, base, volumes, scale, S, near, joint_mask=ALL, gain=1.0, opacity=0.8):
    """rays [h,w,3] pinhole table, zbuf None or [B,h,w] uint64, base uint8 [B,h,w,3] RGB, volumes [B,15,G,G,G] float32, scale [B,15]
    -> out uint8 [B,h,w,3], ambiguous bool [B,h,w], maxima float64 [B,h,w,15]."""
    B, G = volumes.shape[0], volumes.shape[2]
    o, d = view_rays(rays, view12)
    out, amb, mx = np.zeros_like(base), np.zeros(base.shape[:3], dtype=bool), np.zeros(base.shape[:3] + (JOINTS,))
    for b in range(B):
        limit = np.full(base.shape[1:3], np.inf)
        if zbuf is not None:
            z = zbuf[b]
            zs = (z >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
            limit = np.where(z == EMPTY, np.inf, zs)
        live = live_mask(scale[b], joint_mask)
        hit, m, am = march(o, d, volumes[b], scale[b], G, S, near, limit, live)
        out[b], am2 = composite(base[b], hit, m, live, gain, opacity)
        amb[b], mx[b] = am | am2, m
    return out, amb, mx


def overlay(rays, depth, base, volumes, scale, S, near, joint_mask=ALL, gain=1.0, opacity=0.8):
    """rays [H,W,3] unit rays, depth None or [B,dh,dw] float32, base uint8 [B,H,W,3] RGB -> out, ambiguous, maxima."""
    B, G = volumes.shape[0], volumes.shape[2]
    H, W = base.shape[1:3]
    o = np.zeros(3)
    out, amb, mx = np.zeros_like(base), np.zeros(base.shape[:3], dtype=bool), np.zeros(base.shape[:3] + (JOINTS,))
    for b in range(B):
        limit = np.full((H, W), np.inf)
        if depth is not None:
            dh, dw = depth.shape[1:]
            limit = depth[b][(np.arange(H) * dh) // H][:, (np.arange(W) * dw) // W].astype(np.float64)
        live = live_mask(scale[b], joint_mask)
        hit, m, am = march(o, rays, volumes[b], scale[b], G, S, near, limit, live)
        out[b], am2 = composite(base[b], hit, m, live, gain, opacity)
        amb[b], mx[b] = am | am2, m
    return out, amb, mx


def brute_maxima(o, d, vol, scale, G, S, near, limit, live):
    """Independent of the walk and of the slab test of the whole box: for every cell, the slab interval of the ray with that cell's
    own box, clipped to [near, limit); the cell counts when what is left is not empty (the cells tile the box, so a ray that misses
    the box counts no cell).  Quotients, not products with a reciprocal.  -> m [..., 15] and a mask of pixels where some cell's
    decision is within the margin (a ray grazing a cell's edge, or a cell that the range just reaches)."""
    pos, h = grid(G, S)
    shape = d.shape[:-1]
    m = np.zeros(shape + (JOINTS,))
    graze = np.zeros(shape, dtype=bool)
    lim = np.broadcast_to(np.asarray(limit, dtype=np.float64), shape)[..., None]
    with np.errstate(all="ignore"):
        lo_t, hi_t = [], []                      # per axis: [..., G] entry / exit parameters of the G slabs
        for a in range(3):
            da = d[..., a][..., None]
            k = np.arange(G)
            lo, hi = bnd(pos[a], h, k), bnd(pos[a], h, k + 1)
            zero = da == 0.0
            ta, tb = (lo - o[a]) / np.where(zero, 1.0, da), (hi - o[a]) / np.where(zero, 1.0, da)
            inside = (o[a] >= lo) & (o[a] < hi)
            lo_t.append(np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb)))
            hi_t.append(np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb)))
        for ix in range(G):
            for iy in range(G):
                en = np.maximum(np.maximum(lo_t[0][..., ix], lo_t[1][..., iy])[..., None], lo_t[2])         # [..., G] over z
                ex = np.minimum(np.minimum(hi_t[0][..., ix], hi_t[1][..., iy])[..., None], hi_t[2])
                a0 = np.maximum(en, float(near))
                a1 = np.minimum(ex, lim)
                counted = a0 < a1                                                                           # false for any NaN
                graze |= (np.isfinite(a0) & np.isfinite(a1) & (_near(a0, a1) | ((np.abs(a0 - a1) < ABS_S) & (a1 == lim)))).any(axis=-1)
                for j in range(JOINTS):
                    if not (live >> j) & 1:
                        continue
                    v = vol[j, ix, iy].astype(np.float64) * scale[j]                                        # [G]
                    best = np.where(counted & (v > 0.0), v, 0.0).max(axis=-1)
                    m[..., j] = np.maximum(m[..., j], best)
    return m, graze
