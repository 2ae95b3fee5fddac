"""numpy float64 model of csrc/render.hip: a literal restatement of the arithmetic include/sceneego_hip.h states, operation by
operation (numpy rounds every product, sum, quotient and square root separately, as the unfused kernel does).

``splat``   -> the uint64 z-buffer, by a Python-level minimum over the keys (order-free by construction).
``trace``   -> per pixel: hit flag, ray parameter, colour, and the ``ambiguous`` mask: pixels where a last-bit difference in a square
               root or a quotient could legitimately flip a decision or a truncation.  The GPU tests compare every other pixel exactly
               and cap the ambiguous share, so the mask cannot hide a failure.
``resolve`` / ``overlay`` -> the composed images and their ambiguous masks.
"""
import numpy as np

BONES = [(0, 1), (0, 4), (1, 2), (2, 3), (4, 5), (5, 6), (1, 7), (4, 11), (7, 8), (8, 9), (9, 10), (11, 12), (12, 13), (13, 14),
         (7, 11)]       # Skeleton.lines, reference utils/skeleton.py:20-21
R_JOINT, R_BONE = 0.03, 0.0075
JOINT_RGB, BONE_RGB = (0.1, 0.1, 0.7), (0.1, 0.9, 0.1)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
REL, ABS_S, ABS_C = 1e-9, 1e-6, 1e-6


def splat(depth, ray_tab, image, view, f, cx, cy, Hout, Wout, splat, min_z, max_depth, near):
    """depth [B,dh,dw] float32, ray_tab [H,W,3] float64, image [B,H,W,3] uint8 BGR, view [12] -> zbuf [B,Hout,Wout] uint64."""
    B, dh, dw = depth.shape
    H, W, _ = ray_tab.shape
    R, t = np.asarray(view[:9], dtype=np.float64).reshape(3, 3), np.asarray(view[9:], dtype=np.float64)
    sy = (np.arange(H) * dh) // H
    sx = (np.arange(W) * dw) // W
    zbuf = np.full((B, Hout, Wout), EMPTY, dtype=np.uint64)
    off = (splat - 1) // 2
    with np.errstate(all="ignore"):
        for b in range(B):
            d = depth[b][sy][:, sx].astype(np.float64)
            keep = (d > 0.0) & (d <= max_depth)
            p = ray_tab * d[:, :, None]
            keep &= p[:, :, 2] > min_z
            q = [((R[i, 0] * p[:, :, 0] + R[i, 1] * p[:, :, 1]) + R[i, 2] * p[:, :, 2]) + t[i] for i in range(3)]
            keep &= q[2] > near
            u = (f * q[0]) / q[2] + cx
            v = (f * q[1]) / q[2] + cy
            keep &= (u >= -4.0) & (u < float(Wout + 4)) & (v >= -4.0) & (v < float(Hout + 4))
            iu = np.floor(u[keep]).astype(np.int64)
            iv = np.floor(v[keep]).astype(np.int64)
            zbits = q[2][keep].astype(np.float32).view(np.uint32).astype(np.uint64)
            c = image[b][keep].astype(np.uint64)              # B, G, R
            key = (zbits << np.uint64(32)) | (c[:, 2] << np.uint64(16)) | (c[:, 1] << np.uint64(8)) | c[:, 0]
            flat = zbuf[b].reshape(-1)
            for dy in range(splat):
                for dx in range(splat):
                    px, py = iu - off + dx, iv - off + dy
                    inside = (px >= 0) & (px < Wout) & (py >= 0) & (py < Hout)
                    np.minimum.at(flat, (py[inside] * Wout + px[inside]), key[inside])
    return zbuf


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def trace(rays, joints, near, r_joint=R_JOINT, r_bone=R_BONE, joint_rgb=JOINT_RGB, bone_rgb=BONE_RGB):
    """rays [h,w,3] float64, joints [15,3] float64 -> hit bool [h,w], s float64 [h,w], rgb uint8 [h,w,3], ambiguous bool [h,w]."""
    dx, dy, dz = rays[:, :, 0], rays[:, :, 1], rays[:, :, 2]
    shape = dx.shape
    best = np.full(shape, np.inf)
    second = np.full(shape, np.inf)          # the smallest candidate that did not become / stay the hit
    hit = np.zeros(shape, dtype=bool)
    kind = np.zeros(shape, dtype=np.int64)
    nx, ny, nz = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    amb = np.zeros(shape, dtype=bool)
    J = np.asarray(joints, dtype=np.float64)
    fin = np.isfinite(J).all(axis=1)

    def take(s, ok, k, n3):
        nonlocal best, second, hit, kind, nx, ny, nz
        better = ok & (~hit | (s < best))
        second = np.where(better, np.minimum(second, np.where(hit, best, np.inf)), np.where(ok, np.minimum(second, s), second))
        best = np.where(better, s, best)
        kind = np.where(better, k, kind)
        nx, ny, nz = np.where(better, n3[0], nx), np.where(better, n3[1], ny), np.where(better, n3[2], nz)
        hit = hit | better

    with np.errstate(all="ignore"):
        a = _dot(dx, dy, dz, dx, dy, dz)
        for j in range(15):
            if not fin[j]:
                continue
            c = J[j]
            bq = _dot(dx, dy, dz, c[0], c[1], c[2])
            cq = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) - r_joint * r_joint
            disc = bq * bq - a * cq
            amb |= np.abs(disc) <= REL * (bq * bq)
            ok = disc >= 0.0
            sq = np.sqrt(np.where(ok, disc, 0.0))
            for s in ((bq - sq) / a, (bq + sq) / a):
                take(s, ok & (s > near), 0, (s * dx - c[0], s * dy - c[1], s * dz - c[2]))
        for (ia, ib) in BONES:
            if not (fin[ia] and fin[ib]):
                continue
            A, Bj = J[ia], J[ib]
            vx, vy, vz = Bj[0] - A[0], Bj[1] - A[1], Bj[2] - A[2]
            vv = (vx * vx + vy * vy) + vz * vz
            if not (np.sqrt(vv) >= 1e-9):
                continue
            dv = _dot(dx, dy, dz, vx, vy, vz)
            av = (A[0] * vx + A[1] * vy) + A[2] * vz
            kd, ka = dv / vv, av / vv
            ex, ey, ez = dx - kd * vx, dy - kd * vy, dz - kd * vz
            gx, gy, gz = A[0] - ka * vx, A[1] - ka * vy, A[2] - ka * vz
            qa = _dot(ex, ey, ez, ex, ey, ez)
            qb = _dot(ex, ey, ez, gx, gy, gz)
            qc = ((gx * gx + gy * gy) + gz * gz) - r_bone * r_bone
            disc = qb * qb - qa * qc
            amb |= (qa > 0.0) & (np.abs(disc) <= REL * (qb * qb))
            ok = (qa > 0.0) & (disc >= 0.0)
            sq = np.sqrt(np.where(ok, disc, 0.0))
            qa1 = np.where(ok, qa, 1.0)
            for s in ((qb - sq) / qa1, (qb + sq) / qa1):
                t = (s * dv - av) / vv
                amb |= ok & ((np.abs(t) <= REL) | (np.abs(t - 1.0) <= REL))
                take(s, ok & (s > near) & (t >= 0.0) & (t <= 1.0), 1, (s * ex - gx, s * ey - gy, s * ez - gz))
        amb |= hit & (np.abs(second - best) <= REL)
        nn = np.sqrt((nx * nx + ny * ny) + nz * nz)
        dn = np.sqrt((dx * dx + dy * dy) + dz * dz)
        ndl = -(((nx * dx + ny * dy) + nz * dz) / (nn * dn))
        shade = 0.3 + 0.7 * np.where(ndl > 0.0, ndl, 0.0)
        rgb = np.zeros(shape + (3,), dtype=np.uint8)
        for c in range(3):
            base = np.where(kind == 0, float(np.float32(joint_rgb[c])), float(np.float32(bone_rgb[c])))
            val = (255.0 * base) * shade + 0.5
            amb |= hit & (np.abs(val - np.rint(val)) <= ABS_C)
            rgb[:, :, c] = np.clip(np.where(hit, val, 0.0).astype(np.int64), 0, 255)
    return hit, np.where(hit, best, np.inf), rgb, amb


def resolve(rays, joints, zbuf, near, background=(255, 255, 255), **kw):
    """joints [B,15,3] in the frame of rays, zbuf [B,h,w] uint64 -> out uint8 [B,h,w,3] RGB, ambiguous bool [B,h,w]."""
    B = zbuf.shape[0]
    out = np.zeros(zbuf.shape + (3,), dtype=np.uint8)
    amb = np.zeros(zbuf.shape, dtype=bool)
    for b in range(B):
        hit, s, rgb, am = trace(rays, joints[b], near, **kw)
        z = zbuf[b]
        empty = z == EMPTY
        zscene = (z >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            skel = hit & (empty | (s < zscene))
            am = am | (hit & ~empty & (np.abs(s - zscene) < ABS_S))
        w = np.where(empty, np.uint64((background[0] << 16) | (background[1] << 8) | background[2]), z)
        scene = np.stack([(w >> np.uint64(16)) & np.uint64(255), (w >> np.uint64(8)) & np.uint64(255), w & np.uint64(255)],
                         axis=-1).astype(np.uint8)
        out[b] = np.where(skel[:, :, None], rgb, scene)
        amb[b] = am
    return out, amb


def overlay(rays, joints, frame, near, depth=None, **kw):
    """joints [B,15,3] camera frame, frame [B,H,W,3] uint8 BGR, depth None or [B,dh,dw] float32 -> out uint8 [B,H,W,3] RGB, ambiguous."""
    B, H, W, _ = frame.shape
    out = np.zeros(frame.shape, dtype=np.uint8)
    amb = np.zeros((B, H, W), dtype=bool)
    for b in range(B):
        hit, s, rgb, am = trace(rays, joints[b], near, **kw)
        show = hit
        if depth is not None:
            dh, dw = depth.shape[1:]
            d = depth[b][(np.arange(H) * dh) // H][:, (np.arange(W) * dw) // W].astype(np.float64)
            with np.errstate(all="ignore"):
                show = hit & (s < d)
                am = am | (hit & (np.abs(s - d) < ABS_S))
        out[b] = np.where(show[:, :, None], rgb, frame[b][:, :, ::-1])
        amb[b] = am
    return out, amb
