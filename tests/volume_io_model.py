"""float64 numpy models of the kernels that build the V2V input and read its output: the voxeliser (csrc/voxelize.hip), the 4-tap
gather and the intersection pass (csrc/gather.hip, gather_bf16_kernel of csrc/conv3d_bf16.hip) and the soft-argmax
(csrc/softargmax.hip).  Written from the header comments of the entry points (include/sceneego_hip.h) and independent of
sceneego_amd/op.py: no torch operation takes part in the arithmetic.  The tests feed the models the SAME float32 / float64 / int32
arrays the code under test gets."""
import numpy as np

VOXELIZE_VARIANTS = ("exact", "prescale", "divfirst", "float32")


# ------------------------------------------------------------------------------------------------------------------ voxeliser
def nearest_index(dst, src):
    """cv2.resize INTER_NEAREST: source index of every destination index, min(floor(dst * (src / dst)), src - 1), scale in float64."""
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * (float(src) / float(dst))).astype(np.int64), src - 1)


def voxel_coordinate(p, off, G, side, variant="exact"):
    """round_half_even(((p + off) * G) / side), left to right, every operation rounded on its own (no fused multiply-add), in the
    float type of ``p``.  ``off`` None: no addition (the z axis).  The other variants are deliberately WRONG evaluations of the same
    real-number formula (tests/test_volume_io_host.py shows that the tie cases tell them from the right one)."""
    ft = p.dtype.type
    g, s = ft(G), ft(side)
    with np.errstate(all="ignore"):
        t = p if off is None else p + ft(off)
        if variant in ("exact", "float32"):
            q = (t * g) / s
        elif variant == "prescale":
            q = t * (g / s)
        elif variant == "divfirst":
            q = (t / s) * g
        else:
            raise ValueError(variant)
        return np.round(q)


def voxelize_model(depth, ray_tab, up, pad_x, G, side, variant="exact"):
    """The occupied set of se_voxelize_*_f64 as bool [B, G, G, G].
    depth float32 [B, dh, dw]; ray_tab float64 [up_h, up_w, 3]; ``up`` an int (square) or (up_h, up_w) - se_voxelize_full_f64 is the
    case up == (dh, dw), pad_x == 0.  Per pixel (y, x') of the resized map, as the header comment of the kernel lists it:
        d = depth[min(floor(y * (dh / up_h)), dh - 1)][min(floor(x' * (dw / up_w)), dw - 1)]       (as float64)
        p = ray * d;  q = round_half_even(((p + side / 2) * G) / side) for x and y, ((p * G) / side) for z
        0 <= q <= G - 1 on all three axes (a NaN fails): occ[qx][qy][qz] = 1
    and with pad_x > 0 the point (0, 0, 0) of the zero-padded columns goes through the same arithmetic once per sample."""
    depth = np.asarray(depth, dtype=np.float32)
    B, dh, dw = depth.shape
    up_h, up_w = (int(up), int(up)) if np.isscalar(up) else (int(up[0]), int(up[1]))
    ft = np.float32 if variant == "float32" else np.float64
    d = depth[:, nearest_index(up_h, dh)][:, :, nearest_index(up_w, dw)].astype(ft)            # [B, up_h, up_w]
    ray = np.asarray(ray_tab, dtype=np.float64).reshape(up_h, up_w, 3).astype(ft)
    half = ft(side) / ft(2)
    occ = np.zeros((B, G, G, G), dtype=bool)
    with np.errstate(all="ignore"):
        q = [voxel_coordinate(ray[None, :, :, a] * d, None if a == 2 else half, G, side, variant) for a in range(3)]
        good = np.ones(d.shape, dtype=bool)
        for a in range(3):
            good &= (q[a] >= 0) & (q[a] <= G - 1)
    b = np.broadcast_to(np.arange(B)[:, None, None], d.shape)[good]
    occ[b, q[0][good].astype(np.int64), q[1][good].astype(np.int64), q[2][good].astype(np.int64)] = True
    if pad_x > 0:
        z = np.zeros(1, dtype=ft)
        o = [voxel_coordinate(z, None if a == 2 else half, G, side, variant)[0] for a in range(3)]
        if all(0 <= v <= G - 1 for v in o):
            occ[:, int(o[0]), int(o[1]), int(o[2])] = True
    return occ


def place_dense(occ):
    """se_voxelize_f64 / se_voxelize_full_f64: the whole grid is cleared, then set."""
    return occ.astype(np.float32)


def place_strided(buf, occ, c_offset):
    """se_voxelize_strided_f64 on ``buf`` float32 [B, N, stride_c]: channels [c_offset, c_offset + 4) of every record are cleared,
    channel c_offset is the occupancy; everything else is left as it was."""
    out = buf.copy()
    out[:, :, c_offset:c_offset + 4] = 0.0
    out[:, :, c_offset] = occ.reshape(occ.shape[0], -1)
    return out


def place_planar3(buf, occ, channel):
    """se_voxelize_planar3_f64 on ``buf`` float32 [B, triplets_total, N, 3]: scatter only."""
    out = buf.copy()
    out[:, channel // 3, :, channel % 3][occ.reshape(occ.shape[0], -1)] = 1.0
    return out


def place_planar1(buf, occ, channel):
    """se_voxelize_planar1_f64 on ``buf`` float32 [B, planes_total, N]: scatter only."""
    out = buf.copy()
    out[:, channel][occ.reshape(occ.shape[0], -1)] = 1.0
    return out


BF16_ONE = 0x3F80


def place_octet_bf16(buf, occ, c_offset):
    """se_voxelize_strided_bf16 on ``buf`` uint16 (bfloat16 bits) [B, octs_total, N, 8]: the 8 channels of octet c_offset / 8 are
    cleared, lane 0 is the occupancy; the other octets are left as they were."""
    out = buf.copy()
    out[:, c_offset // 8] = 0
    out[:, c_offset // 8, :, 0] = np.where(occ.reshape(occ.shape[0], -1), BF16_ONE, 0).astype(np.uint16)
    return out


# ------------------------------------------------------------------------------------------------------------------ gather
def gather_model(feat, idx, w):
    """feat float32 [B, texels, C], idx int32 [V, 4], w float32 [V, 4] -> (sum float64 [B, V, C] of the four products feat[idx] * w with
    the taps idx < 0 skipped, S = sum of |feat[idx] * w| over the same taps: what a float32 rounding bound is relative to)."""
    f = feat.astype(np.float64)
    B, _, C = f.shape
    V = idx.shape[0]
    out = np.zeros((B, V, C))
    mag = np.zeros((B, V, C))
    for k in range(4):
        live = idx[:, k] >= 0
        prod = f[:, np.where(live, idx[:, k], 0), :] * w[:, k].astype(np.float64)[None, :, None]
        prod = np.where(live[None, :, None], prod, 0.0)
        out += prod
        mag += np.abs(prod)
    return out, mag


def to_planar3(x, triplets_total, fill):
    """channels-last [B, V, C] -> triplet-planar [B, triplets_total, V, 3]; slots >= C hold ``fill``."""
    B, V, C = x.shape
    full = np.full((B, V, triplets_total * 3), fill, dtype=x.dtype)
    full[:, :, :C] = x
    return np.ascontiguousarray(full.reshape(B, V, triplets_total, 3).transpose(0, 2, 1, 3))


def to_planar1(x, planes_total, fill):
    """channels-last [B, V, C] -> planar [B, planes_total, V]; planes >= C hold ``fill``."""
    B, V, C = x.shape
    full = np.full((B, planes_total, V), fill, dtype=x.dtype)
    full[:, :C] = x.transpose(0, 2, 1)
    return full


def bf16_round(x):
    """float32 -> bfloat16 bits (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def intersection_model(buf, occ, channels):
    """se_intersection_f32 on ``buf`` float32 [B, V, stride_c], occ float32 [B, V]: channels [C, 2C) = channels [0, C) * occ, one float32
    multiplication each; everything else is left as it was."""
    out = buf.copy()
    out[:, :, channels:2 * channels] = buf[:, :, :channels] * occ[:, :, None]       # float32 * float32 -> float32: one rounding
    return out


# ------------------------------------------------------------------------------------------------------------------ soft-argmax
def softargmax_model(logits, coord, mode):
    """logits float32 [rows, N], coord float32 [N, 3] -> dict of float64 arrays:
        vol [rows, N]   softmax over the row (mode 1) or relu (mode 0)
        joints [rows, 3] = sum_n vol[n] * coord[n]      (mode 0: NOT normalised, as the header defines it)
        A [rows, 3]     = sum_n vol[n] * |coord[n]|: what a float32 summation bound of the joints is relative to
        D [rows]        = sum_n vol[n] * (M - x[n]) with M the row's maximum (mode 1; 0 in mode 0): the weight-averaged size of the
                          argument of exp, which the rounding of x - M is relative to
        Dc [rows, 3]    = sum_n vol[n] * |coord[n]| * (M - x[n]): the same, weighted like the joints' sums
        peak [rows]     = max_n vol[n]
    A -inf logit has probability exactly 0.  A row that holds a NaN, or nothing but -inf, is NaN throughout (as torch.softmax)."""
    x = logits.astype(np.float64)
    c = coord.astype(np.float64)
    rows, N = x.shape
    vol = np.empty((rows, N))
    D = np.zeros(rows)
    Dc = np.zeros((rows, 3))
    with np.errstate(all="ignore"):
        if mode == 1:
            M = x.max(axis=1)                                       # NaN if the row holds one
            for r in range(rows):
                if not np.isfinite(M[r]):                           # NaN, or -inf throughout (+inf is not a case of these tests)
                    vol[r] = np.nan
                    D[r] = Dc[r] = np.nan
                    continue
                t = M[r] - x[r]                                     # >= 0, +inf at a -inf logit
                e = np.exp(-t)
                vol[r] = e / e.sum()
                tf = np.where(np.isfinite(t), t, 0.0)
                D[r] = (vol[r] * tf).sum()
                Dc[r] = (vol[r] * tf) @ np.abs(c)
        elif mode == 0:
            vol = np.maximum(x, 0.0)
            vol[np.isnan(x)] = np.nan
        else:
            raise ValueError(mode)
        joints = vol @ c
        A = vol @ np.abs(c)
        peak = vol.max(axis=1)
    return {"vol": vol, "joints": joints, "A": A, "D": D, "Dc": Dc, "peak": peak}
