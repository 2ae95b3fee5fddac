"""Inputs of the volume-renderer tests, built once and shared by tests/test_volume_render_host.py (which checks, on the CPU, that
the model's ambiguous share on every one of them is within the cap, and the model against a brute-force formulation) and
tests/test_gpu_volume_render.py (which runs them on the device).  numpy only.

The shapes are the smallest at which the kernel can still go wrong: G = 8, 12 (no multiple of 8 or 16: the last workgroup of the pack
pass is partial), 16, and one G = 64 case; B = 1 and 3; the 32 x 40 ray table and the 48 x 64 view of render_cases.py (neither is a
multiple of the 16 x 16 pixel tile in both directions); an eye inside the box (SIDE_VIEW) and outside it (orbit_view())."""
import functools

import numpy as np

import render_cases as RC
import volume_render_model as M
from sceneego_amd.render import orbit_view

S = 2.0                          # cuboid side, metres (the project's configuration)
NEAR = RC.NEAR
AMBIGUOUS_CAP = RC.AMBIGUOUS_CAP  # the project's existing figure: a condition on the cases, not a measurement
HOUT, WOUT = 48, 64
VIEWS = {"side": RC.SIDE_VIEW, "orbit": orbit_view(), "identity": RC.IDENTITY}
CORNER_JOINT, ZERO_JOINT, NAN_JOINT, OFF_JOINT = 3, 5, 2, 7
ONE = 1 << 9                     # the single-joint mask: the right ankle


@functools.lru_cache(maxsize=None)
def volumes(B, G, seed=17):
    """[B,15,G,G,G] float32: two Gaussian lobes per joint with peaks 1 and 0.6 (a maximum taken wrongly shows); joint 3 is one corner
    cell; joint 5 is all zero; joint 2 has one NaN cell, in the middle of its higher lobe."""
    rng = np.random.default_rng(seed + 10 * G + B)
    ax = np.arange(G, dtype=np.float64)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    v = np.zeros((B, M.JOINTS, G, G, G), dtype=np.float32)
    for b in range(B):
        for j in range(M.JOINTS):
            c = rng.uniform(0.15 * G, 0.85 * G, size=(2, 3))
            sig = rng.uniform(0.06 * G, 0.12 * G, size=2) + 0.5
            lobes = [amp * np.exp(-((x - c[k, 0]) ** 2 + (y - c[k, 1]) ** 2 + (z - c[k, 2]) ** 2) / (2 * sig[k] ** 2))
                     for k, amp in enumerate((1.0, 0.6))]
            v[b, j] = (0.02 * (lobes[0] + lobes[1])).astype(np.float32)
            if j == NAN_JOINT:
                i = np.clip(np.rint(c[0]).astype(int), 0, G - 1)
                v[b, j, i[0], i[1], i[2]] = np.nan
        v[b, CORNER_JOINT] = 0.0
        v[b, CORNER_JOINT, G - 1, 0, G - 1] = 0.03
        v[b, ZERO_JOINT] = 0.0
    return v


@functools.lru_cache(maxsize=None)
def scales(B, G):
    """[B,15] float64: 0.9 / the joint's largest finite value (so that gain 1 never reaches the clamp and gain 4 does), joint 7 is
    switched off by a scale of 0, the all-zero joint 5 by the infinite scale its maximum gives."""
    v = volumes(B, G)
    with np.errstate(all="ignore"):
        s = 0.9 / np.nanmax(v.reshape(B, M.JOINTS, -1), axis=2).astype(np.float64)
    s[:, OFF_JOINT] = 0.0
    return s


@functools.lru_cache(maxsize=None)
def base_view(B):
    return np.random.default_rng(31 + B).integers(0, 256, size=(B, HOUT, WOUT, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def base_frame(B):
    return np.random.default_rng(37 + B).integers(0, 256, size=(B, RC.H, RC.W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def ramp_zbuf(B):
    """Keys whose depth runs from 1.5 m to 5 m across the picture (the limit falls inside the box for both eyes), with a band of
    empty keys; the colour half is arbitrary."""
    rng = np.random.default_rng(41 + B)
    z = (1.5 + 3.5 * (np.arange(WOUT) / (WOUT - 1.0)))[None, None, :] + 0.3 * rng.random((B, HOUT, 1))
    key = (z.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 24, size=z.shape).astype(np.uint64)
    key = np.broadcast_to(key, (B, HOUT, WOUT)).copy()
    key[:, 20:26, :] = M.EMPTY
    return key


def zbuf(name, B):
    if name == "none":
        return None
    if name == "wall":
        return np.concatenate([np.roll(RC.wall_zbuf(), 16 * b, axis=2) for b in range(B)], axis=0)
    return ramp_zbuf(B)


def depth(name, B):
    if name == "none":
        return None
    if name == "wall":
        return np.concatenate([np.roll(RC.wall_depth(), 5 * b, axis=2) for b in range(B)], axis=0)
    return RC.depth_map(B, 16, 20)          # smooth 0.5 - 6 m with patches of 0, negative, 150, NaN and +inf


#             name                     B   G  view      zbuf    mask   gain
VIEW_CASES = [(f"g{G}_b{B}_{v}_{z}", B, G, v, z, M.ALL, 1.0)
              for G in (8, 12, 16) for B in (1, 3) for v, z in (("side", "ramp"), ("orbit", "wall"))]
VIEW_CASES += [("g12_side_open", 1, 12, "side", "none", M.ALL, 1.0), ("g12_orbit_open", 1, 12, "orbit", "none", M.ALL, 1.0),
               ("g12_orbit_ramp", 1, 12, "orbit", "ramp", M.ALL, 1.0), ("g12_side_wall", 1, 12, "side", "wall", M.ALL, 1.0),
               ("g12_orbit_one", 1, 12, "orbit", "none", ONE, 1.0), ("g12_side_one", 1, 12, "side", "ramp", ONE, 1.0),
               ("g12_orbit_nomask", 1, 12, "orbit", "none", 0, 1.0), ("g16_orbit_gain", 1, 16, "orbit", "none", M.ALL, 4.0),
               ("g16_side_gain", 3, 16, "side", "ramp", M.ALL, 4.0), ("g64_orbit", 1, 64, "orbit", "ramp", M.ALL, 1.0)]
#                name                 B   G  depth    mask   gain
OVERLAY_CASES = [(f"g{G}_b{B}_{d}", B, G, d, M.ALL, 1.0) for G in (8, 12, 16) for B, d in ((1, "wall"), (3, "map"))]
OVERLAY_CASES += [("g12_open", 1, 12, "none", M.ALL, 1.0), ("g12_one", 1, 12, "wall", ONE, 1.0), ("g12_nomask", 1, 12, "none", 0, 1.0),
                  ("g16_gain", 1, 16, "none", M.ALL, 4.0), ("g8_b3_wall", 3, 8, "wall", M.ALL, 1.0), ("g64_map", 1, 64, "map", M.ALL, 1.0)]
OPACITY = 0.8


def view_case(name):
    return next(c for c in VIEW_CASES if c[0] == name)


def overlay_case(name):
    return next(c for c in OVERLAY_CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def view_model(name):
    """-> out [B,48,64,3], ambiguous [B,48,64], maxima [B,48,64,15]."""
    _, B, G, v, z, mask, gain = view_case(name)
    return M.view(RC.pinhole_rays(HOUT, WOUT), VIEWS[v], zbuf(z, B), base_view(B), volumes(B, G), scales(B, G), S, NEAR,
                  joint_mask=mask, gain=gain, opacity=OPACITY)


@functools.lru_cache(maxsize=None)
def overlay_model(name):
    _, B, G, d, mask, gain = overlay_case(name)
    return M.overlay(RC.ray_table(), depth(d, B), base_frame(B), volumes(B, G), scales(B, G), S, NEAR, joint_mask=mask, gain=gain,
                     opacity=OPACITY)


# ------------------------------------------------------------------------------------------------ the hand-made ray table
# Directions with exact zeros, among them exactly (0, 0, 1) and (1, 0, 0): an axis with d == 0 is never stepped on and must not be
# divided by.  The origins lie off every cell boundary of G = 8 and 12 (checked by the host test: no pixel is ambiguous); from the
# outside origin the rays along z and y miss the box (their x lies outside its slab), the ray along +x crosses it.
HAND_DIRS = np.array([(0, 0, 1), (1, 0, 0), (0, 1, 0), (0, 0, -1), (-1, 0, 0), (0, -1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 0), (1, -1, 0),
                      (0.3, 0, 1), (0, -0.2, 1), (1, 0.25, 0), (0.5, 0.25, 1), (-0.4, 0.7, 1), (0.1, 0.2, -1)], dtype=np.float64)
HAND_ORIGINS = {"inside": (0.13, -0.21, 0.77), "outside": (-1.7, 0.31, 0.52)}
HAND_CASES = [(o, G) for o in ("inside", "outside") for G in (8, 12)]


def hand_rays():
    return np.ascontiguousarray(HAND_DIRS.reshape(4, 4, 3))


def hand_view(origin):
    """Identity rotation, t = -origin: the eye of the view is the origin and the table's directions are used as they are."""
    return np.concatenate([RC.IDENTITY[:9], -np.asarray(HAND_ORIGINS[origin], dtype=np.float64)])


@functools.lru_cache(maxsize=None)
def hand_base():
    return np.random.default_rng(43).integers(0, 256, size=(1, 4, 4, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def hand_model(origin, G):
    return M.view(hand_rays(), hand_view(origin), None, hand_base(), volumes(1, G), scales(1, G), S, 0.0, joint_mask=M.ALL, gain=1.0,
                  opacity=OPACITY)
