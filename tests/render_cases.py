"""Inputs of the renderer tests, built once and shared by tests/test_render_host.py (which checks, on the CPU, that the model's
ambiguous share on every one of them is within the cap) and tests/test_gpu_render.py (which runs them on the device).  numpy only."""
import functools
import os

import numpy as np

from conftest import CALIB, GOLD
from sceneego_amd.fisheye import FishEyeCameraCalibrated
from sceneego_amd.render import look_at, pinhole_ray_table

import render_model as M

H, W = 32, 40                    # the small "frame": every 32nd pixel of the 1024 x 1280 camera
NEAR, MIN_Z, MAX_DEPTH = 0.05, 0.1, 100.0
FOV = 50.0
AMBIGUOUS_CAP = 0.005
IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
# a camera inside the cloud looking sideways: part of the cloud is behind it and part leaves the frame on every side
SIDE_VIEW = look_at((0.2, 0.1, 1.2), (1.5, 0.3, 2.5), (0.0, 0.0, -1.0))
BIG = dict(r_joint=0.12, r_bone=0.04)          # radii a 32 x 40 / 48 x 64 image resolves; the defaults are sub-pixel there


@functools.lru_cache(maxsize=None)
def ray_table():
    """[H, W, 3] float64: the test calibration's unit rays at the centres of 32 x 32 pixel blocks of the full frame."""
    cam = FishEyeCameraCalibrated(CALIB)
    ys, xs = np.meshgrid(np.arange(H) * 32 + 16, np.arange(W) * 32 + 16, indexing="ij")
    return np.ascontiguousarray(cam.camera2world_ray(np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1)).reshape(H, W, 3))


def pinhole(Hout, Wout):
    f = (Hout / 2.0) / np.tan(np.radians(FOV) / 2.0)
    return f, Wout / 2.0, Hout / 2.0


def pinhole_rays(Hout, Wout):
    return pinhole_ray_table(Hout, Wout, *pinhole(Hout, Wout))


@functools.lru_cache(maxsize=None)
def depth_map(B, dh, dw, seed=3):
    """Smooth 0.5 - 6 m with patches of 0, negative, 150 (> max_depth), NaN and +inf."""
    rng = np.random.default_rng(seed + 100 * dh + B)
    y, x = np.meshgrid(np.linspace(0, 1, dh), np.linspace(0, 1, dw), indexing="ij")
    d = np.empty((B, dh, dw), dtype=np.float32)
    for b in range(B):
        a = rng.uniform(2.0, 7.0, size=4)
        ph = rng.uniform(0, 6.28, size=2)
        d[b] = 0.5 + 5.5 * (0.5 + 0.5 * np.sin(a[0] * x + a[1] * y + ph[0]) * np.cos(a[2] * x - a[3] * y + ph[1]))
        s = dh // 16                                    # patch size: 2 x 2 at 32 x 40, 1 x 1 at 16 x 20
        for k, val in enumerate((0.0, -1.5, 150.0, np.nan, np.inf)):
            r0, c0 = (3 + 2 * k) * s, (4 + 3 * k) * s
            d[b, r0:r0 + 2 * s, c0:c0 + 2 * s] = val
    return d


@functools.lru_cache(maxsize=None)
def image(B, seed=11):
    return np.random.default_rng(seed + B).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)


#              name            B  depth size  out size  splat  view
SPLAT_CASES = [(f"b{B}_d{dh}_o{Ho}_s{s}", B, (dh, dh * 5 // 4), (Ho, Ho * 4 // 3), s, "side")
               for B in (1, 3) for dh in (32, 16) for Ho in (24, 48) for s in (1, 2, 3)]
SPLAT_CASES += [("contention_4x4", 1, (32, 40), (4, 4), 2, "identity"), ("identity_s4", 1, (16, 20), (48, 64), 4, "identity")]
VIEWS = {"side": SIDE_VIEW, "identity": IDENTITY}


def splat_inputs(name):
    _, B, (dh, dw), (Ho, Wo), s, view = next(c for c in SPLAT_CASES if c[0] == name)
    return dict(depth=depth_map(B, dh, dw), ray_tab=ray_table(), image=image(B), view=VIEWS[view], Hout=Ho, Wout=Wo, splat=s)


@functools.lru_cache(maxsize=None)
def splat_model(name):
    k = splat_inputs(name)
    f, cx, cy = pinhole(k["Hout"], k["Wout"])
    return M.splat(k["depth"], k["ray_tab"], k["image"], k["view"], f, cx, cy, k["Hout"], k["Wout"], k["splat"], MIN_Z, MAX_DEPTH, NEAR)


def tie_inputs():
    """4 x 4 blocks of frame pixels share one ray and one depth; colours differ: the lowest colour word of a block must win."""
    rays = ray_table()[2::4, 2::4]                                        # [8, 10, 3]
    tab = np.ascontiguousarray(np.repeat(np.repeat(rays, 4, axis=0), 4, axis=1))
    rng = np.random.default_rng(5)
    block_depth = rng.uniform(1.0, 4.0, size=(1, 8, 10)).astype(np.float32)
    return dict(depth=block_depth, ray_tab=tab, image=image(1, seed=23), view=IDENTITY, Hout=48, Wout=64, splat=1)


# ------------------------------------------------------------------------------------------------------------------ skeletons
@functools.lru_cache(maxsize=None)
def golden_joints():
    return np.load(os.path.join(GOLD, "demo_exr_b1.npz"))["joints"][0].astype(np.float64)


def random_joints(seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.5, 0.5, 15), rng.uniform(-0.4, 0.4, 15), rng.uniform(0.8, 2.0, 15)], axis=1)


def wall_depth():
    """0.8 m over the left half of the frame (nearer than the skeleton), 5 m over the right half."""
    d = np.full((1, 16, 20), 5.0, dtype=np.float32)
    d[:, :, :10] = 0.8
    return d


@functools.lru_cache(maxsize=None)
def skeletons():
    """name -> joints [15, 3] float64 in the frame of the rays."""
    g = golden_joints()
    out = {"golden": g, "random7": random_joints(7), "random8": random_joints(8)}
    c = random_joints(9)
    # bone (2, 3) has zero length.  Two identical spheres tie on every pixel they cover, which the model counts as ambiguous (two
    # candidate roots within 1e-9), so the pair sits 4 m away where it covers under 0.5 % of the 48 x 64 image even at the big radius
    c[2] = c[3] = (0.3, 0.2, 4.0)
    out["coincident"] = c
    n = g.copy()
    n[5] = np.nan                                # sphere 5 and bones (4, 5), (5, 6) vanish
    out["nan_joint"] = n
    b = g.copy()
    b[9] = (0.1, -0.2, -0.6)                     # behind the camera: its sphere is invisible, bone (8, 9) crosses the near plane
    out["behind"] = b
    out["no_hit"] = g + np.array([60.0, 0.0, 0.0])
    return out


@functools.lru_cache(maxsize=None)
def wall_zbuf():
    f, cx, cy = pinhole(48, 64)
    return M.splat(wall_depth(), ray_table(), image(1), IDENTITY, f, cx, cy, 48, 64, 4, MIN_Z, MAX_DEPTH, NEAR)


def zbufs():
    return {"empty": np.full((1, 48, 64), M.EMPTY, dtype=np.uint64), "splat": splat_model("identity_s4"), "wall": wall_zbuf()}


RESOLVE_CASES = [(s, z, r) for s in ("golden", "random7", "random8", "coincident", "nan_joint", "behind", "no_hit")
                 for z in ("empty", "splat", "wall") for r in ("default", "big")]
OVERLAY_CASES = [(s, d, r) for s in ("golden", "random7", "nan_joint", "behind", "no_hit") for d in ("none", "wall")
                 for r in ("default", "big")]


def radii(r):
    return BIG if r == "big" else {}


@functools.lru_cache(maxsize=None)
def resolve_model(skel, zname, r):
    return M.resolve(pinhole_rays(48, 64), skeletons()[skel][None], zbufs()[zname], NEAR, background=(250, 240, 230), **radii(r))


@functools.lru_cache(maxsize=None)
def overlay_model(skel, dname, r):
    depth = wall_depth() if dname == "wall" else None
    return M.overlay(ray_table(), skeletons()[skel][None], image(1), NEAR, depth=depth, **radii(r))
