"""Inputs of the scene-probe tests, built once and shared by tests/test_scene_host.py (model properties, on the CPU) and
tests/test_gpu_scene_check.py (the kernel against tests/scene_model.py, bit for bit).  numpy only."""
import functools

import numpy as np

import render_cases as RC
import scene_model as M
from conftest import CALIB
from sceneego_amd.fisheye import FishEyeCameraCalibrated

MIN_Z, MAX_DEPTH = RC.MIN_Z, RC.MAX_DEPTH
FULL_H, FULL_W = 1024, 1280


@functools.lru_cache(maxsize=None)
def ray_table(H, W, margin=0.0):
    """[H, W, 3] float64: the test calibration's unit rays on an H x W lattice over the frame without a ``margin`` share on every
    side.  margin = 0 reaches the corners, whose rays point backwards (z < 0: dropped by the min_z rule); 0.25 keeps z > 0.1."""
    cam = FishEyeCameraCalibrated(CALIB)
    ys = np.rint(np.linspace(margin * FULL_H, (1.0 - margin) * FULL_H - 1, H))
    xs = np.rint(np.linspace(margin * FULL_W, (1.0 - margin) * FULL_W - 1, W))
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    return np.ascontiguousarray(cam.camera2world_ray(np.stack([xx.reshape(-1), yy.reshape(-1)], axis=1)).reshape(H, W, 3))


def smooth_depth(B, dh, dw, seed):
    """Smooth 0.5 - 6 m (the generator of render_cases.depth_map, without its patches)."""
    rng = np.random.default_rng(seed + 100 * dh + B)
    y, x = np.meshgrid(np.linspace(0, 1, dh), np.linspace(0, 1, dw), indexing="ij")
    d = np.empty((B, dh, dw), dtype=np.float32)
    for b in range(B):
        a = rng.uniform(2.0, 7.0, size=4)
        ph = rng.uniform(0, 6.28, size=2)
        d[b] = 0.5 + 5.5 * (0.5 + 0.5 * np.sin(a[0] * x + a[1] * y + ph[0]) * np.cos(a[2] * x - a[3] * y + ph[1]))
    return d


def add_patches(d):
    """Patches of 0, negative, 150 (> max_depth), NaN and +inf, and one of 0.05 m (a surface whose point has s.z <= min_z)."""
    dh = d.shape[1]
    s = max(1, dh // 16)
    for k, val in enumerate((0.0, -1.5, 150.0, np.nan, np.inf, 0.05)):
        r0, c0 = (1 + 2 * k) * s, (2 + 3 * k) * s
        d[:, r0:r0 + s, c0:c0 + s] = val
    return d


def random_probes(B, P, seed):
    """Points inside the cuboid the network predicts in, in front of the camera."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.8, 0.8, (B, P)), rng.uniform(-0.8, 0.8, (B, P)), rng.uniform(0.2, 1.8, (B, P))], axis=2)


def on_scene_point(k, b, p, n):
    """Sets probe (b, p) of case ``k`` exactly on the scene point of pixel n (which must be one)."""
    _, _, s, is_scene, _ = M.scene(k["depth"], k["ray_tab"], MIN_Z, MAX_DEPTH)
    assert is_scene[b, n], (b, n)
    k["probes"][b, p] = s[b, n]


def _small(dirty):
    d = smooth_depth(2, 12, 20, seed=3)
    tab = ray_table(24, 40).copy()
    if dirty:
        add_patches(d)
        tab[0, 0] = np.nan                                    # a corner of NaN / inf rays: those pixels take part in nothing
        tab[0, 1, 1] = np.inf
        tab[1, 0, 2] = -np.inf
        tab[23, 39, 0] = np.nan
    k = dict(depth=d, ray_tab=tab, probes=random_probes(2, 15, seed=21))
    on_scene_point(k, 1, 4, int(np.flatnonzero(M.scene(d, tab, MIN_Z, MAX_DEPTH)[3][1])[37]))
    return k


def _odd(P):
    d = RC.depth_map(3, 19, 27).copy()                        # with the patches of render_cases
    return dict(depth=d, ray_tab=ray_table(37, 53), probes=random_probes(3, P, seed=30 + P))


def _multi_tile():
    d = smooth_depth(2, 65, 129, seed=5)
    k = dict(depth=d, ray_tab=ray_table(130, 257, margin=0.25), probes=random_probes(2, 60, seed=41))
    on_scene_point(k, 1, 59, 130 * 257 - 1)                   # the very last pixel: the last lane that holds one in the last, partial tile
    on_scene_point(k, 0, 0, 2048)                             # the first pixel of the second tile
    return k


def _empty_frame():
    d = smooth_depth(3, 12, 20, seed=7)
    d[1] = 0.0
    return dict(depth=d, ray_tab=ray_table(24, 40), probes=random_probes(3, 15, seed=51))


def _bad_probe():
    k = dict(depth=smooth_depth(2, 12, 20, seed=3), ray_tab=ray_table(24, 40), probes=random_probes(2, 15, seed=21))
    k["probes"][0, 3, 1] = np.nan
    k["probes"][1, 14, 2] = np.inf
    return k


def _ties():
    t = RC.tie_inputs()                                       # rays in 4 x 4 blocks of equal rays, one depth per block
    k = dict(depth=t["depth"].copy(), ray_tab=t["ray_tab"], probes=random_probes(1, 15, seed=61))
    _, _, s, is_scene, _ = M.scene(k["depth"], k["ray_tab"], MIN_Z, MAX_DEPTH)
    blocks = np.flatnonzero(is_scene[0])
    # probes ON a block's scene point (16 pixels at q = 0) and along a block's ray (16 pixels at the same t): from pixels that are
    # NOT the first of their block, so that taking the probe's own pixel would be wrong
    for p, n in ((0, blocks[len(blocks) // 2 + 5]), (1, blocks[-1])):
        k["probes"][0, p] = s[0, n]
    k["probes"][0, 2] = k["ray_tab"].reshape(-1, 3)[blocks[len(blocks) // 3 + 7]] * 0.75
    return k


BUILDERS = {"small": lambda: _small(False), "odd_p1": lambda: _odd(1), "odd_p45": lambda: _odd(45), "odd_p64": lambda: _odd(64),
            "multi_tile": _multi_tile, "dirty": lambda: _small(True), "empty_frame": _empty_frame, "bad_probe": _bad_probe,
            "ties": _ties}
CASES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(depth [B,dh,dw] float32, ray_tab [H,W,3] float64, probes [B,P,3] float64); shared: do not write to it."""
    k = BUILDERS[name]()
    for a in k.values():
        a.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def model(name):
    k = inputs(name)
    return M.probe(k["depth"], k["ray_tab"], k["probes"], MIN_Z, MAX_DEPTH)
