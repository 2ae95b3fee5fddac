"""CPU: the host side of the renderer (sceneego_amd/render.py, visualize.py, the --render_dir flags) and the conditions the GPU
tests of csrc/render.hip rest on: the numpy model's ambiguous share on every GPU test input is within the cap, and the splat inputs
really exercise what they are meant to (points behind the camera, points leaving the frame on every side, clipped footprints)."""
import numpy as np
import pytest
import torch

import render_cases as C
import render_model as M
from sceneego_amd import _lib
from sceneego_amd.render import look_at, orbit_view, read_ply, write_ply


def _R_t(view):
    return view[:9].reshape(3, 3), view[9:]


@pytest.mark.parametrize("view,target", [(look_at((1.0, 2.0, -0.5), (0.2, -0.1, 1.3), (0, 0, -1)), (0.2, -0.1, 1.3)),
                                         (look_at((0, 0, 0), (0, 0, 1), (0, -1, 0)), (0, 0, 1)),
                                         (orbit_view(), (0, 0, 1)), (orbit_view(200.0, -40.0, 2.0, (0.3, 0.1, 0.8)), (0.3, 0.1, 0.8))])
def test_views_are_rotations_that_centre_the_target(view, target):
    assert view.dtype == np.float64 and view.shape == (12,)
    R, t = _R_t(view)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
    q = R @ np.asarray(target, dtype=np.float64) + t
    assert q[2] > 0 and abs(q[0]) < 1e-12 and abs(q[1]) < 1e-12        # u = f x / z + cx = cx: the image centre


def test_look_at_image_axes():
    R, t = _R_t(look_at((0, 0, 0), (0, 0, 1), (0, -1, 0)))            # the head camera itself: image up is -y
    assert np.allclose(R, np.eye(3)) and np.allclose(t, 0)
    R, t = _R_t(orbit_view(azimuth_deg=0.0, elevation_deg=30.0))
    assert (R @ np.array([0, 0, 0.0]) + t)[1] < 0                      # the head camera (origin) appears above the cuboid centre
    with pytest.raises(ValueError):
        look_at((0, 0, 0), (0, 0, 1), (0, 0, -1))


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((257, 3)).astype(np.float32)
    pts[3] = (np.float32(1e-30), -0.0, 3.4e38)
    rgb = rng.integers(0, 256, size=(257, 3), dtype=np.uint8)
    path = str(tmp_path / "cloud.ply")
    write_ply(path, torch.from_numpy(pts), rgb)
    p2, c2 = read_ply(path)
    assert p2.dtype == np.float32 and c2.dtype == np.uint8
    assert np.array_equal(p2.view(np.uint32), pts.view(np.uint32)) and np.array_equal(c2, rgb)
    head = open(path, "rb").read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 257\n")
    write_ply(path, pts[:0], rgb[:0])
    assert read_ply(path)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(path, pts, rgb[:5])


def test_script_arguments(tmp_path):
    import demo
    import visualize
    a = visualize.parse_args(["--img_path", "a.jpg", "--depth_path", "a.exr", "--pose_path", "a.pkl"])
    assert (a.img_path, a.depth_path, a.pose_path) == ("a.jpg", "a.exr", "a.pkl")
    assert a.output == "render.png" and a.overlay == "overlay.png" and a.ply == "scene.ply"
    a = visualize.parse_args(["--img_path", "a.jpg", "--depth_path", "a.exr", "--pose_path", "a.pkl", "--size", "360x480",
                              "--azimuth", "10", "--elevation", "5", "--distance", "2", "--fov", "40", "--splat", "3"])
    assert a.size == (360, 480) and a.splat == 3 and a.fov == 40.0
    with pytest.raises(SystemExit):
        visualize.parse_args(["--img_path", "a.jpg", "--depth_path", "a.exr"])
    d = demo.parse_args(["--render_dir", str(tmp_path)])
    assert d.render_dir == str(tmp_path) and demo.parse_args([]).render_dir is None
    with pytest.raises(SystemExit):
        demo.parse_args(["--vis", "true"])


def test_wrappers_refuse_cpu_tensors():
    rays = torch.zeros((4, 4, 3), dtype=torch.float64)
    joints = torch.zeros((1, 15, 3), dtype=torch.float64)
    zbuf = torch.zeros((1, 4, 4), dtype=torch.int64)
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(_lib.HipExtensionError):
        _lib.render_splat(torch.zeros((1, 4, 4)), rays, img, torch.zeros(12, dtype=torch.float64), zbuf, 4.0, 2.0, 2.0)
    with pytest.raises(_lib.HipExtensionError):
        _lib.render_resolve(rays, joints, zbuf, img.clone())
    with pytest.raises(_lib.HipExtensionError):
        _lib.render_overlay(rays, joints, img, img.clone())
    from sceneego_amd.render import SceneRenderer
    with pytest.raises(_lib.HipExtensionError):
        SceneRenderer(C.CALIB, device="cpu")


# ------------------------------------------------------------------------------------------------ conditions of the GPU tests
def test_side_view_inputs_exercise_every_drop_rule():
    k = C.splat_inputs("b1_d32_o24_s3")
    R, t = _R_t(k["view"])
    d = k["depth"][0].astype(np.float64)
    with np.errstate(all="ignore"):
        valid = (d > 0) & (d <= C.MAX_DEPTH)
        p = k["ray_tab"] * d[:, :, None]
        valid &= p[:, :, 2] > C.MIN_Z
        q = p @ R.T + t
        f, cx, cy = C.pinhole(24, 32)
        front = valid & (q[:, :, 2] > C.NEAR)
        u, v = f * q[:, :, 0] / q[:, :, 2] + cx, f * q[:, :, 1] / q[:, :, 2] + cy
    assert (~np.isfinite(d)).sum() > 0 and (d <= 0).sum() > 0 and (d > C.MAX_DEPTH).sum() > 0
    assert (valid & ~front).sum() > 0, "no point behind the camera"
    for name, m in (("left", u < -4), ("right", u >= 36), ("top", v < -4), ("bottom", v >= 28)):
        assert (front & m).sum() > 0, f"no point leaves the frame on the {name}"
    inside = front & (u >= -4) & (u < 36) & (v >= -4) & (v < 28)
    iu, iv = np.floor(u[inside]), np.floor(v[inside])
    # a 3 x 3 footprint (offset 1) clipped at each border
    assert (iu <= 0).any() and (iu >= 31).any() and (iv <= 0).any() and (iv >= 23).any()
    assert inside.sum() > 50


def test_contention_and_tie_inputs():
    z = C.splat_model("contention_4x4")
    k = C.splat_inputs("contention_4x4")
    assert (z != M.EMPTY).sum() == 16                # every pixel of the 4 x 4 image is fought over
    k = C.tie_inputs()
    f, cx, cy = C.pinhole(48, 64)
    z = M.splat(k["depth"], k["ray_tab"], k["image"], k["view"], f, cx, cy, 48, 64, 1, C.MIN_Z, C.MAX_DEPTH, C.NEAR)
    assert (z != M.EMPTY).sum() >= 4


@pytest.mark.parametrize("skel,zname,r", C.RESOLVE_CASES)
def test_resolve_inputs_are_unambiguous(skel, zname, r):
    out, amb = C.resolve_model(skel, zname, r)
    share = amb.mean()
    assert share <= C.AMBIGUOUS_CAP, f"ambiguous share {share:.4f}"


@pytest.mark.parametrize("skel,dname,r", C.OVERLAY_CASES)
def test_overlay_inputs_are_unambiguous(skel, dname, r):
    out, amb = C.overlay_model(skel, dname, r)
    assert amb.mean() <= C.AMBIGUOUS_CAP, f"ambiguous share {amb.mean():.4f}"


def test_model_inputs_show_what_they_are_meant_to():
    full, _ = C.resolve_model("golden", "empty", "big")
    bg = np.array([250, 240, 230], dtype=np.uint8)
    skel_px = (full != bg).any(axis=-1)
    assert 50 < skel_px.sum() < full[..., 0].size // 2          # a skeleton is visible
    nan, _ = C.resolve_model("nan_joint", "empty", "big")
    changed = (nan != full).any(axis=-1)
    assert 0 < changed.sum() < skel_px.sum() and not (changed & ~skel_px).any()     # something vanished, nothing appeared
    none, _ = C.resolve_model("no_hit", "wall", "big")
    assert not ((none != bg).all(axis=-1) & (C.wall_zbuf() == M.EMPTY)).any()      # empty pixels show the background
    wall, _ = C.resolve_model("golden", "wall", "big")
    hidden = ((wall != full).any(axis=-1) & skel_px)
    assert hidden.sum() > 0 and (wall == full).all(axis=-1)[skel_px].sum() > 0      # partly behind the wall
    over_free, _ = C.overlay_model("golden", "none", "big")
    over_wall, _ = C.overlay_model("golden", "wall", "big")
    frame_rgb = C.image(1)[:, :, :, ::-1]
    drawn = (over_free != frame_rgb).any(axis=-1)
    assert drawn.sum() > 5 and (over_wall != frame_rgb).any(axis=-1).sum() < drawn.sum()
    behind, _ = C.resolve_model("behind", "empty", "big")
    assert (behind != full).any()


def test_model_splat_min_is_order_free():
    """The model's own minimum does not depend on the order the points are visited in (np.minimum.at over keys)."""
    k = C.splat_inputs("b1_d32_o24_s2")
    f, cx, cy = C.pinhole(24, 32)
    a = C.splat_model("b1_d32_o24_s2")
    flip = dict(k, depth=k["depth"][:, ::-1].copy(), ray_tab=k["ray_tab"][::-1].copy(), image=k["image"][:, ::-1].copy())
    b = M.splat(flip["depth"], flip["ray_tab"], flip["image"], flip["view"], f, cx, cy, 24, 32, 2, C.MIN_Z, C.MAX_DEPTH, C.NEAR)
    assert np.array_equal(a, b)
