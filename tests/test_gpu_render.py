"""GPU: csrc/render.hip against tests/render_model.py (numpy float64, the same operation order).

Splat: the uint64 z-buffer equals the model's bit for bit (only products, sums, quotients and floor: every one correctly rounded on
both sides, and the 64-bit minimum does not depend on the order).  Resolve / overlay: the image equals the model's on every pixel
the model does not mark ambiguous (a square root or a decision within 1e-9 / 1e-6 of flipping); the ambiguous share is capped at
0.5 % here and, for the same inputs, on the CPU in tests/test_render_host.py, so the mask cannot hide a failure.  Then the feature
end to end: SceneRenderer at full size on the demo frame, scene_points against the camera model, demo.py / run_sequence.py
--render_dir."""
import functools
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import render_cases as C
import render_model as M
from conftest import CALIB, GOLD
from sceneego_amd import _lib, synth
from sceneego_amd.fisheye import FishEyeCameraCalibrated
from sceneego_amd.render import SceneRenderer, orbit_view

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = (250, 240, 230)


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_splat(k):
    f, cx, cy = C.pinhole(k["Hout"], k["Wout"])
    B = k["depth"].shape[0]
    zbuf = torch.zeros((B, k["Hout"], k["Wout"]), device=DEV, dtype=torch.int64)        # zeros: the entry point must clear it
    _lib.render_splat(dev(k["depth"]), dev(k["ray_tab"]), dev(k["image"]), dev(np.asarray(k["view"], dtype=np.float64)), zbuf, f, cx, cy,
                      splat=k["splat"], min_z=C.MIN_Z, max_depth=C.MAX_DEPTH, near=C.NEAR)
    torch.cuda.synchronize()
    return zbuf.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ splat
@pytest.mark.parametrize("name", [c[0] for c in C.SPLAT_CASES])
def test_splat_equals_the_model_bit_for_bit(name):
    got = gpu_splat(C.splat_inputs(name))
    want = C.splat_model(name)
    print(f"{name}: {(want != M.EMPTY).sum()} of {want.size} pixels covered, {(got != want).sum()} differ")
    assert np.array_equal(got, want)
    assert np.array_equal(gpu_splat(C.splat_inputs(name)), got), "two launches differ"


def test_splat_forced_tie_takes_the_lowest_colour_word():
    k = C.tie_inputs()
    got = gpu_splat(k)
    f, cx, cy = C.pinhole(48, 64)
    want = M.splat(k["depth"], k["ray_tab"], k["image"], k["view"], f, cx, cy, 48, 64, 1, C.MIN_Z, C.MAX_DEPTH, C.NEAR)
    assert np.array_equal(got, want)
    # stated without the model: a key that survives carries the lowest colour word of its 4 x 4 block of equal rays and depths
    img = k["image"][0].astype(np.uint32)
    word = (img[:, :, 2] << 16) | (img[:, :, 1] << 8) | img[:, :, 0]
    block_min = set(int(word[4 * r:4 * r + 4, 4 * c:4 * c + 4].min()) for r in range(8) for c in range(10))
    kept = got[got != M.EMPTY]
    assert len(kept) >= 4 and all(int(v & np.uint64(0xFFFFFFFF)) in block_min for v in kept)


def test_bad_arguments():
    k = C.splat_inputs("b1_d32_o24_s1")
    f, cx, cy = C.pinhole(24, 32)
    depth, rays, img, view = dev(k["depth"]), dev(k["ray_tab"]), dev(k["image"]), dev(np.asarray(k["view"]))
    SENT = 1234567
    zbuf = torch.full((1, 24, 32), SENT, device=DEV, dtype=torch.int64)
    for s in (0, 5):
        with pytest.raises(_lib.HipExtensionError):
            _lib.render_splat(depth, rays, img, view, zbuf, f, cx, cy, splat=s)
    lib, p = _lib.load(), _lib._ptr
    args = (1, 32, 40, 32, 40, 24, 32, f, cx, cy)
    assert lib.se_render_splat_f64(p(depth), p(rays), p(img), p(view), None, *args, 2, 0.1, 100.0, 0.05, None) == -1
    assert lib.se_render_splat_f64(p(depth), p(rays), p(img), p(view), p(zbuf), *args, 0, 0.1, 100.0, 0.05, None) == -1
    assert lib.se_render_splat_f64(p(depth), p(rays), p(img), p(view), p(zbuf), *args, 5, 0.1, 100.0, 0.05, None) == -1
    assert lib.se_render_splat_f64(p(depth), p(rays), p(img), p(view), p(zbuf), 65536, *args[1:], 2, 0.1, 100.0, 0.05, None) == -1
    assert lib.se_render_splat_f64(p(depth), p(rays), p(img), p(view), p(zbuf), 1, 32, 40, 32, 0, 24, 32, f, cx, cy, 2, 0.1, 100.0, 0.05,
                                   None) == -1
    torch.cuda.synchronize()
    assert (zbuf == SENT).all(), "a refused call launched something"
    with pytest.raises(_lib.HipExtensionError):
        _lib.render_resolve(dev(C.pinhole_rays(24, 32)), torch.zeros((1, 14, 3), device=DEV, dtype=torch.float64), zbuf,
                            torch.zeros((1, 24, 32, 3), device=DEV, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ resolve, overlay
def _compare(got, want, amb, tag):
    share = float(amb.mean())
    wrong = (got != want).any(axis=-1) & ~amb
    print(f"{tag}: ambiguous share {share:.5f}, {int(wrong.sum())} unambiguous pixels differ, "
          f"{int(((got != want).any(axis=-1) & amb).sum())} ambiguous ones")
    assert share <= C.AMBIGUOUS_CAP
    assert not wrong.any(), f"{tag}: {int(wrong.sum())} pixels differ, first at {np.argwhere(wrong)[0]}"


@functools.lru_cache(maxsize=None)
def gpu_resolve(skel, zname, r):
    z = C.zbufs()[zname]
    out = torch.zeros(z.shape + (3,), device=DEV, dtype=torch.uint8)
    _lib.render_resolve(dev(C.pinhole_rays(48, 64)), dev(C.skeletons()[skel][None]), dev(z), out, near=C.NEAR, background=BG, **C.radii(r))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("skel,zname,r", C.RESOLVE_CASES)
def test_resolve_equals_the_model(skel, zname, r):
    want, amb = C.resolve_model(skel, zname, r)
    _compare(gpu_resolve(skel, zname, r), want, amb, f"resolve {skel} {zname} {r}")


@pytest.mark.parametrize("zname", ["empty", "splat", "wall"])
def test_resolve_without_a_hit_returns_the_scene_untouched(zname):
    z = C.zbufs()[zname][0]
    got = gpu_resolve("no_hit", zname, "big")[0]
    empty = z == M.EMPTY
    assert (got[empty] == np.array(BG, dtype=np.uint8)).all()
    w = z[~empty]
    scene = np.stack([(w >> np.uint64(16)) & np.uint64(255), (w >> np.uint64(8)) & np.uint64(255), w & np.uint64(255)], axis=-1)
    assert np.array_equal(got[~empty], scene.astype(np.uint8))


def test_nan_joint_removes_its_primitives_only():
    full, nan = gpu_resolve("golden", "empty", "big")[0], gpu_resolve("nan_joint", "empty", "big")[0]
    bg = np.array(BG, dtype=np.uint8)
    changed = (full != nan).any(axis=-1)
    assert changed.any() and not (changed & (full == bg).all(axis=-1)).any()       # only pixels the full skeleton covered changed


@pytest.mark.parametrize("skel,dname,r", C.OVERLAY_CASES)
def test_overlay_equals_the_model(skel, dname, r):
    want, amb = C.overlay_model(skel, dname, r)
    frame = dev(C.image(1))
    out = torch.zeros_like(frame)
    depth = dev(C.wall_depth()) if dname == "wall" else None
    _lib.render_overlay(dev(C.ray_table()), dev(C.skeletons()[skel][None]), frame, out, depth=depth, near=C.NEAR, **C.radii(r))
    torch.cuda.synchronize()
    _compare(out.cpu().numpy(), want, amb, f"overlay {skel} {dname} {r}")


# ------------------------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def demo_frame():
    from sceneego_amd.preprocess import load_depth, load_image_bgr
    frame = load_image_bgr(os.path.join(GOLD, "demo", "img_001000.jpg"))
    depth = load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr"))
    return frame, depth, SceneRenderer(CALIB, device=DEV)


def test_scene_renderer_full_size():
    frame, depth, r = demo_frame()
    joints = C.golden_joints().astype(np.float32)
    out = r.render(depth, frame, joints).cpu().numpy()
    assert out.shape == (1, 720, 960, 3) and out.dtype == np.uint8
    img = out[0].astype(np.int32)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 100                         # not constant: a scene is there
    blue = (img[:, :, 2] > img[:, :, 0] + 60) & (img[:, :, 2] > img[:, :, 1] + 60) & (np.abs(img[:, :, 0] - img[:, :, 1]) <= 1)
    green = (img[:, :, 1] > img[:, :, 0] + 60) & (img[:, :, 1] > img[:, :, 2] + 60) & (np.abs(img[:, :, 0] - img[:, :, 2]) <= 1)
    print(f"render: {int(blue.sum())} joint-coloured and {int(green.sum())} bone-coloured pixels")
    assert blue.sum() >= 15 and green.sum() >= 15                                   # both skeleton hues
    again = r.render(depth, frame, joints, view=orbit_view()).cpu().numpy()
    assert np.array_equal(again, out)

    over = r.overlay(frame, joints).cpu().numpy()[0]
    rgb = frame[:, :, ::-1]
    changed = (over != rgb).any(axis=-1)
    cam = FishEyeCameraCalibrated(CALIB)
    # the joints dilated by the joint radius (26 directions) and projected by world2camera, plus one pixel for the pixel grid
    dirs = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)], dtype=np.float64)
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    uv = cam.world2camera((joints.astype(np.float64)[:, None, :] + _lib.RENDER_R_JOINT * dirs[None]).reshape(-1, 3))
    x0, x1 = int(np.floor(uv[:, 0].min())) - 1, int(np.ceil(uv[:, 0].max())) + 1
    y0, y1 = int(np.floor(uv[:, 1].min())) - 1, int(np.ceil(uv[:, 1].max())) + 1
    ys, xs = np.nonzero(changed)
    print(f"overlay: {int(changed.sum())} pixels drawn, box x {xs.min()}..{xs.max()} y {ys.min()}..{ys.max()}, allowed x {x0}..{x1} y {y0}..{y1}")
    assert changed.sum() > 200
    assert xs.min() >= x0 and xs.max() <= x1 and ys.min() >= y0 and ys.max() <= y1
    hidden = r.overlay(frame, joints, depth=depth).cpu().numpy()[0]
    assert not ((hidden != rgb).any(axis=-1) & ~changed).any()                      # occlusion only removes skeleton pixels


def test_scene_points_agree_with_the_camera_model():
    frame, depth, r = demo_frame()
    pts, rgb = r.scene_points(depth, frame)
    pts, rgb = pts.cpu().numpy(), rgb.cpu().numpy()
    H, W = frame.shape[:2]
    dh, dw = depth.shape
    d = depth[(np.arange(H) * dh) // H][:, (np.arange(W) * dw) // W].copy()
    d[d > 100] = 0                                                                  # get_point_cloud_single_image
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    p = FishEyeCameraCalibrated(CALIB).camera2world(np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1), d.reshape(-1))
    keep = p[:, 2] > 0.1                                                            # postprocess
    assert keep.sum() == len(pts) and len(pts) > 100000
    err = np.abs(p[keep] - pts.astype(np.float64)).max()
    print(f"scene_points: {len(pts)} points, max |difference to camera2world| = {err:.3e} m")
    assert err <= 1e-6
    assert np.array_equal(rgb, frame.reshape(-1, 3)[keep][:, ::-1])


def _png_size(path):
    from PIL import Image
    with Image.open(path) as im:
        im.load()
        return im.size, im.mode


def test_demo_render_dir(tmp_path, capsys):
    import demo
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    for name in ("a_001000.jpg", "b_001000.jpg"):
        shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg"), img_dir / name)
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), depth_dir / "a_001000.jpg.exr")
    shutil.copy(os.path.join(GOLD, "demo", "img_001796.jpg.exr"), depth_dir / "b_001000.jpg.exr")
    common = ["--img_dir", str(img_dir), "--depth_dir", str(depth_dir), "--weights", "synthetic"]
    demo.main(common + ["--output_dir", str(tmp_path / "plain")])
    demo.main(common + ["--output_dir", str(tmp_path / "drawn"), "--render_dir", str(tmp_path / "png")])
    capsys.readouterr()
    assert sorted(os.listdir(tmp_path / "png")) == ["a_001000.jpg.overlay.png", "a_001000.jpg.render.png", "b_001000.jpg.overlay.png",
                                                    "b_001000.jpg.render.png"]
    for name in ("a_001000.jpg", "b_001000.jpg"):
        assert _png_size(tmp_path / "png" / (name + ".render.png")) == ((960, 720), "RGB")
        assert _png_size(tmp_path / "png" / (name + ".overlay.png")) == ((1280, 1024), "RGB")
        assert (tmp_path / "plain" / (name + ".pkl")).read_bytes() == (tmp_path / "drawn" / (name + ".pkl")).read_bytes()
    assert sorted(os.listdir(tmp_path / "drawn")) == sorted(os.listdir(tmp_path / "plain"))


def test_run_sequence_render_dir(tmp_path, capsys):
    import run_sequence
    depths = [os.path.join(GOLD, "demo", n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 2, depths, estimated_depth_name="est_depth", seed=5)
    common = ["--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
    plain = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl")])
    drawn = run_sequence.main(common + ["--output", str(tmp_path / "drawn.pkl"), "--render_dir", str(tmp_path / "png"), "--render_every", "2"])
    capsys.readouterr()
    assert (tmp_path / "plain.pkl").read_bytes() == (tmp_path / "drawn.pkl").read_bytes()
    images, _, _ = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    assert len(images) == 2 == len(drawn["predictions"]) == len(plain["predictions"])
    want = sorted(os.path.split(images[k])[1] + ext for k in (0,) for ext in (".render.png", ".overlay.png"))
    assert sorted(os.listdir(tmp_path / "png")) == want
    for name in want:
        size = (960, 720) if name.endswith(".render.png") else tuple(reversed(_frame_hw(images[0])))
        assert _png_size(tmp_path / "png" / name) == (size, "RGB")
    with open(tmp_path / "drawn.pkl", "rb") as f:
        assert len(pickle.load(f)) == 2


def _frame_hw(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]
