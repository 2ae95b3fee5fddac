"""GPU: csrc/render_volume.hip against tests/volume_render_model.py (numpy float64, the same operation order).

View and overlay equal the model on every pixel the model does not mark ambiguous (a decision of the slab test, of the cell walk, of
the range, the clamp at 1 or the final rounding within 1e-9 / 1e-6 of flipping); the ambiguous share is capped at 0.5 % here and, for
the same inputs, on the CPU in tests/test_volume_render_host.py, so the mask cannot hide a failure.  Then the identities the
definition promises, the error codes, and the feature end to end: SceneRenderer at full size on a synthetic-weights forward,
demo.py / run_sequence.py --render_volumes."""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

import render_cases as RC
import volume_render_cases as C
import volume_render_model as M
from conftest import CALIB, GOLD
from sceneego_amd import _lib, load_config, synth
from sceneego_amd.fisheye import FishEyeCameraCalibrated
from sceneego_amd.render import SceneRenderer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def packed(B, G):
    """The packed copy of the case volumes, in a buffer that starts as NaN: the pack pass has to write every slot."""
    buf = torch.full((_lib.render_volume_packed_elems(B, G),), float("nan"), device=DEV)
    _lib.render_volume_pack(dev(C.volumes(B, G)), buf)
    torch.cuda.synchronize()
    return buf


def gpu_view(rays, view, zbuf, base, B, G, mask=M.ALL, gain=1.0, near=C.NEAR, scale=None, pk=None):
    out = torch.zeros(base.shape, device=DEV, dtype=torch.uint8)
    _lib.render_volume_view(packed(B, G) if pk is None else pk, dev(C.scales(B, G) if scale is None else scale), dev(rays), view,
                            None if zbuf is None else dev(zbuf), out, G, C.S, base=dev(base), near=near, joint_mask=mask, gain=gain,
                            opacity=C.OPACITY)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def gpu_overlay(depth, base, B, G, mask=M.ALL, gain=1.0, scale=None, pk=None):
    out = torch.zeros(base.shape, device=DEV, dtype=torch.uint8)
    _lib.render_volume_overlay(packed(B, G) if pk is None else pk, dev(C.scales(B, G) if scale is None else scale), dev(RC.ray_table()),
                               out, G, C.S, base=dev(base), depth=None if depth is None else dev(depth), near=C.NEAR, joint_mask=mask,
                               gain=gain, opacity=C.OPACITY)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _compare(got, want, amb, tag):
    share = float(amb.mean())
    wrong = (got != want).any(axis=-1) & ~amb
    print(f"{tag}: ambiguous share {share:.5f}, {int(wrong.sum())} unambiguous pixels differ, "
          f"{int(((got != want).any(axis=-1) & amb).sum())} ambiguous ones")
    assert share <= C.AMBIGUOUS_CAP
    assert not wrong.any(), f"{tag}: {int(wrong.sum())} pixels differ, first at {np.argwhere(wrong)[0]}"


# ------------------------------------------------------------------------------------------------------------------ against the model
def test_pack_interleaves_the_cells():
    for B, G in ((1, 8), (3, 12)):
        got = packed(B, G).cpu().numpy().reshape(B, G ** 3, 16)
        want = np.zeros((B, G ** 3, 16), dtype=np.float32)
        want[:, :, :15] = C.volumes(B, G).reshape(B, 15, G ** 3).transpose(0, 2, 1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))          # bit for bit, the NaN cell included


@pytest.mark.parametrize("name", [c[0] for c in C.VIEW_CASES])
def test_view_equals_the_model(name):
    _, B, G, v, z, mask, gain = C.view_case(name)
    want, amb, _ = C.view_model(name)
    got = gpu_view(RC.pinhole_rays(C.HOUT, C.WOUT), C.VIEWS[v], C.zbuf(z, B), C.base_view(B), B, G, mask=mask, gain=gain)
    _compare(got, want, amb, f"view {name}")
    if name in ("g12_b3_side_ramp", "g64_orbit"):
        again = gpu_view(RC.pinhole_rays(C.HOUT, C.WOUT), C.VIEWS[v], C.zbuf(z, B), C.base_view(B), B, G, mask=mask, gain=gain)
        assert np.array_equal(again, got), "two launches differ"


@pytest.mark.parametrize("name", [c[0] for c in C.OVERLAY_CASES])
def test_overlay_equals_the_model(name):
    _, B, G, d, mask, gain = C.overlay_case(name)
    want, amb, _ = C.overlay_model(name)
    got = gpu_overlay(C.depth(d, B), C.base_frame(B), B, G, mask=mask, gain=gain)
    _compare(got, want, amb, f"overlay {name}")
    if name in ("g12_b3_map", "g64_map"):
        assert np.array_equal(gpu_overlay(C.depth(d, B), C.base_frame(B), B, G, mask=mask, gain=gain), got), "two launches differ"


@pytest.mark.parametrize("origin,G", C.HAND_CASES)
def test_hand_made_rays_with_zero_components(origin, G):
    want, amb, _ = C.hand_model(origin, G)
    got = gpu_view(C.hand_rays(), C.hand_view(origin), None, C.hand_base(), 1, G, near=0.0)
    assert not amb.any()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------ identities
def test_in_place_equals_a_separate_base():
    B, G = 3, 12
    base = C.base_view(B)
    want = gpu_view(RC.pinhole_rays(C.HOUT, C.WOUT), C.VIEWS["orbit"], C.zbuf("ramp", B), base, B, G)
    out = dev(base).clone()
    _lib.render_volume_view(packed(B, G), dev(C.scales(B, G)), dev(RC.pinhole_rays(C.HOUT, C.WOUT)), C.VIEWS["orbit"],
                            dev(C.zbuf("ramp", B)), out, G, C.S, near=C.NEAR, opacity=C.OPACITY)
    assert np.array_equal(out.cpu().numpy(), want) and (want != base).any()


def test_zero_volume_and_zero_mask_return_the_base_bytes():
    B, G = 1, 12
    rays = RC.pinhole_rays(C.HOUT, C.WOUT)
    zero = torch.zeros(_lib.render_volume_packed_elems(B, G), device=DEV)
    ones = np.ones((B, 15))
    for view in ("side", "orbit"):
        assert np.array_equal(gpu_view(rays, C.VIEWS[view], None, C.base_view(B), B, G, gain=1e6, scale=ones, pk=zero), C.base_view(B))
        assert np.array_equal(gpu_view(rays, C.VIEWS[view], None, C.base_view(B), B, G, mask=0, gain=4.0), C.base_view(B))
    assert np.array_equal(gpu_overlay(None, C.base_frame(B), B, G, gain=1e6, scale=ones, pk=zero), C.base_frame(B))
    assert np.array_equal(gpu_overlay(None, C.base_frame(B), B, G, mask=0, gain=4.0), C.base_frame(B))


def test_nan_cell_and_off_joints_change_nothing_beyond_their_definition():
    """The NaN cell counts as absent (never the maximum), a joint with scale 0 / a non-finite scale / a clear mask bit as not drawn."""
    B, G = 1, 12
    rays, view, base = RC.pinhole_rays(C.HOUT, C.WOUT), C.VIEWS["orbit"], C.base_view(B)
    ref = gpu_view(rays, view, None, base, B, G)
    # the NaN cell replaced by 0: the same picture (its neighbours, not it, were the maxima)
    vol = C.volumes(B, G).copy()
    assert np.isnan(vol).sum() == 1
    vol[np.isnan(vol)] = 0.0
    pk = torch.empty(_lib.render_volume_packed_elems(B, G), device=DEV)
    _lib.render_volume_pack(dev(vol), pk)
    assert np.array_equal(gpu_view(rays, view, None, base, B, G, pk=pk), ref)
    # joints 5 (infinite scale) and 7 (scale 0) are off already: clearing their mask bits, or a NaN / negative scale, changes nothing
    off = M.ALL & ~(1 << C.ZERO_JOINT) & ~(1 << C.OFF_JOINT)
    assert np.array_equal(gpu_view(rays, view, None, base, B, G, mask=off), ref)
    sc = C.scales(B, G).copy()
    sc[:, C.ZERO_JOINT], sc[:, C.OFF_JOINT] = np.nan, -3.0
    assert np.array_equal(gpu_view(rays, view, None, base, B, G, scale=sc), ref)
    # and switching one live joint off equals clearing its mask bit
    sc = C.scales(B, G).copy()
    sc[:, 9] = 0.0
    one_off = gpu_view(rays, view, None, base, B, G, scale=sc)
    assert np.array_equal(one_off, gpu_view(rays, view, None, base, B, G, mask=M.ALL & ~(1 << 9)))
    assert (one_off != ref).any()


def test_bad_arguments_return_the_error_code_without_a_launch():
    B, G = 1, 8
    lib, p = _lib.load(), _lib._ptr
    pk, sc, rays = packed(B, G), dev(C.scales(B, G)), dev(RC.pinhole_rays(C.HOUT, C.WOUT))
    tab, depth = dev(RC.ray_table()), dev(RC.wall_depth())
    SENT = 77
    out = torch.full((B, C.HOUT, C.WOUT, 3), SENT, device=DEV, dtype=torch.uint8)
    frame = torch.full((B, RC.H, RC.W, 3), SENT, device=DEV, dtype=torch.uint8)
    import ctypes
    view = (ctypes.c_double * 12)(*C.VIEWS["orbit"])
    bad_view = (ctypes.c_double * 12)(*([float("nan")] + list(C.VIEWS["orbit"][1:])))
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def view_call(pk_=p(pk), sc_=p(sc), rays_=p(rays), v=vp(view), out_=p(out), batch=B, h=C.HOUT, w=C.WOUT, grid=G, side=C.S, near=C.NEAR,
                  mask=M.ALL, gain=1.0, opacity=0.8):
        return lib.se_render_volume_view_f64(pk_, sc_, rays_, v, None, out_, out_, batch, h, w, grid, side, near, mask, gain, opacity, None)

    def overlay_call(pk_=p(pk), out_=p(frame), batch=B, h=RC.H, w=RC.W, dh=16, dw=20, grid=G, side=C.S, near=C.NEAR, mask=M.ALL, gain=1.0,
                     opacity=0.8):
        return lib.se_render_volume_overlay_f64(pk_, p(sc), p(tab), p(depth), out_, out_, batch, h, w, dh, dw, grid, side, near, mask, gain,
                                                opacity, None)

    bad = [dict(pk_=None), dict(sc_=None), dict(rays_=None), dict(v=None), dict(out_=None), dict(batch=0), dict(batch=65536), dict(h=0),
           dict(w=-1), dict(grid=1), dict(grid=1025), dict(side=0.0), dict(side=float("nan")), dict(near=-0.1), dict(near=float("nan")),
           dict(mask=1 << 15), dict(gain=-1.0), dict(gain=float("nan")), dict(gain=float("inf")), dict(opacity=1.5),
           dict(opacity=float("nan")), dict(v=vp(bad_view)), dict(pk_=ctypes.c_void_p(pk.data_ptr() + 4))]
    for kw in bad:
        assert view_call(**kw) == -1, kw
    for kw in (dict(pk_=None), dict(out_=None), dict(batch=0), dict(h=0), dict(dh=0), dict(dw=-3), dict(grid=1), dict(side=-2.0),
               dict(near=-1.0), dict(mask=0x8000), dict(gain=-0.5), dict(opacity=-0.1)):
        assert overlay_call(**kw) == -1, kw
    vol = dev(C.volumes(B, G))
    assert lib.se_render_volume_pack_f32(None, p(pk), pk.numel() * 4, B, G, None) == -1
    assert lib.se_render_volume_pack_f32(p(vol), None, pk.numel() * 4, B, G, None) == -1
    assert lib.se_render_volume_pack_f32(p(vol), p(pk), pk.numel() * 4 - 1, B, G, None) == -1
    assert lib.se_render_volume_pack_f32(p(vol), p(pk), pk.numel() * 4, B, 1, None) == -1
    assert lib.se_render_volume_pack_f32(p(vol), p(pk), pk.numel() * 4, 0, G, None) == -1
    assert lib.se_render_volume_packed_bytes(1, 1) == -1 and lib.se_render_volume_packed_bytes(0, 8) == -1
    torch.cuda.synchronize()
    assert (out == SENT).all() and (frame == SENT).all(), "a refused call launched something"
    assert view_call() == 0 and overlay_call() == 0                       # the same calls with good arguments do launch
    torch.cuda.synchronize()
    assert (out != SENT).any() and (frame != SENT).any()
    with pytest.raises(_lib.HipExtensionError):
        _lib.render_volume_view(pk, sc[:, :14].contiguous(), rays, C.VIEWS["orbit"], None, out, G, C.S)
    with pytest.raises(_lib.HipExtensionError):
        _lib.render_volume_pack(vol, pk[:-1])


# ------------------------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def full_size():
    """One synthetic-weights forward of the demo frame: frame, depth, joints, volumes, statistics, the network, a renderer."""
    from conftest import ROOT
    from sceneego_amd.preprocess import load_depth, load_image_bgr, preprocess_image_device
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    config = load_config(os.path.join(ROOT, "experiments", "sceneego", "test", "sceneego.yaml"))
    net = VoxelNetwork_depth(config, device="cpu")
    net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(DEV).eval()
    frame = load_image_bgr(os.path.join(GOLD, "demo", "img_001000.jpg"))
    depth = torch.from_numpy(load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr"))).to(DEV)[None]
    with torch.no_grad():
        img = preprocess_image_device(torch.from_numpy(frame).to(DEV)[None], config.image_shape)
        kp, _, vol, _ = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)
        stats = net.joint_statistics(vol, kp)
    torch.cuda.synchronize()
    return frame, depth, kp, vol, stats, net, SceneRenderer(CALIB, device=DEV)


def test_full_size_identities_and_the_box():
    frame, depth, kp, vol, _, net, r = full_size()
    side = net.cuboid_side
    base_r, base_o = r.render(depth, frame, kp).clone(), r.overlay(frame, kp, depth=depth).clone()
    zero = torch.zeros_like(vol)
    assert torch.equal(r.render_volumes(depth, frame, kp, zero, side), base_r)
    assert torch.equal(r.overlay_volumes(frame, kp, zero, side, depth=depth), base_o)
    assert torch.equal(r.render_volumes(depth, frame, kp, vol, side, joint_mask=[]), base_r)
    assert torch.equal(r.overlay_volumes(frame, kp, vol, side, depth=depth, joint_mask=()), base_o)
    got_r = r.render_volumes(depth, frame, kp, vol, side, gain=4.0).clone()
    got_o = r.overlay_volumes(frame, kp, vol, side, depth=depth, gain=4.0, occlude=False).clone()
    assert got_r.shape == (1, 720, 960, 3) and got_o.shape == (1, 1024, 1280, 3) and got_r.dtype == got_o.dtype == torch.uint8
    assert (got_r != base_r).any() and (got_o != base_o).any()
    assert torch.equal(r.render_volumes(depth, frame, kp, vol, side, gain=4.0), got_r), "two runs differ"
    assert torch.equal(r.overlay_volumes(frame, kp, vol, side, depth=depth, gain=4.0, occlude=False), got_o), "two runs differ"
    # the base picture is untouched outside the box's projection.  The fisheye camera sits inside the box (every overlay ray crosses
    # it), so this is a statement about the third-person view: a pixel whose ray misses the box grown by 1e-6 m (slab test in float64,
    # written out here) keeps its bytes
    from sceneego_amd.render import orbit_view
    G = vol.shape[2]
    h = side / (G - 1)
    lo, hi = np.array([-side / 2 - h / 2, -side / 2 - h / 2, -h / 2]) - 1e-6, np.array([side / 2 + h / 2, side / 2 + h / 2, side + h / 2]) + 1e-6
    o, d = M.view_rays(r.pinhole.cpu().numpy(), orbit_view())
    with np.errstate(all="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d                 # no direction of this table has a zero component
        s0 = np.fmin(ta, tb).max(axis=-1)
        s1 = np.fmax(ta, tb).min(axis=-1)
    assert (d != 0).all()
    outside = ~(np.maximum(s0, 0.0) < s1)
    changed = (got_r != base_r).any(dim=-1)[0].cpu().numpy()
    print(f"view: {int(changed.sum())} pixels changed, {int(outside.sum())} of {outside.size} pixels look past the box")
    assert outside.sum() > 1000 and changed.sum() > 1000 and not (changed & outside).any()


def test_full_size_brightest_pixel_lies_on_the_peak():
    """Single-joint mask on a black frame without a skeleton (NaN joints draw nothing): the brightest overlay pixel lies within 2 pixels
    of the fisheye projection of that joint's peak_coord, because the peak cell is on that pixel's ray.  An 8-bit picture has ties:
    every pixel whose ray crosses the peak cell carries the same value, so the statement is about the set of brightest pixels, whose
    size is printed.  Joints whose peak projects outside the frame are not visible and are skipped (printed, too)."""
    frame, depth, kp, vol, stats, net, r = full_size()
    cam = FishEyeCameraCalibrated(CALIB)
    black = np.zeros_like(frame)
    nowhere = torch.full((1, 15, 3), float("nan"))
    peaks = stats["peak_coord"][0].double().cpu().numpy()
    # a little below 1 / max: the peak maps to 0.999, so the clamp at 1 stays off
    sc = 0.999 / vol.amax(dim=(2, 3, 4)).double()
    tested = 0
    for j in range(15):
        u, v = cam.world2camera(peaks[j][None])[0]
        if not (3 <= u < frame.shape[1] - 3 and 3 <= v < frame.shape[0] - 3):
            print(f"joint {j}: peak {peaks[j]} projects to ({u:.1f}, {v:.1f}), outside the frame: skipped")
            continue
        over = r.overlay_volumes(black, nowhere, vol, net.cuboid_side, joint_mask=[j], scale=sc, opacity=1.0)[0].cpu().numpy()
        col = np.array(_lib.render_volume_palette()[j], dtype=np.int64)
        k = int(col.argmax())                                # on black c = a * col: the colour's largest channel measures a
        bright = over[:, :, k].astype(np.int64)
        ys, xs = np.nonzero(bright == bright.max())
        dist = np.hypot(xs + 0.5 - u, ys + 0.5 - v)
        print(f"joint {j}: {len(xs)} brightest pixels (value {bright.max()} of {col[k]}), peak projects to ({u:.2f}, {v:.2f}), "
              f"nearest brightest pixel {dist.min():.2f} px away")
        assert bright.max() == int(np.floor(0.999 * col[k] + 0.5))
        assert dist.min() <= 2.0
        tested += 1
    assert tested >= 1


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def test_demo_render_volumes(tmp_path, capsys):
    import demo
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg"), img_dir / "a_001000.jpg")
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), depth_dir / "a_001000.jpg.exr")
    common = ["--img_dir", str(img_dir), "--depth_dir", str(depth_dir), "--weights", "synthetic"]
    demo.main(common + ["--output_dir", str(tmp_path / "plain"), "--render_dir", str(tmp_path / "png0")])
    demo.main(common + ["--output_dir", str(tmp_path / "drawn"), "--render_dir", str(tmp_path / "png"), "--render_volumes", "true",
                        "--volume_joints", "9,10,13,14", "--save_volumes", "true"])
    capsys.readouterr()
    names = ["a_001000.jpg" + e for e in (".overlay.png", ".render.png", ".volumes.overlay.png", ".volumes.render.png")]
    assert sorted(os.listdir(tmp_path / "png")) == names
    for n in names[:2]:                                                     # the existing pair is byte-identical
        assert (tmp_path / "png" / n).read_bytes() == (tmp_path / "png0" / n).read_bytes()
    assert (tmp_path / "plain" / "a_001000.jpg.pkl").read_bytes() == (tmp_path / "drawn" / "a_001000.jpg.pkl").read_bytes()
    assert sorted(os.listdir(tmp_path / "drawn")) == ["a_001000.jpg.pkl", "a_001000.jpg.volumes.npy"]
    # the files decode to the renderer's arrays: the saved volumes through the same methods give the same pictures
    vol = np.load(tmp_path / "drawn" / "a_001000.jpg.volumes.npy")
    assert vol.shape == (15, 64, 64, 64) and vol.dtype == np.float32
    import pickle
    with open(tmp_path / "drawn" / "a_001000.jpg.pkl", "rb") as f:
        kp = pickle.load(f)
    frame, depth, _, _, _, net, r = full_size()
    want_r = r.render_volumes(depth, frame, kp, torch.from_numpy(vol), net.cuboid_side, joint_mask=(9, 10, 13, 14))[0].cpu().numpy()
    assert np.array_equal(_decode(tmp_path / "png" / names[3]), want_r)
    want_o = r.overlay_volumes(frame, kp, torch.from_numpy(vol), net.cuboid_side, depth=depth, joint_mask=(9, 10, 13, 14))[0].cpu().numpy()
    assert np.array_equal(_decode(tmp_path / "png" / names[2]), want_o)
    assert (want_o != _decode(tmp_path / "png" / names[0])).any()


def test_run_sequence_render_volumes(tmp_path, capsys):
    """One run writes the four pictures of every frame and the video; a second, independent pass over the same sequence (the runner's
    own loaders and forward, no rendering; the forward's outputs taken by a hook) supplies frames, depth, joints and volumes, from
    which every file is recomputed: stale or zero volumes, a wrong mask or a picture overwritten in the shared buffers would show."""
    import pickle

    import jpeg_encode_cases as JC
    import run_sequence
    from sceneego_amd.jpeg_device import JpegFile
    depths = [os.path.join(GOLD, "demo", n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr")]
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 2, depths, estimated_depth_name="est_depth", seed=5)
    common = ["--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
    which = (3, 9, 14)
    drawn = run_sequence.main(common + ["--output", str(tmp_path / "drawn.pkl"), "--render_dir", str(tmp_path / "png"),
                                        "--render_volumes", "true", "--volume_joints", "3,9,14", "--render_video", str(tmp_path / "v.avi"),
                                        "--render_quality", "90"])
    capsys.readouterr()
    images, _, depth_paths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    stems = [os.path.split(p)[1] for p in images]
    want = sorted(s + e for s in stems for e in (".render.png", ".overlay.png", ".volumes.render.png", ".volumes.overlay.png"))
    assert sorted(os.listdir(tmp_path / "png")) == want and len(stems) == 2

    from conftest import ROOT
    config = load_config(os.path.join(ROOT, "experiments", "sceneego", "test", "sceneego.yaml"))
    runner = run_sequence.SequenceRunner(config, weights="synthetic")
    seen = []
    hook = runner.net.register_forward_hook(
        lambda mod, args, kwargs, out: seen.append((out[0].clone(), out[2].clone(), kwargs["depth_map_batch"].clone())), with_kwargs=True)
    preds = runner.run(images, depth_paths, config.test.batch_size)
    hook.remove()
    kp = torch.cat([s[0] for s in seen])
    vol = torch.cat([s[1] for s in seen])
    depth = torch.cat([s[2] for s in seen])
    assert len(kp) == 2 and np.array_equal(np.stack(preds), kp.cpu().numpy())
    with open(tmp_path / "drawn.pkl", "rb") as f:
        assert np.array_equal(np.stack(pickle.load(f)), np.stack(preds))
    assert len(drawn["predictions"]) == 2
    frames = runner._frames_u8([JpegFile(p) for p in images])
    r = SceneRenderer(CALIB, frame_size=tuple(frames.shape[1:3]), device=DEV)
    side = runner.net.cuboid_side
    plain_r, plain_o = r.render(depth, frames, kp).cpu().numpy(), r.overlay(frames, kp, depth=depth).cpu().numpy()
    vol_r = r.render_volumes(depth, frames, kp, vol, side, joint_mask=which).clone()
    vol_o = r.overlay_volumes(frames, kp, vol, side, depth=depth, joint_mask=which).cpu().numpy()
    all_r = r.render_volumes(depth, frames, kp, vol, side).cpu().numpy()
    for k, s in enumerate(stems):
        assert np.array_equal(_decode(tmp_path / "png" / (s + ".render.png")), plain_r[k])
        assert np.array_equal(_decode(tmp_path / "png" / (s + ".overlay.png")), plain_o[k])
        assert np.array_equal(_decode(tmp_path / "png" / (s + ".volumes.render.png")), vol_r[k].cpu().numpy())
        assert np.array_equal(_decode(tmp_path / "png" / (s + ".volumes.overlay.png")), vol_o[k])
        # the comparisons above distinguish what they should: the volumes are visible, and the mask matters
        assert (vol_r[k].cpu().numpy() != plain_r[k]).any() and (vol_o[k] != plain_o[k]).any() and (all_r[k] != vol_r[k].cpu().numpy()).any()
    # the video shows the volume view: its frames are the encoder's bytes of those pictures (the encoder is bitwise reproducible)
    payloads = JC.check_avi((tmp_path / "v.avi").read_bytes(), 2, 960, 720, 25)
    assert payloads == [bytes(b) for b in runner._encoder().encode(vol_r, quality=90, subsampling="420")]
    assert payloads != [bytes(b) for b in runner._encoder().encode(torch.from_numpy(plain_r).to(DEV), quality=90, subsampling="420")]


def test_default_scale_passes_over_a_nan_cell():
    """Through the public method a NaN voxel never wins and does not switch its joint off: the default scale is taken over the finite
    values, so the picture equals the one of the same volumes with that cell set to 0."""
    frame, depth, kp, vol, _, net, r = full_size()
    j = 9
    flat = int(vol[0, j].argmin())                       # any cell that is not the joint's maximum
    holed, zeroed = vol.clone(), vol.clone()
    holed[0, j].view(-1)[flat] = float("nan")
    zeroed[0, j].view(-1)[flat] = 0.0
    want = r.overlay_volumes(frame, kp, zeroed, net.cuboid_side, joint_mask=[j]).clone()
    got = r.overlay_volumes(frame, kp, holed, net.cuboid_side, joint_mask=[j]).clone()
    assert torch.equal(got, want)
    assert (got != r.overlay(frame, kp)).any()            # the joint is drawn
