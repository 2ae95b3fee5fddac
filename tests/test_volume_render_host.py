"""CPU: the float64 model of the volume renderer (tests/volume_render_model.py) on the cases of tests/volume_render_cases.py: its
ambiguous share stays within the cap on every case (so the mask cannot hide a failure on the device), its cell walk agrees with an
independent brute-force formulation, and the zero-volume identity holds.  Then what runs without a device: the argument validation
of SceneRenderer.render_volumes / overlay_volumes and the parsing of the new command-line flags."""
import numpy as np
import pytest
import torch

import render_cases as RC
import volume_render_cases as C
import volume_render_model as M
from sceneego_amd import _lib
from sceneego_amd.render import SceneRenderer


@pytest.mark.parametrize("name", [c[0] for c in C.VIEW_CASES])
def test_view_ambiguous_share_is_within_the_cap(name):
    out, amb, _ = C.view_model(name)
    print(f"{name}: ambiguous share {amb.mean():.5f}, {(out != C.base_view(out.shape[0])).any(axis=-1).mean():.3f} of the pixels drawn")
    assert amb.mean() <= C.AMBIGUOUS_CAP


@pytest.mark.parametrize("name", [c[0] for c in C.OVERLAY_CASES])
def test_overlay_ambiguous_share_is_within_the_cap(name):
    out, amb, _ = C.overlay_model(name)
    print(f"{name}: ambiguous share {amb.mean():.5f}, {(out != C.base_frame(out.shape[0])).any(axis=-1).mean():.3f} of the pixels drawn")
    assert amb.mean() <= C.AMBIGUOUS_CAP


@pytest.mark.parametrize("origin,G", C.HAND_CASES)
def test_hand_made_rays_are_off_every_boundary(origin, G):
    out, amb, mx = C.hand_model(origin, G)
    assert not amb.any()
    hit = (mx > 0).any(axis=-1)[0].reshape(-1)
    if origin == "inside":
        assert hit.all()
    else:
        # x = -1.7 is outside the box: only directions with a positive x component can reach it; (1, 0, 0) does, and the rays along
        # y and z, which never step on x, miss without a division by their zero components
        assert not hit[C.HAND_DIRS[:, 0] <= 0].any() and hit[1] and hit[[0, 2, 3, 5]].sum() == 0
        assert np.array_equal(out[0].reshape(-1, 3)[~hit], C.hand_base()[0].reshape(-1, 3)[~hit])


def _brute(o, d, limit, B, G, mx, amb, tag):
    """The model's maxima equal the brute force's wherever unambiguous.  The brute force has near-ties of its own (a ray grazing a
    cell's edge; a cell the range just reaches): each is a near-tie of the walk as well (two `next` values, a start index, an entry
    parameter against the limit), so they must lie inside the model's ambiguous mask but for a handful of pixels, and everything
    excluded together stays within the cap: the second mask cannot hide a disagreement."""
    vol, sc = C.volumes(B, G), C.scales(B, G)
    for b in range(B):
        live = M.live_mask(sc[b], M.ALL)
        want, graze = M.brute_maxima(o, d, vol[b], sc[b], G, C.S, C.NEAR if tag != "hand" else 0.0, limit[b], live)
        ok = ~(amb[b] | graze)
        print(f"{tag} b{b}: {int(amb[b].sum())} ambiguous, {int((graze & ~amb[b]).sum())} grazing only, of {ok.size} pixels; "
              f"{int((mx[b][ok] != want[ok]).sum())} maxima differ")
        assert (graze & ~amb[b]).sum() <= max(1, 0.001 * ok.size)
        assert (~ok).mean() <= C.AMBIGUOUS_CAP
        assert np.array_equal(mx[b][ok], want[ok])
        assert (want[ok] > 0).any()


@pytest.mark.parametrize("name", [c[0] for c in C.VIEW_CASES if c[2] == 8])
def test_view_maxima_equal_the_brute_force(name):
    _, B, G, v, z, _, _ = C.view_case(name)
    _, amb, mx = C.view_model(name)
    o, d = M.view_rays(RC.pinhole_rays(C.HOUT, C.WOUT), C.VIEWS[v])
    zb = C.zbuf(z, B)
    zs = (zb >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    _brute(o, d, np.where(zb == M.EMPTY, np.inf, zs), B, G, mx, amb, name)


@pytest.mark.parametrize("name", [c[0] for c in C.OVERLAY_CASES if c[2] == 8])
def test_overlay_maxima_equal_the_brute_force(name):
    _, B, G, dn, _, _ = C.overlay_case(name)
    _, amb, mx = C.overlay_model(name)
    dep = C.depth(dn, B)
    dh, dw = dep.shape[1:]
    limit = dep[:, (np.arange(RC.H) * dh) // RC.H][:, :, (np.arange(RC.W) * dw) // RC.W].astype(np.float64)
    _brute(np.zeros(3), RC.ray_table(), limit, B, G, mx, amb, name)


@pytest.mark.parametrize("origin", ["inside", "outside"])
def test_hand_made_maxima_equal_the_brute_force(origin):
    _, amb, mx = C.hand_model(origin, 8)
    o, d = M.view_rays(C.hand_rays(), C.hand_view(origin))
    _brute(o, d, np.full((1, 4, 4), np.inf), 1, 8, mx, amb, "hand")


def test_zero_volume_and_zero_mask_leave_the_base_picture():
    rays, base = RC.pinhole_rays(C.HOUT, C.WOUT), C.base_view(1)
    zero = np.zeros((1, 15, 8, 8, 8), dtype=np.float32)
    ones = np.ones((1, 15))
    out, amb, _ = M.view(rays, C.VIEWS["orbit"], None, base, zero, ones, C.S, C.NEAR, gain=50.0)
    assert np.array_equal(out, base) and not amb.any()
    out, amb, _ = M.view(rays, C.VIEWS["orbit"], None, base, C.volumes(1, 8), C.scales(1, 8), C.S, C.NEAR, joint_mask=0)
    assert np.array_equal(out, base) and not amb.any()
    out, _, _ = M.overlay(RC.ray_table(), None, C.base_frame(1), zero, ones, C.S, C.NEAR)
    assert np.array_equal(out, C.base_frame(1))
    # and a volume that is not zero draws something: the identity above is not vacuous
    out, _, _ = M.view(rays, C.VIEWS["orbit"], None, base, C.volumes(1, 8), C.scales(1, 8), C.S, C.NEAR)
    assert (out != base).any()


def test_palette_separates_the_body_sides():
    pal = np.array(_lib.render_volume_palette())
    assert pal.shape == (15, 3) and len({tuple(c) for c in pal}) == 15
    neck, right, left = pal[0], pal[[1, 2, 3, 7, 8, 9, 10]], pal[[4, 5, 6, 11, 12, 13, 14]]
    assert neck.max() - neck.min() <= 10                                   # neutral
    assert (right[:, 0] > right[:, 2]).all() and (left[:, 2] + left[:, 1] > 2 * left[:, 0]).all()      # warm / cold


# ------------------------------------------------------------------------------------------------ argument validation, no device
def _host_renderer():
    """A SceneRenderer without its device state: every check of the two new methods runs before anything is launched."""
    r = SceneRenderer.__new__(SceneRenderer)
    r.device = torch.device("cpu")
    r.H, r.W, r.Hout, r.Wout = 32, 40, 48, 64
    r.f, r.cx, r.cy, r.splat, r.background = 50.0, 32.0, 24.0, 2, (255, 255, 255)
    r.ray_tab = torch.zeros((32, 40, 3), dtype=torch.float64)            # host tensors: a launch would refuse them
    r.pinhole = torch.zeros((48, 64, 3), dtype=torch.float64)
    r._buf = {}
    return r


def _good():
    return dict(frame=np.zeros((1, 32, 40, 3), dtype=np.uint8), joints=np.zeros((1, 15, 3), dtype=np.float32),
                depth=np.ones((1, 16, 20), dtype=np.float32), vol=torch.zeros((1, 15, 8, 8, 8)))


@pytest.mark.parametrize("method", ["render_volumes", "overlay_volumes"])
def test_bad_arguments_are_refused_before_any_launch(method):
    r, g = _host_renderer(), _good()

    def call(vol=g["vol"], side=2.0, frame=g["frame"], **kw):
        if method == "render_volumes":
            return r.render_volumes(g["depth"], frame, g["joints"], vol, side, **kw)
        return r.overlay_volumes(frame, g["joints"], vol, side, depth=g["depth"], **kw)

    for vol in (torch.zeros((1, 15, 8, 8, 8), dtype=torch.float64), torch.zeros((1, 14, 8, 8, 8)), torch.zeros((1, 15, 8, 8, 4)),
                torch.zeros((2, 15, 8, 8, 8)), torch.zeros((15, 8, 8)), torch.zeros((1, 15, 1, 1, 1))):
        with pytest.raises(ValueError, match="volumes must be|volumes need"):
            call(vol=vol)
    with pytest.raises(ValueError, match="frames must be uint8"):
        call(frame=np.zeros((1, 32, 40, 3), dtype=np.float32))
    for side in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cuboid_side"):
            call(side=side)
    for mask in ([15], [-1], [0.5], 3, "9"):
        with pytest.raises(ValueError, match="joint_mask"):
            call(joint_mask=mask)
    for scale in (np.ones((1, 14)), np.ones((2, 15)), np.ones((1, 15, 1))):
        with pytest.raises(ValueError, match="scale must be"):
            call(scale=scale)
    for gain in (-1.0, float("nan"), float("inf"), 1e31):
        with pytest.raises(ValueError, match="gain"):
            call(gain=gain)
    for opacity in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="opacity"):
            call(opacity=opacity)
    # good arguments get as far as the kernels, which refuse host tensors loudly: no CPU fallback
    with pytest.raises(_lib.HipExtensionError):
        call(joint_mask=[9, 10], scale=np.ones((1, 15)))


def test_joint_mask_bits():
    assert SceneRenderer._joint_mask(None) == 0x7FFF and SceneRenderer._joint_mask([]) == 0
    assert SceneRenderer._joint_mask((9, 10, 13, 14)) == (1 << 9) | (1 << 10) | (1 << 13) | (1 << 14)
    assert SceneRenderer._joint_mask(np.array([0, 0, 3])) == 0b1001


def test_library_helpers_without_a_device():
    assert _lib.render_volume_packed_elems(1, 64) == 64 ** 3 * 16 and _lib.render_volume_packed_elems(3, 12) == 3 * 12 ** 3 * 16
    for B, G in ((0, 8), (1, 1), (1, 1025), (65536, 8)):
        with pytest.raises(_lib.HipExtensionError):
            _lib.render_volume_packed_elems(B, G)


# ------------------------------------------------------------------------------------------------ command-line flags
def test_demo_flags():
    import demo
    a = demo.parse_args([])
    assert a.render_volumes is False and a.save_volumes is False and a.volume_joints is None
    a = demo.parse_args(["--render_dir", "d", "--render_volumes", "true", "--volume_joints", "9,10,13,14", "--save_volumes", "TRUE"])
    assert a.render_volumes is True and a.save_volumes is True and a.volume_joints == (9, 10, 13, 14)
    for bad in (["--render_volumes", "yes"], ["--render_volumes", "true"], ["--render_dir", "d", "--volume_joints", "1"],
                ["--render_dir", "d", "--render_volumes", "true", "--volume_joints", "15"],
                ["--render_dir", "d", "--render_volumes", "true", "--volume_joints", "a,b"], ["--save_volumes", "1"]):
        with pytest.raises(SystemExit):
            demo.parse_args(bad)


def test_run_sequence_flags():
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    a = run_sequence.parse_args(base)
    assert a.render_volumes is False and a.volume_joints is None
    a = run_sequence.parse_args(base + ["--render_dir", "d", "--render_volumes", "true", "--volume_joints", "3, 6"])
    assert a.render_volumes is True and a.volume_joints == (3, 6)
    for bad in (["--render_volumes", "true"], ["--render_dir", "d", "--render_volumes", "maybe"],
                ["--render_dir", "d", "--render_volumes", "true", "--volume_joints", "-1"]):
        with pytest.raises(SystemExit):
            run_sequence.parse_args(base + bad)


def test_visualize_flags():
    import visualize
    a = visualize.parse_args(["--img_path", "i", "--depth_path", "d", "--pose_path", "p"])
    assert a.volumes_path is None
    a = visualize.parse_args(["--img_path", "i", "--depth_path", "d", "--pose_path", "p", "--volumes_path", "v.npy",
                              "--volume_joints", "0"])
    assert a.volumes_path == "v.npy" and a.volume_joints == (0,)
