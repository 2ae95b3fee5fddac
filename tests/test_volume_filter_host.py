"""CPU: the float64 model of the grid Bayes filter (tests/volume_filter_model.py) has the properties the definition promises, the
demonstration the filter exists for holds on it, and the Python surface refuses bad arguments before anything touches a device."""
import numpy as np
import pytest
import torch

from sceneego_amd import _lib, load_config
from sceneego_amd.volume_filter import VolumeFilter, default_radius, gaussian_taps
from volume_filter_cases import SIDE, coord_grid, make_logits, softmax32, taps_for
from volume_filter_model import blur3, volume_filter_model


def _sequence(T, rows, G, R, seed=3):
    return softmax32(make_logits(T, rows, G, R, seed)), coord_grid(G)


# ------------------------------------------------------------------------------------------------------------------ taps
@pytest.mark.parametrize("sigma,radius,h", [(0.1, 10, 2.0 / 64), (0.2, 5, 0.125), (0.05, 1, 0.3), (3.0, 16, 0.01)])
def test_taps_sum_to_one_and_are_symmetric(sigma, radius, h):
    w = gaussian_taps(sigma, radius, h)
    assert w.dtype == np.float32 and w.shape == (2 * radius + 1,)
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= (2 * radius + 1) * 2.0 ** -25      # each tap rounded once
    assert np.array_equal(w, w[::-1]) and (w > 0).all() and w.argmax() == radius
    assert (np.diff(w[:radius + 1]) > 0).all()


def test_sigma_zero_or_radius_zero_is_the_identity():
    assert np.array_equal(gaussian_taps(0.0, 0, 0.1), np.ones(1, dtype=np.float32))
    assert np.array_equal(gaussian_taps(0.3, 0, 0.1), np.ones(1, dtype=np.float32))
    w = gaussian_taps(0.0, 3, 0.1)
    assert np.array_equal(w, np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float32))
    b = np.random.default_rng(0).random((2, 6 ** 3))
    assert np.array_equal(blur3(b, w, 6), b)


def test_default_radius():
    assert default_radius(0.10, 64, 2.0) == 10           # ceil(0.3 / 0.03125) = 10
    assert default_radius(1.0, 64, 2.0) == 16            # capped
    assert default_radius(1.0, 6, 2.0) == 5              # G - 1
    assert default_radius(0.0, 64, 2.0) == 0
    f = VolumeFilter(coord_grid(16), 16, SIDE, sigma=0.2)
    assert f.radius == 5 and f.taps.shape == (11,) and f.frames_seen == 0 and f.state is None


# ------------------------------------------------------------------------------------------------------------------ the model
def test_blur_is_zero_padded_and_loses_mass_at_the_border():
    G, R = 6, 2
    w = taps_for(G, R).astype(np.float64)
    b = np.zeros((1, G ** 3))
    b[0, 0] = 1.0                                          # the corner voxel
    q = blur3(b, w, G).reshape(G, G, G)
    assert np.allclose(q[:R + 1, :R + 1, :R + 1], np.einsum("i,j,k->ijk", w[R::-1], w[R::-1], w[R::-1]), rtol=1e-15, atol=0)
    assert q[R + 1:].sum() == 0 and q[:, R + 1:].sum() == 0 and q[:, :, R + 1:].sum() == 0
    assert abs(q.sum() - w[R:].sum() ** 3) < 1e-15 and q.sum() < 0.6     # nothing wraps round: the rest left the grid
    centre = np.zeros((1, G ** 3))
    centre[0, (3 * G + 3) * G + 3] = 1.0
    assert abs(blur3(centre, w, G).sum() - w[R - 2:R + 3].sum() ** 3) < 1e-15


def test_radius_zero_floor_zero_is_the_normalised_product():
    T, rows, G = 4, 3, 8
    p, c = _sequence(T, rows, G, 0)
    b, j, ev, rs = volume_filter_model(p, c, taps_for(G, 0), G, 0.0)
    want = p[0].astype(np.float64)
    for t in range(1, T):
        a = p[t].astype(np.float64) * want
        assert np.allclose(ev[t], a.sum(axis=1), rtol=1e-14, atol=0)
        want = a / a.sum(axis=1, keepdims=True)
        assert np.allclose(b[t], want, rtol=1e-13, atol=0)
    assert rs[0].all() and not rs[1:].any() and np.isnan(ev[0]).all()
    assert np.array_equal(b[0], p[0].astype(np.float64))


def test_floor_one_forgets_the_past():
    T, rows, G, R = 3, 2, 8, 2
    p, c = _sequence(T, rows, G, R)
    b, j, ev, rs = volume_filter_model(p, c, taps_for(G, R), G, 1.0)
    for t in range(1, T):
        s = p[t].astype(np.float64).sum(axis=1)
        assert np.allclose(b[t], p[t] / s[:, None], rtol=1e-13, atol=0)
        assert np.allclose(ev[t], s / G ** 3, rtol=1e-13, atol=0)
        assert np.allclose(j[t], (p[t] / s[:, None]) @ c.astype(np.float64), rtol=0, atol=1e-13)


@pytest.mark.parametrize("rows,G,R,floor", [(3, 8, 2, 1e-3), (2, 6, 5, 0.0), (4, 10, 3, 1e-2)])
def test_every_belief_sums_to_one(rows, G, R, floor):
    p, c = _sequence(5, rows, G, R)
    b, j, ev, rs = volume_filter_model(p, c, taps_for(G, R), G, floor)
    assert not rs[1:].any()
    assert np.abs(b[1:].sum(axis=2) - 1.0).max() <= 1e-12
    assert (b >= 0).all() and (ev[1:] > 0).all()


def test_the_model_does_not_depend_on_how_the_frames_are_cut():
    rows, G, R = 3, 8, 2
    p, c = _sequence(5, rows, G, R)
    w = taps_for(G, R)
    whole = volume_filter_model(p, c, w, G, 1e-3)
    first = volume_filter_model(p[:2], c, w, G, 1e-3)
    second = volume_filter_model(p[2:], c, w, G, 1e-3, state=first[0][-1], have_prior=np.ones(rows, dtype=bool))
    for a, x, y in zip(whole, first, second):
        assert np.array_equal(a, np.concatenate([x, y]), equal_nan=True)


def test_restart_on_disjoint_supports():
    G, R = 8, 1
    N = G ** 3
    c = coord_grid(G)
    p = np.zeros((3, 2, N), dtype=np.float32)
    p[:, 1] = softmax32(make_logits(3, 1, G, R, 9))[:, 0]           # an ordinary row beside it
    lo = np.zeros((G, G, G), dtype=np.float32)
    lo[:2, :2, :2] = 0.125
    hi = np.zeros((G, G, G), dtype=np.float32)
    hi[5:7, 5:7, 5:7] = 0.125
    p[0, 0], p[1, 0], p[2, 0] = lo.reshape(-1), hi.reshape(-1), hi.reshape(-1)      # frame 1 is out of reach of blur3(frame 0)
    b, j, ev, rs = volume_filter_model(p, c, taps_for(G, R), G, 0.0)
    assert rs.tolist() == [[True, True], [True, False], [False, False]]
    assert ev[1, 0] == 0.0 and np.array_equal(b[1, 0], p[1, 0].astype(np.float64))
    assert ev[2, 0] > 0 and abs(b[2, 0].sum() - 1) < 1e-12
    # with a floor the same frame is an update, not a restart
    b, j, ev, rs = volume_filter_model(p, c, taps_for(G, R), G, 1e-3)
    assert not rs[1:].any() and ev[1, 0] == pytest.approx(float(np.float32(1e-3)) / N, rel=1e-12)


def test_a_nan_row_restarts_twice_and_leaves_the_others_alone():
    rows, G, R = 3, 8, 2
    p, c = _sequence(5, rows, G, R)
    w = taps_for(G, R)
    clean = volume_filter_model(p, c, w, G, 1e-3)
    bad = p.copy()
    bad[2, 1, 77] = np.nan
    b, j, ev, rs = volume_filter_model(bad, c, w, G, 1e-3)
    assert rs[:, 1].tolist() == [True, False, True, True, False]
    assert rs[:, 0].tolist() == rs[:, 2].tolist() == [True, False, False, False, False]
    assert np.isnan(ev[2, 1]) and np.isnan(ev[3, 1]) and np.isnan(j[2, 1]).all() and np.isfinite(j[3, 1]).all()
    assert np.array_equal(b[2, 1], bad[2, 1].astype(np.float64), equal_nan=True) and np.array_equal(b[3, 1], p[3, 1].astype(np.float64))
    for x, y in zip((b, j, ev, rs), clean):
        assert np.array_equal(x[:, [0, 2]], y[:, [0, 2]], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ the demonstration
@pytest.mark.parametrize("floor", [0.0, 1e-3, 1e-2])
def test_the_filter_holds_on_to_the_lobe_it_followed(floor):
    """G = 16, sigma 0.2 m (1.6 voxels), R = 5.  Lobe A (logit amplitude 8, 1.5 voxels wide) moves 0.5 voxel per frame from (4, 4, 4);
    lobe B at (12, 11, 12) has 1.05 x its amplitude in frames 2-4 only.  The raw expectation sum p c is dragged more than 6 voxels from
    A in those frames (6.75-7.08 here); the filtered joint stays within 0.25 voxel of A from frame 1 on (below 0.09 here)."""
    G, R, T, width = 16, 5, 6, 1.5
    h = SIDE / G
    ax = np.arange(G, dtype=np.float64)

    def bump(c):
        g = [np.exp(-(ax - c[a]) ** 2 / (2 * width * width)) for a in range(3)]
        return g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]

    centres = np.array([[4.0, 4.0, 4.0 + 0.5 * t] for t in range(T)])
    logits = np.zeros((T, 1, G ** 3), dtype=np.float32)
    for t in range(T):
        v = 8.0 * bump(centres[t])
        if 2 <= t <= 4:
            v = v + 1.05 * 8.0 * bump(np.array([12.0, 11.0, 12.0]))
        logits[t, 0] = v.reshape(-1)
    p = softmax32(logits)
    voxel = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)          # coordinates in voxel units
    raw = np.linalg.norm(p[:, 0].astype(np.float64) @ voxel - centres, axis=1)
    b, j, ev, rs = volume_filter_model(p, coord_grid(G), gaussian_taps(0.2, R, h), G, floor)
    filtered = np.linalg.norm(b[:, 0] @ voxel - centres, axis=1)
    print(f"floor {floor}: raw {np.round(raw, 2).tolist()} filtered {np.round(filtered, 3).tolist()} voxels from lobe A")
    assert (raw[2:5] > 6.0).all()
    assert (filtered[1:] <= 0.25).all()
    assert not rs[1:].any()
    # the joints the model returns are the same expectation on the grid's own coordinates
    assert np.allclose(j[:, 0], b[:, 0] @ coord_grid(G).astype(np.float64), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_volume_filter_refuses_bad_parameters_without_a_device():
    c = coord_grid(8)
    for kw in ({"sigma": -0.1}, {"sigma": float("nan")}, {"sigma": float("inf")}, {"floor": -1e-3}, {"floor": 1.5},
               {"floor": float("nan")}, {"radius": -1}, {"radius": 8}, {"radius": 17}, {"radius": 1.5}):
        with pytest.raises(ValueError):
            VolumeFilter(c, 8, SIDE, **kw)
    with pytest.raises(ValueError):
        VolumeFilter(c, 1, SIDE)
    with pytest.raises(ValueError):
        VolumeFilter(c, 129, SIDE)
    with pytest.raises(ValueError):
        VolumeFilter(c, 8, 0.0)
    with pytest.raises(ValueError):
        VolumeFilter(c[:-1], 8, SIDE)
    with pytest.raises(ValueError):
        VolumeFilter(np.zeros((8, 8, 8, 2), dtype=np.float32), 8, SIDE)
    VolumeFilter(c.reshape(8, 8, 8, 3), 8, SIDE, sigma=0.0, radius=7, floor=1.0)
    VolumeFilter(torch.from_numpy(c), 8, SIDE, radius=0, floor=0.0)


def test_step_and_reset_refuse_bad_shapes_without_a_device():
    f = VolumeFilter(coord_grid(8), 8, SIDE, sigma=0.2)
    good = torch.zeros((2, 3, 8, 8, 8))
    for bad in (torch.zeros((3, 8, 8, 8)), torch.zeros((2, 3, 8, 8, 4)), torch.zeros((2, 3, 6, 6, 6)), good.double(),
                torch.zeros((0, 3, 8, 8, 8)), good.numpy()):
        with pytest.raises(ValueError):
            f.step(bad)
    with pytest.raises(ValueError):
        f.step(good, joints=torch.zeros((2, 3, 2)))
    with pytest.raises(ValueError):
        f.reset(rows=[0])                                   # no rows before the first step
    f.reset()
    assert f.frames_seen == 0
    # a well-formed call gets as far as the device check: there is no CPU path
    with pytest.raises(_lib.HipExtensionError):
        f.step(good)


def test_the_network_entry_point_validates_on_the_host():
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    cfg = load_config()
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    f = net.volume_filter()
    G = net.volume_size
    assert isinstance(f, VolumeFilter) and f.grid == G and f.cuboid_side == net.cuboid_side
    assert f.radius == default_radius(0.10, G, net.cuboid_side) and f.floor == 1e-3 and f.sigma == 0.10
    assert net.volume_filter(sigma=0.05, radius=3, floor=0.0).taps.shape == (7,)
    with pytest.raises(ValueError):
        net.volume_filter(sigma=-1.0)
    with pytest.raises(ValueError):
        net.volume_filter(radius=G)
    cfg.model.volume_softmax = False
    with pytest.raises(ValueError):
        VoxelNetwork_depth(cfg, device="cpu", verbose=False).volume_filter()


def test_binding_lists_the_filter():
    assert _lib.ABI_VERSION >= 33
    assert "se_volume_filter_f32" in _lib.SIGNATURES and "se_volume_filter_scratch_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["se_volume_filter_f32"][1]) == 18
    lib = _lib.load()
    assert lib.se_volume_filter_scratch_bytes(15, 64, 10) == 15 * (64 ** 3 + 8 * 64) * 4
    assert lib.se_volume_filter_scratch_bytes(15, 64, 17) == 0 and lib.se_volume_filter_scratch_bytes(3, 6, 6) == 0
    assert lib.se_volume_filter_scratch_bytes(3, 6, 5) > 0 and lib.se_volume_filter_scratch_bytes(0, 64, 10) == 0
    assert lib.se_volume_filter_scratch_bytes(1, 129, 10) == 0 and lib.se_volume_filter_scratch_bytes(1, 128, 16) > 0
    assert _lib.FILTER_CHAIN <= 512                         # the GPU test's tolerance is built on it


# ------------------------------------------------------------------------------------------------------------------ command line
def test_run_sequence_parser_takes_the_filter_flags():
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    a = run_sequence.parse_args(base)
    assert a.filter is None and a.render_volumes is False and a.render_filtered is False
    a = run_sequence.parse_args(base + ["--filter_output", "f.pkl"])
    assert a.filter == {"sigma": 0.1, "radius": None, "floor": 1e-3} and a.filter_info_output is None
    a = run_sequence.parse_args(base + ["--filter_info_output", "i.pkl", "--filter_sigma", "0.05", "--filter_radius", "4",
                                        "--filter_floor", "0"])
    assert a.filter == {"sigma": 0.05, "radius": 4, "floor": 0.0}
    a = run_sequence.parse_args(base + ["--render_volumes", "filtered", "--render_dir", "d"])
    assert a.render_volumes is True and a.render_filtered is True and a.filter is not None
    a = run_sequence.parse_args(base + ["--render_volumes", "true", "--render_dir", "d"])
    assert a.render_volumes is True and a.render_filtered is False and a.filter is None
    a = run_sequence.parse_args(base + ["--render_volumes", "false"])
    assert a.render_volumes is False and a.render_filtered is False
    for bad in (["--render_volumes", "beliefs", "--render_dir", "d"], ["--render_volumes", "filtered"],
                ["--filter_output", "f.pkl", "--filter_sigma", "-1"], ["--filter_output", "f.pkl", "--filter_floor", "2"],
                ["--filter_output", "f.pkl", "--filter_radius", "17"]):
        with pytest.raises(SystemExit):
            run_sequence.parse_args(base + bad)
