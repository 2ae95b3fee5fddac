"""CPU: the float64 model of the filter's backward pass (tests/volume_smoother_model.py) gives the forward-backward marginals of the
hidden Markov model it claims to, has the properties the definition promises, the demonstration the smoother exists for holds on it,
and the Python surface refuses bad arguments before anything touches a device."""
import numpy as np
import pytest
import torch

from sceneego_amd import _lib, load_config
from sceneego_amd.volume_filter import gaussian_taps
from sceneego_amd.volume_smoother import VolumeSmoother
from volume_filter_cases import SIDE, coord_grid, make_logits, softmax32, taps_for
from volume_filter_model import blur3, volume_filter_model
from volume_smoother_model import volume_smoother_model


def _forward(p, c, w, G, floor):
    """The filter's model, its beliefs rounded to float32 as the kernel hands them on: (belief32, restarted)."""
    b, _, _, rs = volume_filter_model(p, c, w, G, floor)
    return b.astype(np.float32), rs


def _smooth(p, c, w, G, floor):
    b32, rs = _forward(p, c, w, G, floor)
    return b32, rs, volume_smoother_model(p, b32, rs, c, w, G, floor)


# ------------------------------------------------------------------------------------------------------------------ the claim
def test_the_model_equals_dense_forward_backward_marginals():
    """G = 4: the transition matrix M[n, m] = (1 - floor) K[n, m] + floor / N is built column by column with blur3 (column m is blur3 of
    the unit vector at m, so blur3(b) = K b) and the textbook alpha-beta recursion runs on it in float64.  The smoother takes float32
    beliefs, so the dense marginals are formed from the same rounded beliefs; that these are alpha is checked apart, below."""
    G, R, floor, T, rows = 4, 2, 1e-2, 5, 3
    N = G ** 3
    p = softmax32(make_logits(T, rows, G, R, seed=11) * 0.3)
    c, w = coord_grid(G), taps_for(G, R)
    eps = float(np.float32(floor))
    K = np.stack([blur3(np.eye(N)[m][None], w, G)[0] for m in range(N)], axis=1)
    M = (1.0 - eps) * K + eps / N                       # x_t = n given x_{t-1} = m
    b32, rs, sm = _smooth(p, c, w, G, floor)
    assert not rs[1:].any() and sm["smoothed"][:-1].all() and not sm["smoothed"][-1].any()
    P = p.astype(np.float64)
    worst = 0.0
    for r in range(rows):
        # beta_t(m) = sum_n M[n, m] p_{t+1}(n) beta_{t+1}(n); the marginal of frame t is b_t beta_t, normalised.  b_t is the model's own
        # filtered belief (rounded to float32: the smoother's input), which is alpha_t normalised up to that rounding.
        beta = np.ones(N)
        want = [None] * T
        want[T - 1] = b32[T - 1, r].astype(np.float64)
        for t in range(T - 2, -1, -1):
            beta = M.T @ (P[t + 1, r] * beta)
            beta /= beta.sum()
            g = b32[t, r].astype(np.float64) * beta
            want[t] = g / g.sum()
        for t in range(T):
            worst = max(worst, float(np.abs(sm["gamma"][t, r] - want[t]).max() / want[t].max()))
    print(f"dense forward-backward at G = {G}: worst difference {worst:.3e} of the peak")
    assert worst <= 1e-9
    # ... and alpha itself: the float64 filter against the dense alpha recursion, so that b beta is the marginal of the whole model
    b64 = volume_filter_model(p, c, w, G, floor)[0]
    for r in range(rows):
        alpha = P[0, r].copy()
        for t in range(1, T):
            alpha = P[t, r] * (M @ alpha)
            alpha /= alpha.sum()
            assert np.abs(alpha - b64[t, r]).max() <= 1e-9 * alpha.max()


def test_blur_with_reversed_taps_is_the_adjoint():
    G, R = 6, 2
    rng = np.random.default_rng(5)
    w = rng.random(2 * R + 1)                          # asymmetric
    x, y = rng.random((2, G ** 3)), rng.random((2, G ** 3))
    lhs, rhs = (blur3(x, w, G) * y).sum(), (x * blur3(y, w[::-1], G)).sum()
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert abs((blur3(x, w, G) * y).sum() - (x * blur3(y, w, G)).sum()) > 1e-3 * abs(lhs)      # not self-adjoint: the reversal matters


def test_time_reversal():
    """Smoothing the time-reversed sequence gives the time-reversed marginals: the model is symmetric in time for symmetric taps.  The
    property belongs to the recursion, not to float32 beliefs (rounding b_t breaks it at 2^-24), so the model is given the float64
    beliefs of the filter model here."""
    T, rows, G, R, floor = 5, 3, 8, 2, 1e-3
    p = softmax32(make_logits(T, rows, G, R, seed=3))
    c, w = coord_grid(G), taps_for(G, R)

    def marginals(seq):
        b, _, _, rs = volume_filter_model(seq, c, w, G, floor)
        assert not rs[1:].any()
        return volume_smoother_model(seq, b, rs, c, w, G, floor)["gamma"]

    fwd, rev = marginals(p), marginals(p[::-1].copy())
    worst = float((np.abs(fwd - rev[::-1]).max(axis=2) / fwd.max(axis=2)).max())
    print(f"time reversal: worst difference {worst:.3e} of the peak")
    assert worst <= 1e-12
    # on the float32 beliefs the kernel is given, the marginals differ from these by that rounding only
    b, _, _, rs = volume_filter_model(p, c, w, G, floor)
    sm = volume_smoother_model(p, b.astype(np.float32), rs, c, w, G, floor)
    assert np.abs(sm["gamma"] - fwd).max() <= 2.0 ** -22 * fwd.max()


def test_the_last_frame_is_the_filtered_belief_bit_for_bit():
    T, rows, G, R = 4, 3, 8, 2
    p = softmax32(make_logits(T, rows, G, R, seed=3))
    b32, rs, sm = _smooth(p, coord_grid(G), taps_for(G, R), G, 1e-3)
    assert np.array_equal(sm["gamma"][-1], b32[-1].astype(np.float64)) and np.array_equal(sm["r"][-1], p[-1].astype(np.float64))
    assert not sm["smoothed"][-1].any() and np.isnan(sm["agreement"][-1]).all() and not sm["linked"][-1].any()
    assert sm["smoothed"][:-1].all() and np.abs(sm["gamma"].sum(axis=2) - 1).max() <= 1e-6


def test_the_model_does_not_depend_on_how_the_frames_are_cut():
    T, rows, G, R = 5, 3, 8, 2
    p = softmax32(make_logits(T, rows, G, R, seed=3))
    c, w = coord_grid(G), taps_for(G, R)
    b32, rs = _forward(p, c, w, G, 1e-3)
    whole = volume_smoother_model(p, b32, rs, c, w, G, 1e-3)
    second = volume_smoother_model(p[2:], b32[2:], rs[2:], c, w, G, 1e-3)
    first = volume_smoother_model(p[:2], b32[:2], rs[:2], c, w, G, 1e-3, state=second["r"][0], have_link=~rs[2])
    for key in whole:
        assert np.array_equal(whole[key], np.concatenate([first[key], second[key]]), equal_nan=True), key


def test_a_forward_restart_cuts_the_chain_both_ways():
    T, rows, G, R = 6, 3, 8, 2
    p = softmax32(make_logits(T, rows, G, R, seed=3))
    c, w = coord_grid(G), taps_for(G, R)
    clean = _smooth(p, c, w, G, 1e-3)[2]
    bad = p.copy()
    bad[3, 1, 77] = np.nan                             # the filter restarts row 1 at frames 3 and 4
    b32, rs, sm = _smooth(bad, c, w, G, 1e-3)
    assert rs[:, 1].tolist() == [True, False, False, True, True, False]
    assert sm["linked"][:, 1].tolist() == [True, True, False, False, True, False]
    assert sm["smoothed"][:, 1].tolist() == [True, True, False, False, True, False]
    for key in sm:
        assert np.array_equal(sm[key][:, [0, 2]], clean[key][:, [0, 2]], equal_nan=True), key
    # the NaN stays in frame 3: gamma_3 = b_3 = p_3 holds it, no frame before or after does
    assert np.isnan(sm["gamma"][3, 1]).any() and np.isnan(sm["joints"][3, 1]).all()
    for t in (0, 1, 2, 4, 5):
        assert np.isfinite(sm["gamma"][t, 1]).all() and np.isfinite(sm["r"][t, 1]).all() and np.isfinite(sm["joints"][t, 1]).all()
    assert np.array_equal(sm["gamma"][2, 1], b32[2, 1].astype(np.float64)) and np.array_equal(sm["r"][2, 1], p[2, 1].astype(np.float64))
    assert np.array_equal(sm["gamma"][3, 1], b32[3, 1].astype(np.float64), equal_nan=True)
    # frames 0..2 of the row are smoothed over 0..2 alone: the same as smoothing the sequence cut there
    head = volume_smoother_model(p[:3, 1:2], b32[:3, 1:2], rs[:3, 1:2], c, w, G, 1e-3)
    assert np.array_equal(sm["gamma"][:3, 1:2], head["gamma"])


def test_a_nan_in_the_backward_sum_falls_back_to_the_copy():
    """s and S are decided apart: a volume with a NaN in a frame the filter did not restart at cannot occur (the filter restarts on it),
    so the fallback is entered through the state a caller hands over."""
    T, rows, G, R = 2, 2, 6, 1
    p = softmax32(make_logits(T, rows, G, R, seed=4))
    c, w = coord_grid(G), taps_for(G, R)
    b32, rs = _forward(p, c, w, G, 1e-3)
    state = p[1].astype(np.float64).copy()
    state[0, 5] = np.nan
    sm = volume_smoother_model(p, b32, rs, c, w, G, 1e-3, state=state, have_link=np.ones(rows, dtype=bool))
    assert sm["linked"][1].all() and sm["smoothed"][1].tolist() == [False, True] and np.isnan(sm["agreement"][1, 0])
    assert np.array_equal(sm["gamma"][1, 0], b32[1, 0].astype(np.float64)) and np.array_equal(sm["r"][1, 0], p[1, 0].astype(np.float64))
    assert sm["smoothed"][0].all() and np.isfinite(sm["gamma"][0]).all()


# ------------------------------------------------------------------------------------------------------------------ the demonstration
def _two_lobes(T, false_frames, factor):
    """G = 16: lobe A (logit amplitude 8, 1.5 voxels wide) moves 0.5 voxel per frame from (4, 4, 4); the static lobe B at (12, 11, 12)
    has ``factor`` times its amplitude in ``false_frames``.  (softmaxed volumes [T, 1, N], the centres of A, voxel coordinates)"""
    G, width = 16, 1.5
    ax = np.arange(G, dtype=np.float64)

    def bump(c):
        g = [np.exp(-(ax - c[a]) ** 2 / (2 * width * width)) for a in range(3)]
        return g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]

    centres = np.array([[4.0, 4.0, 4.0 + 0.5 * t] for t in range(T)])
    logits = np.zeros((T, 1, G ** 3), dtype=np.float32)
    for t in range(T):
        v = 8.0 * bump(centres[t])
        if t in false_frames:
            v = v + factor * 8.0 * bump(np.array([12.0, 11.0, 12.0]))
        logits[t, 0] = v.reshape(-1)
    voxel = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return softmax32(logits), centres, voxel


def _distances(p, centres, voxel, floor):
    G, R = 16, 5
    w = gaussian_taps(0.2, R, SIDE / G)
    b32, rs, sm = _smooth(p, coord_grid(G), w, G, floor)
    raw = np.linalg.norm(p[:, 0].astype(np.float64) @ voxel - centres, axis=1)
    filtered = np.linalg.norm(b32[:, 0].astype(np.float64) @ voxel - centres, axis=1)
    smoothed = np.linalg.norm(sm["gamma"][:, 0] @ voxel - centres, axis=1)
    return raw, filtered, smoothed


@pytest.mark.parametrize("floor", [0.0, 1e-3, 1e-2])
def test_later_frames_resolve_an_ambiguous_first_frame(floor):
    """A second lobe at 1.02 x the logit amplitude in frame 0 only: the filter has no prior there, so the raw and the filtered joint are
    dragged towards it (6.9 voxels off here); the smoothed joint is within 0.5 voxel of lobe A in every frame (0.083 here)."""
    p, centres, voxel = _two_lobes(6, (0,), 1.02)
    raw, filtered, smoothed = _distances(p, centres, voxel, floor)
    print(f"floor {floor}: raw {np.round(raw, 3).tolist()} filtered {np.round(filtered, 3).tolist()} "
          f"smoothed {np.round(smoothed, 3).tolist()} voxels from lobe A")
    assert raw[0] >= 5.0 and filtered[0] >= 5.0
    assert (smoothed <= 0.5).all()


def test_where_the_smoother_stops_helping():
    """Printed, not asserted (the README quotes them): the false lobe over frames 0..2, at 1.01, 1.05, 1.3 and 1.6 x the amplitude.  With
    these lobes (logit amplitude 8) the smoothed joint stays with lobe A up to 1.05 x, is pulled off it at 1.3 x (more the larger the
    floor) and stays with the false lobe at 1.6 x for any floor > 0: one jump is then the likelier explanation under the model."""
    for factor in (1.01, 1.05, 1.3, 1.6):
        p, centres, voxel = _two_lobes(6, (0, 1, 2), factor)
        for floor in (0.0, 1e-3, 1e-2):
            raw, filtered, smoothed = _distances(p, centres, voxel, floor)
            print(f"false lobe x{factor} in frames 0..2, floor {floor}: smoothed up to {smoothed.max():.3f} voxels from lobe A "
                  f"(per frame {np.round(smoothed, 3).tolist()}), filtered up to {filtered.max():.3f}, raw up to {raw.max():.3f}")


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_volume_smoother_refuses_bad_parameters_without_a_device():
    c = coord_grid(8)
    for kw in ({"sigma": -0.1}, {"sigma": float("nan")}, {"floor": -1e-3}, {"floor": 1.5}, {"floor": float("nan")}, {"radius": -1},
               {"radius": 8}, {"radius": 17}, {"radius": 1.5}, {"max_bytes": -1}, {"max_bytes": float("nan")}):
        with pytest.raises(ValueError):
            VolumeSmoother(c, 8, SIDE, **kw)
    with pytest.raises(ValueError):
        VolumeSmoother(c, 129, SIDE)
    with pytest.raises(ValueError):
        VolumeSmoother(c[:-1], 8, SIDE)
    s = VolumeSmoother(c, 8, SIDE, sigma=0.2, max_bytes=1 << 20)
    assert s.filter.radius == 3 and s.frames_stored == 0 and s.bytes_stored == 0 and s.max_bytes == 1 << 20


def test_push_and_finish_refuse_bad_calls_without_a_device():
    s = VolumeSmoother(coord_grid(8), 8, SIDE, sigma=0.2, max_bytes=1 << 20)
    good = torch.zeros((2, 3, 8, 8, 8))
    for bad in (torch.zeros((3, 8, 8, 8)), torch.zeros((2, 3, 8, 8, 4)), torch.zeros((2, 3, 6, 6, 6)), good.double(),
                torch.zeros((0, 3, 8, 8, 8)), good.numpy()):
        with pytest.raises(ValueError):
            s.push(bad)
    with pytest.raises(ValueError):
        s.push(good, joints=torch.zeros((2, 3, 2)))
    with pytest.raises(ValueError):
        s.finish()                                      # nothing stored
    s.reset()
    # a well-formed call gets as far as the device check: there is no CPU path
    with pytest.raises(_lib.HipExtensionError):
        s.push(good)
    assert s.frames_stored == 0


def test_the_network_entry_point_validates_on_the_host():
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    cfg = load_config()
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    s = net.volume_smoother()
    assert isinstance(s, VolumeSmoother) and s.filter.grid == net.volume_size and s.filter.radius == 10 and s.filter.floor == 1e-3
    assert s.max_bytes is None and net.volume_smoother(max_bytes=123).max_bytes == 123
    with pytest.raises(ValueError):
        net.volume_smoother(sigma=-1.0)
    cfg.model.volume_softmax = False
    with pytest.raises(ValueError):
        VoxelNetwork_depth(cfg, device="cpu", verbose=False).volume_smoother()


def test_binding_lists_the_smoother():
    assert _lib.ABI_VERSION >= 35
    assert "se_volume_smooth_f32" in _lib.SIGNATURES and "se_volume_smooth_scratch_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["se_volume_smooth_f32"][1]) == 20
    lib = _lib.load()
    assert lib.se_volume_smooth_scratch_bytes(15, 64, 10) >= 15 * (2 * 64 ** 3 + 8 * 64) * 4
    assert lib.se_volume_smooth_scratch_bytes(15, 64, 17) == 0 and lib.se_volume_smooth_scratch_bytes(3, 6, 6) == 0
    assert lib.se_volume_smooth_scratch_bytes(0, 64, 10) == 0 and lib.se_volume_smooth_scratch_bytes(1, 128, 16) > 0
    assert lib.se_volume_smooth_scratch_bytes(15, 64, 10) % 16 == 0
    assert _lib.SMOOTH_CHAIN <= 512                         # the GPU test's tolerance is built on it


def test_run_sequence_parser_takes_the_smoother_flags():
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    a = run_sequence.parse_args(base)
    assert a.smooth is None and a.filter is None
    a = run_sequence.parse_args(base + ["--smooth_output", "s.pkl", "--filter_sigma", "0.05", "--filter_radius", "4"])
    assert a.filter == {"sigma": 0.05, "radius": 4, "floor": 1e-3} and a.smooth == {"max_bytes": None} and a.filter_output is None
    a = run_sequence.parse_args(base + ["--smooth_info_output", "i.pkl", "--smooth_max_gb", "1.5"])
    assert a.smooth == {"max_bytes": int(1.5 * 2 ** 30)} and a.filter is not None
    for bad in (["--smooth_output", "s.pkl", "--smooth_max_gb", "-1"], ["--smooth_max_gb", "1"]):
        with pytest.raises(SystemExit):
            run_sequence.parse_args(base + bad)
