"""CPU: the numpy model of the max-product pass (tests/volume_viterbi_model.py) finds the best path of the hidden Markov model it claims
to (against a dense Viterbi), has the properties the definition promises, the demonstration the path exists for holds on it, and the
Python surface refuses bad arguments before anything touches a device."""
import numpy as np
import pytest
import torch

from sceneego_amd import _lib, load_config
from sceneego_amd.volume_viterbi import VolumeViterbi, segment_log_scores
from volume_filter_cases import SIDE, coord_grid, make_logits, softmax32, taps_for
from volume_filter_model import volume_filter_model
from volume_smoother_model import volume_smoother_model
from volume_viterbi_model import JUMP, dense_viterbi, refine_model, viterbi_path, volume_viterbi_model


def _path(p, w, G, floor, dtype=np.float32, refine=1, coord=None):
    m = volume_viterbi_model(p, w, G, floor, dtype=dtype)
    index, jumped = viterbi_path(m["back"], m["peak"], m["restarted"])
    m["index"], m["jumped"] = index, jumped
    if coord is not None:
        m["joints"] = refine_model(p, coord, index, G, refine)
    return m


def _log_score(m):
    return segment_log_scores(m["best"], m["exponent"], m["restarted"])


# ------------------------------------------------------------------------------------------------------------------ the claim
def test_the_model_finds_the_best_path_of_the_dense_recursion():
    """G = 4, float64: the score of the model's path equals the best score of a Viterbi over all 64 x 64 transitions with the score
    max(keep W(d), uniform), to 1e-12 relative, and the path itself is the dense one on every seed where the dense recursion won each
    of its choices along that path by more than 1e-9 (a closer call may go either way between two orders of the same products)."""
    G, T = 4, 6
    tried = qualified = 0
    for seed in range(24):
        R, floor = (1, 2, 3)[seed % 3], (1e-3, 1e-2, 0.1, 0.0)[seed % 4]
        p = softmax32(make_logits(T, 1, G, R, seed=7000 + seed))
        w = taps_for(G, R)
        want_log, want_path, gap = dense_viterbi(p[:, 0], w, G, floor)
        m = _path(p, w, G, floor, dtype=np.float64)
        assert m["restarted"][:, 0].tolist() == [True] + [False] * (T - 1)
        got_log = _log_score(m)[-1, 0]
        assert abs(got_log - want_log) <= 1e-12 * max(1.0, abs(want_log)), (seed, got_log, want_log)
        tried += 1
        if gap > 1e-9:
            qualified += 1
            assert m["index"][:, 0].tolist() == want_path.tolist(), seed
    print(f"{qualified} of {tried} seeds decide every choice on the best path by more than 1e-9")
    assert qualified >= 0.9 * tried


# ------------------------------------------------------------------------------------------------------------------ the demonstration
def _ghost(T, true_factor=None, ghost_factor=1.0):
    """16^3: the true lobe (logit amplitude 8, 1 voxel wide) at (3 + 0.5 t, 4, 5) and its mirror image, the ghost, 7 voxels away at
    (3 + 0.5 t, 11, 5) with ``ghost_factor`` times the amplitude; ``true_factor``: {frame: factor} for the true lobe.  (softmaxed
    volumes [T, 1, N], the centres of the true lobe and of the ghost, the voxel-index coordinates [N, 3] float32)"""
    G = 16
    ax = np.arange(G, dtype=np.float64)

    def bump(c):
        g = [np.exp(-(ax - c[a]) ** 2 / 2.0) for a in range(3)]
        return g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]

    true = np.array([[3.0 + 0.5 * t, 4.0, 5.0] for t in range(T)])
    ghost = true + np.array([0.0, 7.0, 0.0])
    logits = np.zeros((T, 1, G ** 3), dtype=np.float32)
    for t in range(T):
        f = (true_factor or {}).get(t, 1.0)
        logits[t, 0] = (f * 8.0 * bump(true[t]) + ghost_factor * 8.0 * bump(ghost[t])).reshape(-1)
    voxel = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    return softmax32(logits), true, ghost, voxel


def _ghost_distances(p, true, ghost, voxel, floor):
    """Voxels from the true lobe and from the ghost, per frame: the smoothed joint, the path's voxel centre, the refined path joint."""
    G, R = 16, 5
    w = taps_for(G, R)
    c = coord_grid(G)
    b, _, _, rs = volume_filter_model(p, c, w, G, floor)
    b32 = b.astype(np.float32)
    sm = volume_smoother_model(p, b32, rs, c, w, G, floor)
    smoothed = sm["gamma"][:, 0] @ voxel.astype(np.float64)
    m = _path(p, w, G, floor, refine=1, coord=voxel)
    centre = voxel[m["index"][:, 0]].astype(np.float64)
    refined = m["joints"][:, 0].astype(np.float64)
    d = lambda x, to: np.linalg.norm(x - to, axis=1)            # noqa: E731
    return {"smoothed": (d(smoothed, true), d(smoothed, ghost)), "centre": (d(centre, true), d(centre, ghost)),
            "refined": (d(refined, true), d(refined, ghost)), "jumped": m["jumped"][:, 0]}


@pytest.mark.parametrize("floor", [0.0, 1e-3, 1e-2])
def test_two_equal_lobes_the_smoothed_joint_is_between_them_and_the_path_on_one(floor):
    p, true, ghost, voxel = _ghost(8)
    r = _ghost_distances(p, true, ghost, voxel, floor)
    s = np.minimum(*r["smoothed"])
    print(f"balanced, floor {floor}: smoothed joint {s.min():.2f} - {s.max():.2f} voxels from the nearer lobe; path voxel centre at most "
          f"{np.minimum(*r['centre']).max():.3f}, refined at most {np.minimum(*r['refined']).max():.3f} voxel from its lobe")
    assert (r["smoothed"][0] > 1.5).all() and (r["smoothed"][1] > 1.5).all()
    on_true, on_ghost = (r["centre"][0] < 1.0).all(), (r["centre"][1] < 1.0).all()
    assert on_true != on_ghost and not r["jumped"].any()      # one lobe, the same one in all 8 frames
    assert np.minimum(*r["refined"]).max() < 0.1


def test_one_frame_of_evidence_puts_the_path_on_the_true_lobe():
    p, true, ghost, voxel = _ghost(8, true_factor={3: 1.1})
    r = _ghost_distances(p, true, ghost, voxel, 1e-3)
    print(f"true lobe at 1.1 x in frame 3: smoothed joint {r['smoothed'][0].min():.2f} - {r['smoothed'][0].max():.2f} voxels from the true "
          f"lobe, refined path at most {r['refined'][0].max():.3f}")
    assert (r["smoothed"][0] > 1.5).all() and (r["smoothed"][1] > 1.5).all()
    assert (r["refined"][0] < 0.1).all()


def test_the_limit_a_slightly_stronger_ghost_is_followed_in_every_frame():
    for kw in ({"ghost_factor": 1.02}, {"ghost_factor": 1.05, "true_factor": {3: 1.3}}):
        p, true, ghost, voxel = _ghost(8, **kw)
        r = _ghost_distances(p, true, ghost, voxel, 1e-3)
        print(f"{kw}: smoothed joint {r['smoothed'][0].min():.2f} - {r['smoothed'][0].max():.2f} voxels from the truth, path "
              f"{r['refined'][0].min():.2f} - {r['refined'][0].max():.2f} (on the ghost to {r['refined'][1].max():.3f})")
        if "true_factor" not in kw:
            assert (r["centre"][1] < 1.0).all() and (r["refined"][0] > 6.0).all()


# ------------------------------------------------------------------------------------------------------------------ properties
def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def test_the_model_does_not_depend_on_how_the_frames_are_cut():
    rows, G, R, T, floor = 3, 8, 3, 5, 1e-3
    p = softmax32(make_logits(T, rows, G, R, seed=11))
    w = taps_for(G, R)
    whole = volume_viterbi_model(p, w, G, floor)
    a = volume_viterbi_model(p[:2], w, G, floor)
    b = volume_viterbi_model(p[2:], w, G, floor, state=a["state"][-1], peak_state=a["peak"][-1], best_state=a["best"][-1],
                             have_prior=np.ones(rows))
    for key in ("state", "back", "peak", "best", "exponent", "restarted"):
        assert np.array_equal(_bits(whole[key]), _bits(np.concatenate([a[key], b[key]]))), key
    assert (whole["best"] >= 1).all() and (whole["best"] < 2).all()
    assert whole["restarted"].tolist() == [[True] * rows] + [[False] * rows] * (T - 1)


def test_a_teleporting_lobe_is_reached_by_a_jump():
    G, R, floor = 8, 1, 1e-2
    ax = np.arange(G, dtype=np.float64)
    logits = np.zeros((4, 1, G ** 3), dtype=np.float32)
    for t, c in enumerate(((1, 1, 1), (1, 1, 2), (6, 6, 6), (6, 6, 5))):
        g = [np.exp(-(ax - c[a]) ** 2 / 2.0) for a in range(3)]
        logits[t, 0] = (12.0 * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]).reshape(-1)
    m = _path(softmax32(logits), taps_for(G, R), G, floor)
    assert m["jumped"][:, 0].tolist() == [False, False, True, False]
    assert m["index"][:, 0].tolist() == [(1 * G + 1) * G + 1, (1 * G + 1) * G + 2, (6 * G + 6) * G + 6, (6 * G + 6) * G + 5]
    assert m["back"][2, 0, m["index"][2, 0]] == (m["index"][1, 0] | JUMP) and not m["restarted"][1:].any()
    assert m["jump_bits"][2, 0] > 0
    # with floor = 0 a jump scores 0 and is never taken: no back-pointer carries the bit, the path creeps through the background
    z = _path(softmax32(logits), taps_for(G, R), G, 0.0)
    assert not z["jumped"].any() and not z["jump_bits"].any() and not z["restarted"][1:].any()


def test_a_zeroed_frame_starts_a_segment_and_the_segments_equal_separate_runs():
    rows, G, R, T, floor = 2, 8, 2, 6, 1e-3
    p = softmax32(make_logits(T, rows, G, R, seed=5))
    p[3, 1] = 0.0
    w = taps_for(G, R)
    m = _path(p, w, G, floor)
    assert m["restarted"][:, 1].tolist() == [True, False, False, True, True, False]
    assert m["peak"][3, 1] == -1 and np.isnan(m["best"][3, 1]) and m["exponent"][3, 1] == 0 and m["index"][3, 1] == -1
    assert (m["back"][3, 1] == -1).all() and (m["back"][4, 1] == -1).all() and np.array_equal(m["state"][3, 1], p[3, 1])
    head, tail = _path(p[:3], w, G, floor), _path(p[4:], w, G, floor)
    for key in ("state", "back", "peak", "best", "exponent", "index", "jumped"):
        assert np.array_equal(_bits(m[key][:3, 1]), _bits(head[key][:, 1])), key
        assert np.array_equal(_bits(m[key][4:, 1]), _bits(tail[key][:, 1])), key
    clean = _path(softmax32(make_logits(T, rows, G, R, seed=5)), w, G, floor)
    for key in ("state", "back", "index"):
        assert np.array_equal(_bits(m[key][:, 0]), _bits(clean[key][:, 0])), key
    ls = _log_score(m)
    assert np.isfinite(ls[[2, 5], 1]).all() and np.isnan(ls[[0, 1, 3, 4], 1]).all() and np.isfinite(ls[5, 0]) and np.isnan(ls[:5, 0]).all()
    # a NaN cell is passed over by every maximum and by the refinement
    q = softmax32(make_logits(T, rows, G, R, seed=5))
    q[2, 0, 77] = np.nan
    n = _path(q, w, G, floor, coord=coord_grid(G))
    assert not n["restarted"][1:, 0].any() and np.isnan(n["state"][2, 0, 77]) and np.isfinite(n["joints"]).all()


def test_float32_and_float64_give_the_same_path_on_these_inputs():
    rows, G, R, T, floor = 3, 8, 3, 5, 1e-3
    p = softmax32(make_logits(T, rows, G, R, seed=11))
    w = taps_for(G, R)
    a, b = _path(p, w, G, floor), _path(p, w, G, floor, dtype=np.float64)
    assert np.array_equal(a["index"], b["index"]) and not a["tied"].any()


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_volume_viterbi_refuses_bad_parameters_without_a_device():
    c = coord_grid(8)
    for kw in ({"sigma": -0.1}, {"sigma": float("nan")}, {"floor": -1e-3}, {"floor": 1.5}, {"floor": float("nan")}, {"radius": -1},
               {"radius": 8}, {"radius": 17}, {"radius": 1.5}, {"max_bytes": -1}, {"max_bytes": float("nan")}, {"refine": -1},
               {"refine": 4}, {"refine": 1.5}, {"refine": True}):
        with pytest.raises(ValueError):
            VolumeViterbi(c, 8, SIDE, **kw)
    with pytest.raises(ValueError):
        VolumeViterbi(c, 129, SIDE)
    with pytest.raises(ValueError):
        VolumeViterbi(c[:-1], 8, SIDE)
    v = VolumeViterbi(c, 8, SIDE, sigma=0.2, max_bytes=1 << 20)
    assert v.filter.radius == 3 and v.refine == 1 and v.frames_stored == 0 and v.bytes_stored == 0 and v.max_bytes == 1 << 20
    assert v.state is None


def test_push_and_finish_refuse_bad_calls_without_a_device():
    v = VolumeViterbi(coord_grid(8), 8, SIDE, sigma=0.2, max_bytes=1 << 20)
    good = torch.zeros((2, 3, 8, 8, 8))
    for bad in (torch.zeros((3, 8, 8, 8)), torch.zeros((2, 3, 8, 8, 4)), torch.zeros((2, 3, 6, 6, 6)), good.double(),
                torch.zeros((0, 3, 8, 8, 8)), good.numpy()):
        with pytest.raises(ValueError):
            v.push(bad)
    with pytest.raises(ValueError):
        v.push(good, joints=torch.zeros((2, 3, 2)))
    with pytest.raises(ValueError):
        v.finish()                                      # nothing stored
    v.reset()
    with pytest.raises(_lib.HipExtensionError):         # a well-formed call gets as far as the device check: there is no CPU path
        v.push(good)
    assert v.frames_stored == 0 and v.frames_seen == 0


def test_the_network_entry_point_validates_on_the_host():
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    cfg = load_config()
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    v = net.volume_path()
    assert isinstance(v, VolumeViterbi) and v.filter.grid == net.volume_size and v.filter.radius == 10 and v.filter.floor == 1e-3
    assert v.refine == 1 and v.max_bytes is None and net.volume_path(max_bytes=123, refine=0).max_bytes == 123
    with pytest.raises(ValueError):
        net.volume_path(sigma=-1.0)
    with pytest.raises(ValueError):
        net.volume_path(refine=9)
    cfg.model.volume_softmax = False
    with pytest.raises(ValueError):
        VoxelNetwork_depth(cfg, device="cpu", verbose=False).volume_path()


def test_binding_lists_the_viterbi_entry_points():
    assert _lib.ABI_VERSION >= 36
    for name, n in (("se_volume_viterbi_f32", 20), ("se_volume_viterbi_path_i32", 11), ("se_volume_viterbi_refine_f32", 10),
                    ("se_volume_viterbi_scratch_bytes", 3)):
        assert len(_lib.SIGNATURES[name][1]) == n, name
    lib = _lib.load()
    assert lib.se_volume_viterbi_scratch_bytes(15, 64, 10) >= 15 * ((64 ** 3 + 4 * 64) * 4 + 2 * 64 ** 3)
    assert lib.se_volume_viterbi_scratch_bytes(15, 64, 17) == 0 and lib.se_volume_viterbi_scratch_bytes(3, 6, 6) == 0
    assert lib.se_volume_viterbi_scratch_bytes(0, 64, 10) == 0 and lib.se_volume_viterbi_scratch_bytes(1, 128, 16) > 0
    assert lib.se_volume_viterbi_scratch_bytes(1, 3, 1) % 16 == 0
    # the C entry points refuse null pointers before they touch a device
    assert lib.se_volume_viterbi_f32(*([None] * 11), 0, 1, 1, 8, 2, 1, 0.0, None, None) == -1
    assert lib.se_volume_viterbi_path_i32(*([None] * 6), 1, 1, 8, 0, None) == -1
    assert lib.se_volume_viterbi_refine_f32(*([None] * 4), 1, 1, 8, 2, 0, None) == -1


def test_run_sequence_parser_takes_the_path_flags():
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    a = run_sequence.parse_args(base)
    assert a.path is None and a.filter is None
    a = run_sequence.parse_args(base + ["--path_output", "p.pkl", "--filter_sigma", "0.05", "--filter_radius", "4"])
    assert a.path == {"sigma": 0.05, "radius": 4, "floor": 1e-3, "refine": 1, "max_bytes": None} and a.filter is None and a.smooth is None
    a = run_sequence.parse_args(base + ["--path_info_output", "i.pkl", "--path_max_gb", "1.5", "--path_refine", "0"])
    assert a.path["max_bytes"] == int(1.5 * 2 ** 30) and a.path["refine"] == 0
    for bad in (["--path_output", "p.pkl", "--path_max_gb", "-1"], ["--path_max_gb", "1"], ["--path_refine", "2"],
                ["--path_output", "p.pkl", "--path_refine", "7"]):
        with pytest.raises(SystemExit):
            run_sequence.parse_args(base + bad)
