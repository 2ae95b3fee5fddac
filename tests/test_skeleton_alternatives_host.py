"""CPU: the numpy model of the runner-up poses (tests/skeleton_alternatives_model.py) against a brute force over all poses, the
agreement of every joint's max-marginal maximum with the pose's score, the float32 definition against the float64 recursion, what the
margin is for (the true and the mirrored ghost pair of the pose's host test), the command lines and the per-frame dicts.  Nothing here
touches a device."""
import itertools

import numpy as np
import pytest
import torch

from sceneego_amd import _lib, op
from sceneego_amd.skeleton_pose import SkeletonPose
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, shell_taps
from skeleton_alternatives_model import exponent_sums, skeleton_alternatives_model, window_mask
from skeleton_pose_model import pose_log_score, skeleton_pose_model
from skeleton_prior_cases import CHAIN3, STAR5, lengths_for, make_logits, taps_for, voxel_coord
from test_skeleton_pose_host import ghost_pair_logits
from volume_filter_cases import softmax32

TREE = KINEMATIC_PARENTS


def _case(parents, G, R, seed, frames=1):
    L = lengths_for(parents, G, R, seed)
    return softmax32(make_logits(frames, parents, L, G, seed)[0]), taps_for(L, G, R)


# ------------------------------------------------------------------------------------------------------------------ 1. brute force
@pytest.mark.parametrize("floor", [1e-3, 0.0])
@pytest.mark.parametrize("seed", [5, 6])
def test_brute_force_over_all_poses_of_a_chain(seed, floor):
    """G = 3, R = 2, separation 0: every max-marginal and every alternative pose against the 27^3 poses."""
    parents, G, R = CHAIN3, 3, 2
    N = G ** 3
    p, taps = _case(parents, G, R, seed)
    with np.errstate(divide="ignore"):
        scores = np.array([pose_log_score(p[0], taps, parents, G, floor, x) for x in itertools.product(range(N), repeat=3)]).reshape(N, N, N)
    got = skeleton_alternatives_model(p, taps, parents, G, floor, 0, dtype=np.float64)
    single = skeleton_alternatives_model(p, taps, parents, G, floor, 0, dtype=np.float32)
    assert got["complete"][0] and np.array_equal(got["index"], skeleton_pose_model(p, taps, parents, G, floor, dtype=np.float64)["index"])
    worst = 0.0
    for j in range(3):
        brute = scores.max(axis=tuple(a for a in range(3) if a != j))
        finite = np.isfinite(brute)
        assert finite.any() and (got["max_marginals"][0, j][~finite] == 0).all()
        worst = max(worst, np.abs(got["log_max_marginals"][0, j][finite] - brute[finite]).max())
        outside = window_mask(int(got["index"][0, j]), G, 0).reshape([N if a == j else 1 for a in range(3)])
        masked = np.where(outside, scores, -np.inf)
        best = np.unravel_index(int(masked.argmax()), masked.shape)
        assert np.sort(masked.reshape(-1))[-1] - np.sort(masked.reshape(-1))[-2] > 1e-9         # one best alternative
        assert got["alt_pose"][0, j].tolist() == list(best) == single["alt_pose"][0, j].tolist()
        assert abs(got["alt_log_score"][0, j] - masked.max()) <= 1e-12
        assert np.isclose(got["margin"][0, j], scores.max() - masked.max(), rtol=0, atol=1e-12)
    print(f"seed {seed} floor {floor}: log max-marginals against the brute force {worst:.2e}, margins {got['margin'][0].round(4).tolist()}")
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ 2. consistency
@pytest.mark.parametrize("tree,G,R,floor", [("tree15", 4, 3, 1e-3), ("star5", 4, 3, 1e-2), ("tree15", 8, 4, 1e-3)])
def test_every_joint_agrees_on_the_score_and_every_alternative_pose_has_its_score(tree, G, R, floor):
    parents = {"tree15": TREE, "star5": STAR5}[tree]
    J = len(parents)
    p, taps = _case(parents, G, R, seed=1)
    got = skeleton_alternatives_model(p, taps, parents, G, floor, 1, dtype=np.float64)
    single = skeleton_alternatives_model(p, taps, parents, G, floor, 1, dtype=np.float32)
    assert got["complete"][0] and (got["alt_index"][0] >= 0).all()
    spread = np.abs(got["log_mm_best"][0] - got["log_score"][0]).max()
    errs = [abs(pose_log_score(p[0], taps, parents, G, floor, got["alt_pose"][0, a].tolist()) - got["alt_log_score"][0, a]) for a in range(J)]
    print(f"{tree} G {G}: log score {got['log_score'][0]:.6f}, spread of the maxima {spread:.2e}, alternative poses {max(errs):.2e}")
    assert spread <= 1e-12 and max(errs) <= 1e-12
    assert np.array_equal(got["mm_peak"], got["index"]) and np.array_equal(got["pose_value"], got["mm_best"])
    assert (got["margin"][0] >= 0).all() and (got["alt_pose"][0][np.arange(J), np.arange(J)] == got["alt_index"][0]).all()
    for a in range(J):                                                   # the anchor is outside its window, and only it has to be
        assert window_mask(int(got["index"][0, a]), G, 1)[got["alt_index"][0, a]]
    # the float32 definition gives the float64 poses
    assert np.array_equal(single["index"], got["index"]) and np.array_equal(single["alt_pose"], got["alt_pose"])
    assert np.array_equal(single["alt_jumped"], got["alt_jumped"]) and single["max_marginals"].dtype == np.float32
    assert np.allclose(single["margin"], got["margin"], rtol=0, atol=1e-4)


def test_exponent_sums_cover_every_joint_once():
    """Esub_j + F_j adds the upward exponent of every joint outside the path and the downward one of every edge on it: with all
    upward exponents 1 and all downward ones 0 it counts the joints that are no proper ancestor of j."""
    J = len(TREE)
    Esub, F = exponent_sums(TREE, np.ones(J, dtype=np.int32), np.zeros(J, dtype=np.int32))
    depth = [0] * J
    for j in range(1, J):
        depth[j] = depth[TREE[j]] + 1
    assert (Esub + F).tolist() == [J - depth[j] for j in range(J)] and Esub[0] == J and F[0] == 0


def test_fallback_fills():
    G, R = 4, 3
    p, taps = _case(CHAIN3, G, R, seed=2, frames=2)
    bad = p.copy()
    bad[0, 1] = 0.0
    got = skeleton_alternatives_model(bad, taps, CHAIN3, G, 1e-3, 1)
    assert got["complete"].tolist() == [False, True] and got["solved"].tolist() == [False, True]
    assert (got["alt_index"][0] == -1).all() and (got["mm_peak"][0] == -1).all() and (got["alt_pose"][0] == -1).all()
    assert np.isnan(got["alt_value"][0]).all() and np.isnan(got["mm_best"][0]).all() and np.isnan(got["pose_value"][0]).all()
    assert not got["down_exponent"][0].any() and not got["alt_jumped"][0].any() and np.isnan(got["margin"][0]).all()
    assert np.array_equal(got["max_marginals"][0].view(np.int32), bad[0].view(np.int32))
    clean = skeleton_alternatives_model(p, taps, CHAIN3, G, 1e-3, 1)
    assert np.array_equal(got["alt_pose"][1], clean["alt_pose"][1]) and np.array_equal(got["margin"][1], clean["margin"][1])
    none = skeleton_alternatives_model(p, taps, CHAIN3, G, 1e-3, G - 1)   # a window that covers the grid: complete, no alternative
    assert none["complete"].all() and (none["alt_index"] == -1).all() and np.isposinf(none["margin"]).all()
    assert np.isneginf(none["alt_log_score"]).all() and (none["alt_value"] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ 3. what it is for
@pytest.mark.parametrize("lead,want_margin", [(1.02, 0.2400), (1.3, 3.600), (1 / 1.02, 0.2353)])
def test_the_margin_says_how_close_the_ghost_pair_was(lead, want_margin):
    """The true pair of lobes and the mirrored ghost pair of the pose's host test (16^3, R = 5, bones 3.5 and 3, tau 0.5 voxel, floor
    1e-3), separation 2: the pose follows the stronger pair on both joints, all or nothing; the runner-up pose of the elbow and of the
    wrist is the other pair on both joints, and the margin says by how much it lost.  Printed below and quoted in the README."""
    G, R = 16, 5
    logits, true, ghost = ghost_pair_logits(lead=lead)
    p = softmax32(logits)
    coord = voxel_coord(G).astype(np.float64)
    taps = shell_taps(np.array([0.0, 3.5, 3.0]), 0.5, 1.0, R)
    got = skeleton_alternatives_model(p, taps, CHAIN3, G, 1e-3, 2)
    pose = coord[got["index"][0]]
    first, second = (true, ghost) if lead > 1 else (ghost, true)
    assert got["complete"][0] and (np.linalg.norm(pose - first, axis=1) < 1.0).all()
    for a in (1, 2):
        alt = coord[got["alt_pose"][0, a]]
        d = np.linalg.norm(alt[1:] - second[1:], axis=1)
        print(f"lead {lead:.4f}, anchor {a}: runner-up {alt.tolist()}, {d.round(3).tolist()} voxels from the other pair's lobes, log margin "
              f"{got['margin'][0, a]:.4f}")
        assert (d <= 0.5).all() and abs(got["margin"][0, a] - want_margin) <= 1e-3
        assert not got["alt_jumped"][0, a].any()
    assert got["margin"][0, 0] > 3.0                                     # the root has one lobe: no close second place


# ------------------------------------------------------------------------------------------------------------------ 4. host surface
def test_alternatives_validates_before_the_device():
    s = SkeletonPose(np.zeros((8, 8, 8, 3), dtype=np.float32), 8, 2.0, [0.5] * 14)
    vols = torch.zeros((1, 15, 8, 8, 8))
    for kw in ({"separation": -1}, {"separation": 1.5}, {"separation": True}, {"separation": None}, {"joints": torch.zeros((2, 15, 3))}):
        with pytest.raises(ValueError):
            s.alternatives(vols, **kw)
    with pytest.raises(ValueError):
        s.alternatives(torch.zeros((1, 14, 8, 8, 8)))
    with pytest.raises(_lib.HipExtensionError):
        s.alternatives(vols)                                             # a CPU tensor: there is no fallback
    assert "se_skeleton_alternatives_f32" in _lib.SIGNATURES and "se_skeleton_alternatives_scratch_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["se_skeleton_alternatives_f32"][1]) == 28 and len(_lib.ALTERNATIVES_OUTPUTS) == 14


def test_command_line_parsers():
    import evaluate
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    a = run_sequence.parse_args(base + ["--map_alternatives_output", "alt.pkl"])
    assert a.map and a.map_alternatives_output == "alt.pkl" and a.map_separation is None and a.map_output is None and not a.skeleton
    a = run_sequence.parse_args(base + ["--map_alternatives_output", "alt.pkl", "--map_separation", "0", "--map_refine", "2", "--map_output", "m.pkl"])
    assert (a.map_separation, a.map_refine, a.map_output) == (0, 2, "m.pkl")
    assert run_sequence.parse_args(base + ["--map_output", "m.pkl"]).map_alternatives_output is None
    for bad in (["--map_separation", "2"], ["--map_output", "m.pkl", "--map_separation", "2"],
                ["--map_alternatives_output", "alt.pkl", "--map_separation", "-1"]):
        with pytest.raises(SystemExit):
            run_sequence.parse_args(base + bad)
    e = evaluate.build_parser().parse_args(["--pred_dir", "map.pkl", "--alternatives", "alt.pkl"])
    assert e.alternatives == "alt.pkl" and e.gt is None
    assert evaluate.build_parser().parse_args(["--pred_dir", "map.pkl"]).alternatives is None


def test_best_of_two_and_the_per_frame_dicts(tmp_path, capsys):
    import pickle

    import evaluate
    B, J = 3, 15
    rng = np.random.default_rng(0)
    gt = rng.normal(size=(B, J, 3))
    pred = gt + np.array([0.01, 0.2, 0.05])[:, None, None]
    runner = gt + np.array([0.5, 0.02, np.nan])[:, None, None]
    frames = [{"runner_up": np.int64(-1 if t == 2 else 4), "runner_up_joints": runner[t].astype(np.float32),
               "runner_up_margin": np.float64([3.0, 0.1, np.inf][t])} for t in range(B)]
    r = evaluate.best_of_two(frames, pred, gt)
    err = np.sqrt(3.0) * np.array([0.01, 0.2, 0.05])
    assert np.isclose(r["best_of_two_mpjpe"], np.mean([err[0], np.sqrt(3.0) * 0.02, err[2]]), rtol=1e-6)
    assert np.isclose(r["runner_up_closer_share"], 1 / 3) and r["frames_with_margin"] == 2 and r["spearman_error_margin"] == -1.0
    with open(tmp_path / "map.pkl", "wb") as f:
        pickle.dump([p.astype(np.float32) for p in pred], f)
    with open(tmp_path / "alt.pkl", "wb") as f:
        pickle.dump(frames, f)
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(gt, f)
    ev = evaluate.main(["--pred_dir", str(tmp_path / "map.pkl"), "--alternatives", str(tmp_path / "alt.pkl"), "--gt", str(tmp_path / "gt.pkl")])
    assert np.isclose(ev["alternatives"]["best_of_two_mpjpe"], r["best_of_two_mpjpe"], rtol=1e-5)
    only = evaluate.main(["--pred_dir", str(tmp_path / "map.pkl"), "--alternatives", str(tmp_path / "alt.pkl")])
    out = capsys.readouterr().out
    assert "best-of-two MPJPE" in out and "runner-up margin: mean" in out
    assert np.isclose(only["alternatives"]["mean_runner_up_margin"], 1.55) and np.isclose(only["alternatives"]["below_ln2_share"], 1 / 3)
    # the per-frame dicts of a result on the host
    keys = op.POSE_KEYS + op.ALTERNATIVES_KEYS
    result = {k: torch.zeros((2, 4)) for k in keys}
    result["solved"] = torch.tensor([True, False])
    result["max_marginals"] = torch.zeros((2, 3, 2, 2, 2))
    per = op.skeleton_alternatives_to_numpy(result)
    assert len(per) == 2 and tuple(per[0]) == keys + ("max_marginals",) and per[1]["max_marginals"].shape == (3, 2, 2, 2)
    assert per[1]["solved"] == np.False_ and per[0]["margin"].shape == (4,)
    del result["max_marginals"]
    assert tuple(op.skeleton_alternatives_to_numpy(result)[0]) == keys
