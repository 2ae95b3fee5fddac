"""CPU: the numpy model of the most probable pose (tests/skeleton_pose_model.py) against a dense max-product over N x N transition
matrices and a brute force over all poses, the float32 definition against the float64 recursion, the tie rule, the edge cases of the
definition and what the pose is for (a true and a mirrored ghost pair of lobes).  Nothing here touches a device."""
import itertools

import numpy as np
import pytest

from sceneego_amd import _lib
from sceneego_amd.skeleton_pose import SkeletonPose
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, shell_taps
from skeleton_pose_model import dense_pose, pose_log_score, shell_max, shell_max_at, skeleton_pose_model, tap_voxel
from skeleton_prior_cases import CHAIN3, SIDE, STAR5, _bump, lengths_for, make_logits, taps_for, voxel_coord
from skeleton_prior_model import skeleton_couple_model
from volume_filter_cases import softmax32
from volume_viterbi_model import refine_model, row_max

TREE = KINEMATIC_PARENTS
TREES = {"tree15": TREE, "star5": STAR5, "chain3": CHAIN3}
SEEDS = (1, 2, 3)
FLOORS = (0.0, 1e-3)


def _case(parents, G, R, seed, frames=1):
    L = lengths_for(parents, G, R, seed)
    logits, poses = make_logits(frames, parents, L, G, seed)
    return softmax32(logits), taps_for(L, G, R), L, poses


# ------------------------------------------------------------------------------------------------------------------ 1. dense program
@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("tree", ["tree15", "star5", "chain3"])
def test_float64_model_equals_the_dense_max_product(tree, seed, floor):
    """G = 4, R = 3.  The log score to 1e-12 relative (fewer than 60 float64 roundings lie on any chain), the pose exactly; every
    choice on the pose's path is decided by a relative margin above 1e-9, asserted: no seed is left out."""
    parents, G, R = TREES[tree], 4, 3
    p, taps, _, _ = _case(parents, G, R, seed)
    want_score, want_pose, gap = dense_pose(p[0], taps, parents, G, floor)
    got = skeleton_pose_model(p, taps, parents, G, floor, dtype=np.float64)
    print(f"{tree} seed {seed} floor {floor}: log score {want_score:.12f}, margin {gap:.3g}, jumps {int(got['jumped'].sum())}")
    assert gap > 1e-9
    assert got["solved"].all() and np.array_equal(got["index"][0], want_pose)
    assert abs(got["log_score"][0] - want_score) <= 1e-12 * abs(want_score)
    assert np.isclose(pose_log_score(p[0], taps, parents, G, floor, want_pose), want_score, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------------------------ 2. brute force
@pytest.mark.parametrize("floor", FLOORS)
def test_brute_force_over_all_poses_of_a_chain(floor):
    parents, G, R = CHAIN3, 3, 2
    N = G ** 3
    p, taps, _, _ = _case(parents, G, R, seed=7)
    scores = np.array([pose_log_score(p[0], taps, parents, G, floor, x) for x in itertools.product(range(N), repeat=3)])
    assert len(scores) == 27 ** 3
    best = int(scores.argmax())
    top = np.sort(scores)[-2:]
    assert top[1] - top[0] > 1e-9                                        # one best pose
    want_pose = [best // (N * N), best // N % N, best % N]
    for dtype in (np.float64, np.float32):
        got = skeleton_pose_model(p, taps, parents, G, floor, dtype=dtype)
        assert got["solved"].all() and got["index"][0].tolist() == want_pose
        assert np.isclose(got["log_score"][0], scores[best], rtol=1e-12 if dtype is np.float64 else 1e-6, atol=0)


# ------------------------------------------------------------------------------------------------------------------ 3. float32
@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("tree", ["tree15", "star5", "chain3"])
def test_float32_pose_is_the_float64_pose(tree, seed, floor):
    parents, G, R = TREES[tree], 4, 3
    p, taps, _, _ = _case(parents, G, R, seed)
    a = skeleton_pose_model(p, taps, parents, G, floor, dtype=np.float32)
    b = skeleton_pose_model(p, taps, parents, G, floor, dtype=np.float64)
    assert a["solved"].all() and np.array_equal(a["index"], b["index"]) and np.array_equal(a["jumped"], b["jumped"])
    assert a["best_root"].dtype == np.float32 and (a["best_root"] >= 1).all() and (a["best_root"] < 2).all()
    assert np.allclose(a["log_score"], b["log_score"], rtol=1e-5, atol=0)


def test_the_gather_form_of_the_message_equals_the_whole_volume():
    G, R = 8, 3
    p, taps, _, _ = _case(CHAIN3, G, R, seed=5)
    voxels = np.arange(G ** 3)
    for j in (1, 2):
        e3, arg = shell_max(p[0, j], taps[j], G, R)
        e3_at, arg_at = shell_max_at(p[0, j], taps[j], G, R, voxels)
        assert np.array_equal(e3.view(np.int32), e3_at.view(np.int32)) and np.array_equal(arg, arg_at)


# ------------------------------------------------------------------------------------------------------------------ 4, 5. ties
def test_uniform_child_resolves_every_tie_to_the_lowest_tap_inside_the_grid():
    """A uniform child volume makes every tap of equal |d|^2 tie exactly (shell_taps gives bit-equal weights to sign flips and
    permutations of d): the predecessor is the lowest tap index inside the grid that holds the largest weight, at every voxel."""
    G, R = 6, 3
    N, W = G ** 3, 2 * R + 1
    h = SIDE / G
    taps = shell_taps([0.0, 1.4 * h], 0.5 * h, h, R)
    w3 = taps[1].reshape(W, W, W)
    assert np.array_equal(w3, w3[::-1]) and np.array_equal(w3, w3.transpose(2, 0, 1)) and np.array_equal(w3, w3[:, ::-1, ::-1])
    child = np.full(N, np.float32(1.0 / N))
    e3, arg = shell_max(child, taps[1], G, R)
    for x in range(N):
        i, j, k = x // (G * G), x // G % G, x % G
        inside = [t for t in np.flatnonzero(taps[1]) if 0 <= i + t // (W * W) - R < G and 0 <= j + t // W % W - R < G
                  and 0 <= k + t % W - R < G]
        top = max(taps[1][t] for t in inside)
        assert arg[x] == min(t for t in inside if taps[1][t] == top) and e3[x] == child[0] * top
    corners = [0, G - 1, N - 1, N - G]
    assert len({int(arg[x]) for x in corners}) > 1                       # the clipping moves the winner
    # ... and through the whole pass: the child of the pose is the lowest voxel its parent's argument names
    prob = np.stack([softmax32(make_logits(1, (0,), np.zeros(1), G, seed=2)[0])[0, 0], child])[None]
    got = skeleton_pose_model(prob, taps, (0, 0), G, 1e-3)
    x0 = int(got["index"][0, 0])
    assert got["solved"][0] and not got["jumped"].any() and got["index"][0, 1] == tap_voxel(x0, int(arg[x0]), G, R)


def test_identical_joints_leave_the_result_defined():
    parents, G, R = STAR5, 4, 3
    p, taps, _, _ = _case(parents, G, R, seed=3)
    p = p.copy()
    p[0, 2] = p[0, 1]
    taps = taps.copy()
    taps[2] = taps[1]
    a = skeleton_pose_model(p, taps, parents, G, 1e-3)
    b = skeleton_pose_model(p.copy(), taps.copy(), parents, G, 1e-3)
    assert a["solved"].all() and a["index"][0, 1] == a["index"][0, 2] and a["jumped"][0, 1] == a["jumped"][0, 2]
    assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["exponent"], b["exponent"])
    assert np.array_equal(a["m"][0][1].view(np.int32), a["m"][0][2].view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ 6. edge cases
def test_a_single_nan_cell_is_passed_over():
    G, R = 8, 3
    p, taps, _, _ = _case(CHAIN3, G, R, seed=4, frames=2)
    clean = skeleton_pose_model(p, taps, CHAIN3, G, 1e-3)
    bad = p.copy()
    cell = int(np.argmin(p[1, 2]))                                       # far from every lobe: the pose does not pass through it
    bad[1, 2, cell] = np.nan
    got = skeleton_pose_model(bad, taps, CHAIN3, G, 1e-3)
    assert got["solved"].all() and np.array_equal(got["index"], clean["index"]) and np.isfinite(got["log_score"]).all()
    assert np.isnan(got["s"][1][2][cell]) and not np.isnan(got["m"][1][2]).any()


def test_a_row_of_zeros_falls_back():
    G, R = 8, 3
    p, taps, _, _ = _case(CHAIN3, G, R, seed=4, frames=2)
    bad = p.copy()
    bad[0, 1] = 0.0
    got = skeleton_pose_model(bad, taps, CHAIN3, G, 1e-3)
    assert got["solved"].tolist() == [False, True] and np.isnan(got["log_score"][0]) and np.isnan(got["best_root"][0])
    assert got["index"][0].tolist() == [int(p[0, 0].argmax()), -1, int(p[0, 2].argmax())]
    assert not got["jumped"][0].any() and not got["exponent"][0].any()
    clean = skeleton_pose_model(p, taps, CHAIN3, G, 1e-3)
    assert np.array_equal(got["index"][1], clean["index"][1]) and got["log_score"][1] == clean["log_score"][1]


def test_floor_zero_without_mass_on_the_shell_falls_back():
    """floor = 0: the root's volume is a compact box and the child's volume is zero wherever the root's shell reaches: M_0 = 0."""
    G, R = 8, 3
    N = G ** 3
    p, taps, _, _ = _case(CHAIN3, G, R, seed=4)
    bad = p.copy()
    box = np.zeros((G, G, G), dtype=np.float32)
    box[3:5, 3:5, 3:5] = 0.125
    bad[0, 0] = box.reshape(-1)
    reach = shell_max((box.reshape(N) > 0).astype(np.float32), taps[1], G, R)[0] > 0
    assert 0 < reach.sum() < N
    bad[0, 1][reach] = 0.0
    assert (bad[0, 1] > 0).any()
    got = skeleton_pose_model(bad, taps, CHAIN3, G, 0.0)
    assert not got["solved"][0] and got["M"][0, 0] == 0.0 and got["M"][0, 1] > 0
    assert got["index"][0].tolist() == [int(row_max(bad[0, j][None])[1][0]) for j in range(3)]
    assert skeleton_pose_model(bad, taps, CHAIN3, G, 1e-3)["solved"][0]  # the floor bridges the gap: both edges of the root's child jump
    assert skeleton_pose_model(bad, taps, CHAIN3, G, 1e-3)["jumped"][0, 1]


def test_floor_one_makes_every_edge_jump():
    G, R = 4, 3
    p, taps, _, _ = _case(TREE, G, R, seed=1)
    got = skeleton_pose_model(p, taps, TREE, G, 1.0)
    assert got["solved"][0] and got["jumped"][0, 1:].all() and not got["jumped"][0, 0]
    assert got["index"][0].tolist() == p[0].argmax(axis=1).tolist()      # every joint the peak of its own volume


def test_one_joint_pose_is_the_peak():
    G = 8
    p = softmax32(make_logits(2, (0,), np.zeros(1), G, seed=3)[0])
    got = skeleton_pose_model(p, np.zeros((1, 1), dtype=np.float32), (0,), G, 0.0)
    assert got["solved"].all() and got["index"][:, 0].tolist() == p[:, 0].argmax(axis=1).tolist()
    assert np.allclose(got["log_score"], np.log(p[:, 0].max(axis=1).astype(np.float64)), rtol=1e-15)


def test_pose_validates_before_the_device():
    coord = np.zeros((8, 8, 8, 3), dtype=np.float32)
    ok = dict(coord=coord, grid=8, cuboid_side=2.0, bone_lengths=[0.5] * 14)
    s = SkeletonPose(**ok)
    assert s.radius == 3 and s.joints == 15 and s.taps.shape == (15, 343) and s.floor == 1e-3 and s.refine == 1 and s.parents == TREE
    for bad in ({"refine": 4}, {"refine": -1}, {"refine": 1.5}, {"refine": True}, {"tau": 0.0}, {"floor": 1.5}, {"bone_lengths": [0.5] * 13},
                {"parents": (0, 0, 3, 1)}, {"grid": 1}):
        with pytest.raises(ValueError):
            SkeletonPose(**{**ok, **bad})
    import torch
    with pytest.raises(ValueError):
        s.solve(torch.zeros((1, 14, 8, 8, 8)))
    with pytest.raises(ValueError):
        s.solve(torch.zeros((1, 15, 8, 8, 8)), joints=torch.zeros((2, 15, 3)))
    with pytest.raises(_lib.HipExtensionError):
        s.solve(torch.zeros((1, 15, 8, 8, 8)))                           # a CPU tensor: there is no fallback


def test_command_line_parser():
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    a = run_sequence.parse_args(base + ["--map_output", "m.pkl"])
    assert a.map and a.map_output == "m.pkl" and a.map_info_output is None and a.map_refine is None and not a.skeleton
    a = run_sequence.parse_args(base + ["--map_info_output", "i.pkl", "--map_refine", "0", "--bone_lengths", "b.npy", "--skeleton_tau", "0.05",
                                        "--skeleton_floor", "0", "--skeleton_output", "s.pkl"])
    assert a.map and a.skeleton and (a.map_refine, a.bone_lengths, a.skeleton_tau, a.skeleton_floor) == (0, "b.npy", 0.05, 0.0)
    assert not run_sequence.parse_args(base).map
    for bad in (["--map_refine", "1"], ["--map_output", "m.pkl", "--map_refine", "4"], ["--map_output", "m.pkl", "--map_refine", "-1"]):
        with pytest.raises(SystemExit):
            run_sequence.parse_args(base + bad)


# ------------------------------------------------------------------------------------------------------------------ 7. what it is for
def ghost_pair_logits(amplitude=6.0, lead=1.02):
    """16^3, chain [0, 0, 1], bones of 3.5 and 3 voxels.  The root has one lobe at (8, 7.5, 4); joints 1 and 2 have a true lobe at
    (8, 4, 4) and (8, 4, 7) and a ghost lobe mirrored 7 voxels away at (8, 11, 4) and (8, 11, 7): each pair one bone apart, both
    elbows one bone from the root.  Lobes of 0.8 voxel sigma; the true pair at ``lead`` times the logit amplitude of the ghost pair.
    Returns (logits [1, 3, 4096] float64, true [3, 3], ghost [3, 3])."""
    G = 16
    ax = np.arange(G, dtype=np.float64)
    true = np.array([[8, 7.5, 4], [8, 4, 4], [8, 4, 7]], dtype=np.float64)
    ghost = true + np.array([[0, 0, 0], [0, 7, 0], [0, 7, 0]], dtype=np.float64)
    logits = np.stack([amplitude * lead * _bump(ax, true[j], 0.8) for j in range(3)])
    for j in (1, 2):
        logits[j] += amplitude * _bump(ax, ghost[j], 0.8)
    return logits.reshape(1, 3, G ** 3), true, ghost


def test_pose_takes_one_side_where_the_marginals_hedge():
    """A true pair of lobes and a mirrored ghost pair, the true pair at 1.02x the logit amplitude.  The coupled expectations hedge
    between the sides; the pose takes both joints from one pair.  Values of the committed generator (voxels): printed below and quoted
    in the README."""
    G, R = 16, 5
    logits, true, ghost = ghost_pair_logits()
    p = softmax32(logits)
    coord = voxel_coord(G)
    L = np.array([0.0, 3.5, 3.0])
    taps = shell_taps(L, 0.5, 1.0, R)
    got = skeleton_pose_model(p, taps, CHAIN3, G, 1e-3)
    pose = coord[got["index"][0]].astype(np.float64)
    refined = refine_model(p, coord, got["index"], G, 1)[0].astype(np.float64)
    to_true, to_ghost = np.linalg.norm(pose - true, axis=1), np.linalg.norm(pose - ghost, axis=1)
    bones = np.abs(np.linalg.norm(pose[1:] - pose[[0, 1]], axis=1) - L[1:])
    bones_refined = np.abs(np.linalg.norm(refined[1:] - refined[[0, 1]], axis=1) - L[1:])
    _, cj, _, cc, _ = skeleton_couple_model(p, coord, taps, CHAIN3, G, 1e-3)
    c_true, c_ghost = np.linalg.norm(cj[0] - true, axis=1), np.linalg.norm(cj[0] - ghost, axis=1)
    c_bones = np.abs(np.linalg.norm(cj[0, 1:] - cj[0, [0, 1]], axis=1) - L[1:])
    print(f"pose: to the true lobes {to_true.round(3).tolist()}, to the ghosts {to_ghost.round(3).tolist()}, bone error "
          f"{bones.round(3).tolist()} (refined {bones_refined.round(3).tolist()}) voxels, jumped {got['jumped'][0].tolist()}")
    print(f"coupled expectations: to the true lobes {c_true.round(3).tolist()}, to the ghosts {c_ghost.round(3).tolist()}, bone error "
          f"{c_bones.round(3).tolist()} voxels")
    assert got["solved"][0] and cc[0] and not got["jumped"].any()
    side = to_true[1:] < to_ghost[1:]
    assert side[0] == side[1] and side.all()                             # both from the same pair: the stronger one
    assert (to_true < 1.0).all() and (bones < 1.0).all() and (bones_refined < 1.0).all()
    assert (c_true[1:] > 2.0).all() and (c_ghost[1:] > 2.0).all()        # the expectations lie between the lobes
    # the same with the ghost pair leading: the pose follows it, all or nothing
    flipped = skeleton_pose_model(softmax32(ghost_pair_logits(lead=1 / 1.02)[0]), taps, CHAIN3, G, 1e-3)
    fp = coord[flipped["index"][0]].astype(np.float64)
    assert (np.linalg.norm(fp - ghost, axis=1) < 1.0).all()
