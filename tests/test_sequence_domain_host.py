"""CPU: the cases of tests/sequence_domain_cases.py are what they claim to be.  Every case is built and run through its model here and
the model's own input condition is asserted, so that a seed whose frames would not be linked, whose pose would fall back or whose edge
statistics would be invalid fails on a machine without a GPU and not on the device; the case lists reach the paths they are there for;
and the Python classes accept an odd grid.  Nothing here touches a device."""
import numpy as np
import pytest
import torch

import sequence_domain_cases as S
import volume_domain_cases as D
from sceneego_amd import _lib
from sceneego_amd.motion_fit import MotionModelFit
from sceneego_amd.skeleton_fit import SkeletonModelFit
from sceneego_amd.skeleton_pose import SkeletonPose
from sceneego_amd.volume_smoother import VolumeSmoother
from sceneego_amd.volume_viterbi import VolumeViterbi
from skeleton_pose_model import shell_max_at
from test_gpu_skeleton_fit import fit_bound, moment_bound
from test_gpu_volume_smoother import e1

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ sequences
@pytest.mark.parametrize("rows,G,R,floor,T", S.SEQUENCE_CASES + [S.SEQUENCE_ALIGN_CASE])
def test_sequence_case_meets_the_models_conditions(rows, G, R, floor, T):
    N = G ** 3
    k = S.filter_inputs(rows, G, R, T)
    b, rs = S.sequence_forward(rows, G, R, floor, T)
    assert b.dtype == np.float32 and b.shape == k["p"].shape == (T, rows, N) and rs[0].all() and not rs[1:].any()
    amin, smin = S.smoother_condition(S.smoother_want(rows, G, R, floor, T), N)
    Smin, s2 = S.stats_condition(S.stats_want(rows, G, R, floor, T), N)
    want = S.viterbi_want(rows, G, R, floor, T)
    S.viterbi_condition(want)
    bound = 2 * (T - 1) * e1(R)
    print(f"rows {rows} G {G} R {R} floor {floor}: agreement x N >= {amin:.3g}, s x N >= {smin:.3g}, S x N >= {Smin:.3g}; smoother bound of "
          f"frame 0 {bound / U:.0f} u; Viterbi exponents {want['exponent'].min()}..{want['exponent'].max()}, {int(want['jumped'].sum())} jumps")
    assert bound < 0.01 and abs(s2 - smin) <= 1e-9 * smin              # the two models walk the same backward recursion
    assert 0 <= R <= min(_lib.FILTER_MAX_RADIUS, G - 1) and 2 <= G <= _lib.FILTER_MAX_GRID


def test_sequence_cases_reach_what_they_claim():
    cases = S.SEQUENCE_CASES
    grids = {G for _, G, _, _, _ in cases}
    assert sum((G ** 3) & 3 != 0 for G in grids) >= 5, "the scalar finish passes: voxels & 3 != 0"
    assert {2, 3} <= grids and max(grids) == 127 and all(G % 2 for G in grids if G > 2)
    assert any(R == _lib.FILTER_MAX_RADIUS == G - 1 and G < 128 for _, G, R, _, _ in cases)
    assert any(R == _lib.FILTER_MAX_RADIUS and G == 127 for _, G, R, _, _ in cases)
    assert any(G < 4 and R == G - 1 for _, G, R, _, _ in cases) and any(R == 0 for _, _, R, _, _ in cases)
    assert any(floor == 0.0 for _, _, _, floor, _ in cases)
    rows, G, R, floor, T = S.SEQUENCE_ALIGN_CASE
    assert (G ** 3) & 3 == 0 and (rows * G ** 3 * 4) % 16 == 0         # the vector pass is what an offset base turns off, in every frame
    for c in S.SEQUENCE_CUT_CASES + [S.SMOOTHER_NAN_CASE, S.STATS_CUT_CASE, S.VITERBI_NAN_CASE]:
        assert c in cases and (c[1] ** 3) & 3 != 0
    assert {c[1] for c in S.SEQUENCE_CUT_CASES} == {9, 3} and S.SMOOTHER_NAN_CASE[1] == 9 and S.VITERBI_NAN_CASE[1] == 5


def test_the_jump_case_jumps_at_an_odd_grid():
    G, R, floor = S.VITERBI_JUMP_CASE
    k = S.viterbi_jump_inputs()
    m = k["m"]
    assert G == 9 and k["p"].shape == (4, 3, G ** 3) and k["p"].dtype == np.float32
    assert not m["tied"].any() and m["jumped"][2].all() and not m["jumped"][[0, 1, 3]].any() and not m["restarted"][1:].any()
    # none of the generated sequences jumps, which is why this one is constructed
    assert not any(S.viterbi_want(*c)["jumped"].any() for c in S.SEQUENCE_CASES)


def test_the_viterbi_nan_case_is_what_it_claims():
    rows, G, R, floor, T = S.VITERBI_NAN_CASE
    m = S.viterbi_nan_inputs()["m"]
    assert m["restarted"][:, 1].tolist() == [True, False, False, False]               # the NaN cell is passed over
    assert m["restarted"][:, 3].tolist() == [True, False, True, True] and m["peak"][2, 3] == -1 and m["index"][2, 3] == -1
    assert not m["tied"].any() and np.isnan(m["best"][2, 3]) and np.isnan(m["state"][1][1, 60])


def test_the_smoother_nan_case_cuts_the_chain():
    rows, G, R, floor, T = S.SMOOTHER_NAN_CASE
    from volume_filter_model import volume_filter_model
    from volume_smoother_model import volume_smoother_model
    k = S.filter_inputs(rows, G, R, T)
    p = k["p"].copy()
    p[2, 1] = np.nan
    wb, _, _, rs = volume_filter_model(p, k["c"], k["taps"], G, floor)
    assert rs[:, 1].tolist() == [True, False, True, True]
    sm = volume_smoother_model(p, wb.astype(np.float32), rs, k["c"], k["taps"], G, floor)
    assert sm["smoothed"][:, 1].tolist() == [True, False, False, False] and sm["smoothed"][:-1, [0, 2]].all()


# ------------------------------------------------------------------------------------------------------------------ skeletons
@pytest.mark.parametrize("frames,tree,G,R,floor", S.TREE_CASES)
def test_tree_case_meets_the_pose_models_condition(frames, tree, G, R, floor):
    k = S.skeleton_inputs(frames, tree, G, R)
    J = len(k["parents"])
    assert k["p"].dtype == np.float32 and k["p"].shape == (frames, J, G ** 3) and k["taps"].shape == (J, (2 * R + 1) ** 3)
    want = S.pose_want(frames, tree, G, R, floor)
    print(f"frames {frames} {tree} G {G} R {R} floor {floor}: solved {want['solved'].tolist()}, jumps {int(want['jumped'].sum())}, log score "
          f"{want['log_score'].round(3).tolist()}")
    assert want["solved"].all() and (want["index"] >= 0).all()
    assert 0 <= R <= min(_lib.SKELETON_MAX_RADIUS, G - 1) and 1 <= J <= _lib.SKELETON_MAX_JOINTS


def test_the_pose_model_mirrors_with_its_input():
    """What the GPU test's mirrored launch at two column tiles rests on.  The shell taps depend on |d| alone, so the pose model of volumes
    mirrored along k forms the same products in the same order: the same maxima, exponents and best_root bit for bit, and - unless
    two candidates tie exactly, where the lower index wins on either side - the mirrored voxels.  Checked on the model at 65^3; the pose
    of the 127^3 case lies in the first column tile (k = 45..47), its mirror image in the second."""
    frames, tree, G, R, floor = 1, "chain3", 65, 4, 1e-3
    k = S.skeleton_inputs(frames, tree, G, R)
    W = 2 * R + 1
    taps = k["taps"].reshape(-1, W, W, W)
    assert np.array_equal(taps, taps[..., ::-1])
    from skeleton_pose_model import skeleton_pose_model
    want = S.pose_want(frames, tree, G, R, floor)
    mirror = skeleton_pose_model(S.mirrored_k(k["p"], G), k["taps"], k["parents"], G, floor)
    assert np.array_equal(mirror["index"], S.mirrored_index(want["index"], G)) and np.array_equal(mirror["exponent"], want["exponent"])
    assert np.array_equal(mirror["best_root"].view(np.int32), want["best_root"].view(np.int32)) and mirror["solved"].all()
    big = S.pose_want(1, "chain3", 127, 6, 1e-3)["index"] % 127
    assert (big < 64).all() and (126 - big >= 64).all()
    t127 = S.skeleton_inputs(1, "chain3", 127, 6)["taps"].reshape(-1, 13, 13, 13)
    assert np.array_equal(t127, t127[..., ::-1])


@pytest.mark.parametrize("frames,tree,G,R,floor", S.ALTERNATIVES_CASES)
def test_tree_case_meets_the_alternatives_models_condition(frames, tree, G, R, floor):
    pose = S.pose_want(frames, tree, G, R, floor)
    for sep in S.separations(G):
        want = S.alternatives_want(frames, tree, G, R, floor, sep)
        assert want["solved"].all() and want["complete"].all(), sep
        assert np.array_equal(want["index"], pose["index"]) and np.array_equal(want["exponent"], pose["exponent"])
        if sep == G - 1:
            assert (want["alt_index"] == -1).all(), "a window over the whole grid leaves nothing"
        else:
            assert (want["alt_index"] != want["index"]).all()
            if floor > 0 and (sep == 0 or G >= 5):                        # at 3^3 a window of one voxel around the centre is the grid
                assert (want["alt_index"] >= 0).all()
    print(f"frames {frames} {tree} G {G} R {R} floor {floor}: alternatives at separation 1: "
          f"{int((S.alternatives_want(frames, tree, G, R, floor, 1)['alt_index'] >= 0).sum())} of {pose['index'].size}")


def test_the_fallback_case_falls_back():
    frames, tree, G, R, floor = S.TREE_FALLBACK_CASE
    k = S.skeleton_inputs(frames, tree, G, R)
    from skeleton_alternatives_model import skeleton_alternatives_model
    from skeleton_pose_model import skeleton_pose_model
    p = S.fallback_inputs()
    want = skeleton_pose_model(p, k["taps"], k["parents"], G, floor)
    assert want["solved"].tolist() == [False, True] and want["index"][0, 2] == -1 and (want["index"][0, :2] >= 0).all()
    clean = S.pose_want(frames, tree, G, R, floor)
    assert np.array_equal(want["index"][1], clean["index"][1])            # the NaN cell lies off the pose
    alt = skeleton_alternatives_model(p, k["taps"], k["parents"], G, floor, 1)
    assert alt["complete"].tolist() == [False, True]


@pytest.mark.parametrize("frames,tree,G,R,floor", S.EDGE_CASES)
def test_tree_case_meets_the_edge_statistics_condition(frames, tree, G, R, floor):
    k = S.skeleton_inputs(frames, tree, G, R)
    blocks = S.edge_blocks(frames, tree, G, R)
    small, s0 = S.edge_condition(S.edge_want(frames, tree, G, R, floor), blocks, G, floor)
    bound = fit_bound(k["parents"], G, R)
    print(f"frames {frames} {tree} G {G} R {R} floor {floor}: smallest normaliser {small:.3g}, smallest S0 {s0:.3g}; bound {bound / U:.0f} u")
    assert bound < 0.01
    assert floor > 0 or D.skeleton_method(G) == "direct"


def test_tree_cases_reach_what_they_claim():
    cases = S.TREE_CASES
    assert any(G % 2 and (G + 63) // 64 == 2 for _, _, G, _, _ in cases), "an odd grid across two column tiles"
    assert sum(G % 2 for _, _, G, _, _ in cases) == 6 and any(R == G - 1 for _, _, G, R, _ in cases)
    assert sum(len(S.TREES[t]) == _lib.SKELETON_MAX_JOINTS == 32 for _, t, _, _, _ in cases) == 3
    par = S.TREES["chain32"]
    depth = [0] * 32
    for j in range(1, 32):
        depth[j] = depth[par[j]] + 1
    assert max(depth) == 31
    for group in (S.ALTERNATIVES_CASES, S.EDGE_CASES):
        assert any((G + 63) // 64 == 2 and G % 2 for _, _, G, _, _ in group) and sum(len(S.TREES[t]) == 32 for _, t, _, _, _ in group) == 3
        assert all(floor > 0 for _, _, G, _, floor in group if D.skeleton_method(G) == "fft")
    assert S.EDGE_CASES == cases and (1, "chain3", 127, 6, 1e-3) in S.EDGE_CASES       # the edge statistics: every whole tree, 127^3 too
    assert max(G for _, _, G, _, _ in S.ALTERNATIVES_CASES) == 65
    assert S.TREE_BATCH_CASE in cases and S.TREE_BATCH_CASE[0] == 5 and S.TREE_ALIGN_CASE in cases and S.TREE_ALIGN_CASE[2] % 2 == 1
    assert S.TREE_FALLBACK_CASE[2] == 9 and S.TREE_FALLBACK_CASE[4] == 0.0
    # the chains behind the bounds, at the grids of the cases
    assert [_lib.MOMENT_CHAIN(G) for G in (3, 5, 9, 65, 80, 127, 128)] == [19, 19, 19, 29, 31, 50, 50]
    assert _lib.SMOOTH_CHAIN == _lib.STATS_CHAIN == 80 and _lib.SKELETON_SUM_CHAIN == 142


def test_the_stand_alone_shapes():
    assert [(G, R) for G, R in S.SHELL_FULL] == [(80, 24), (128, 20)] and S.SHELL_FULL[0][1] == _lib.SKELETON_MAX_RADIUS
    for G, R in S.SHELL_FULL:
        assert (G + 63) // 64 == 2
        v = S.full_voxels(G)
        assert np.isin(v, D.correlate_voxels(G)).sum() >= S.FULL_SAMPLE * 0.95 and v.max() == G ** 3 - 1 and v.min() == 0
        assert (v // (G * G) == G - 1).sum() >= S.FULL_SAMPLE // 3 and (v % G >= 64).sum() >= S.FULL_SAMPLE // 3
        assert np.isin([(G - 1) * G * G + 15 * G + 63, (G - 1) * G * G + 16 * G + 64], v).all()
        k = S.shell_inputs(G, R)
        lengths = k["lengths"] / (S.SIDE / G)
        assert abs(lengths.max() - (R - 1.51)) < 1e-9, "a full-length shell: the longest bone the block takes"
        nnz = np.count_nonzero(k["taps"], axis=1)
        assert nnz[0] == 0 and (nnz[1:] > 1000).all() and moment_bound(G, R) < 0.01
        assert k["e"].shape == k["m"].shape == (3, G ** 3) and (k["e"] >= 0).all() and (k["m"] >= 0).all()
    G, R, bones = S.SHELL_DEEP
    assert (np.count_nonzero(S.shell_inputs(G, R, bones)["taps"], axis=1)[1:] < 1000).all()
    assert S.SHELL_ODD[0] == 127 and S.SHELL_SMALL == (9, 8) and S.small_shell_taps().shape == (3, 17 ** 3)


def test_the_sampled_maximum_is_affordable_on_the_host():
    """One chunk of the model behind the full-length shells, so that a slower model shows here and not as a GPU test of minutes."""
    G, R = S.SHELL_FULL[0]
    k = S.shell_inputs(G, R)
    e3, arg = shell_max_at(k["a"][1], k["taps"][2], G, R, S.full_voxels(G)[:128])
    assert (e3 > 0).all() and (arg >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ the classes
def test_the_classes_accept_an_odd_grid_without_a_device():
    side, G = 2.0, 9
    coord = torch.zeros((G ** 3, 3))
    s = VolumeSmoother(coord, G, side, sigma=0.10)
    assert s.filter.grid == G and s.filter.radius == 2 and s.frames_stored == 0
    v = VolumeViterbi(coord, G, side, sigma=1.0)
    assert v.filter.radius == G - 1 and v.frames_stored == 0
    m = MotionModelFit(coord, G, side, sigma=0.10)
    assert m.frames_stored == 0
    sp = SkeletonPose(coord, G, side, [0.5, 0.3], parents=(0, 0, 1))
    assert sp.radius == int(np.ceil((0.5 + 0.09) / (side / G))) == 3 and sp.parents == (0, 0, 1)
    f = SkeletonModelFit(G, side, [0.0, 0.5, 0.3], tau=0.03, parents=(0, 0, 1))
    assert f.radius == 3 and f.frames_stored == 0
    assert VolumeSmoother(torch.zeros((27, 3)), 3, side, sigma=1.0).filter.radius == 2
