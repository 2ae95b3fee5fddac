"""CPU: the cases of tests/path_sampler_domain_cases.py are what they claim to be.  Every case is built and run through its model here
and the model's own input condition is asserted, so that a change to a generator whose frames would tie, die, not be linked or never
jump fails on a machine without a GPU and cannot silently empty a GPU test; the case lists reach the paths they are there for; and
the models are held to something independent at the new shapes where that is cheap: the backward model's max-marginals to the brute
force over every trajectory at 3^3, the trajectory sampler's law to the dense transition at 3^3, the pose sampler's conditionals to the
dense edge factor at 3^3.  Nothing here touches a device."""
import numpy as np
import pytest

import path_sampler_domain_cases as C
import sequence_domain_cases as S
from sceneego_amd import _lib
from skeleton_sampler_model import FRESH, JUMP, STEP
from test_skeleton_sampler_host import law_error
from test_volume_sampler_host import conditional_law_error
from volume_viterbi_alternatives_model import backward_model, brute_force_max_marginals
from volume_viterbi_model import JUMP as JUMP_BIT, viterbi_path, volume_viterbi_model


# ------------------------------------------------------------------------------------------------------------------ runner-up trajectories
@pytest.mark.parametrize("rows,G,R,floor,T", C.SEQUENCE_CASES + [C.SEQUENCE_ALIGN_CASE])
def test_sequence_case_meets_the_backward_models_condition(rows, G, R, floor, T):
    f, b = C.alternatives_want(rows, G, R, floor, T)
    C.alternatives_condition(f, b)
    mm = b["mm"]
    fin = np.isfinite(b["margin"])
    print(f"rows {rows} G {G} R {R} floor {floor}: max-marginals down to {mm[mm > 0].min():.3g}, {int((mm == 0).sum())} exact zeros; "
          f"margins {b['margin'][fin].min() if fin.any() else float('nan'):.3f}..{b['margin'][fin].max() if fin.any() else float('nan'):.3f}, "
          f"{int((b['alt_index'] < 0).sum())} frames without an alternative, {int((b['anchor'] >= 0).sum())} anchors")
    assert b["mm"].dtype == np.float32 and b["succ"].shape == (T, rows, G ** 3)
    if G > C.SEP + 1 + 2:                                       # a window of 5 voxels leaves something of the grid
        assert (b["alt_index"] >= 0).any() and (b["anchor"] >= 0).any() and (b["runner_up_index"] >= 0).any()


@pytest.mark.parametrize("G", C.ALTERNATIVES_SEPARATION_GRIDS)
def test_separations_at_odd_grids(G):
    rows, _, R, floor, T = C.case_of(G)
    for sep in (0, G - 1, G + 5):
        f, b = C.alternatives_want(rows, G, R, floor, T, sep)
        C.alternatives_condition(f, b)
        if sep == 0:
            assert (b["alt_index"] >= 0).all() and (b["alt_index"] != f["index"]).all()
        else:
            assert (b["alt_index"] == -1).all() and np.isnan(b["alt_value"]).all() and (b["margin"] == np.inf).all()
            assert (b["anchor"] == -1).all() and np.isfinite(b["path_value"]).all()


def test_the_backward_models_max_marginals_equal_the_brute_force_at_the_smallest_odd_grid():
    """The first three frames of both rows of the 3^3 case, float64: every mm_t(x) against the maximum over all 27^3 trajectories that
    are at x in frame t, to 1e-12 relative (test_volume_path_alternatives_host.py does it on inputs of its own at T = 4)."""
    rows, G, R, floor, T = C.case_of(3)
    k = C.filter_inputs(rows, G, R, T)
    for row in range(rows):
        p = np.ascontiguousarray(k["p"][:3, row:row + 1])
        f = volume_viterbi_model(p, k["taps"], G, floor, dtype=np.float64)
        f["index"], f["jumped"] = viterbi_path(f["back"], f["peak"], f["restarted"])
        b = backward_model(p, f, f["index"], k["taps"], G, floor, 0, dtype=np.float64)
        want, _, _ = brute_force_max_marginals(p[:, 0], k["taps"], G, floor)
        got = b["mm"][:, 0] / b["mm"][:, 0].max(axis=1, keepdims=True)
        want = want / want.max(axis=1, keepdims=True)
        err = np.abs(got - want) / np.where(want > 0, want, 1.0)
        assert (got[want == 0] == 0).all() and err.max() <= 1e-12 and b["complete"].all(), (row, err.max())


def test_the_jump_nan_and_death_cases_are_what_they_claim():
    k, b = C.alternatives_jump_want()
    f = k["m"]
    jump_bits = int(((b["succ"] >= 0) & ((b["succ"] & JUMP_BIT) != 0)).sum())
    assert S.VITERBI_JUMP_CASE[0] == 9 and not f["tied"].any() and not b["tied"].any() and b["complete"].all()
    assert jump_bits > 0 and b["runner_up_jumped"].any() and f["jumped"][2].all()
    n = C.alternatives_nan_inputs()
    f, b = n["f"], n["b"]
    assert f["restarted"][:, 0].tolist() == [True, False, False, False]                # the NaN cell is passed over
    assert f["restarted"][:, 1].tolist() == [True, False, True, True] and f["index"][2, 1] == -1
    assert b["linked"][:, 1].tolist() == [True, False, False, False] and b["linked"][:, 0].tolist() == [True, True, True, False]
    assert not f["tied"].any() and not b["tied"].any() and b["complete"].all()
    assert np.isnan(b["mm"][1, 0, 400]) and np.isnan(b["mm"][2, 1]).all() and (b["succ"][1:, 1] == -1).all()
    assert (b["anchor"][:, 1] >= 0).sum() == 2 and b["runner_up_index"][2, 1] == -1      # the segments [0, 1] and [3]; frame 2 has none
    d = C.alternatives_death_inputs()
    b = d["b"]
    assert d["G"] == 9 and (d["G"] ** 3) % 256 != 0
    assert b["death"].T.tolist() == [[False, True, False, False], [False] * 4] and b["complete"].T.tolist() == [[0, 0, 1, 1], [1] * 4]
    assert np.isnan(b["mm"][1, 0]).all() and (b["succ"][1, 0] == -1).all() and np.isnan(b["path_value"][1, 0])


# ------------------------------------------------------------------------------------------------------------------ trajectory samples
@pytest.mark.parametrize("rows,G,R,floor,T", C.SAMPLER_CASES + [C.SEQUENCE_ALIGN_CASE])
def test_sequence_case_meets_the_sampler_models_condition(rows, G, R, floor, T):
    b, rs = S.sequence_forward(rows, G, R, floor, T)
    assert np.isfinite(b).all() and rs[0].all() and not rs[1:].any()
    want = C.sampler_want(rows, G, R, floor, T)
    kinds = C.sampler_condition(want, floor)
    assert want["index"].shape == (C.samples_for(floor), T, rows) and (want["index"] < G ** 3).all()
    assert np.array_equal(want["next"], want["index"][:, 0])
    print(f"rows {rows} G {G} R {R} floor {floor}: {want['index'].size} draws, kinds of the linked frames {sorted(kinds)}")


def test_sampler_cases_reach_what_they_claim():
    assert C.SEQUENCE_CASES == S.SEQUENCE_CASES and len(C.SEQUENCE_CASES) == 7 and C.SEQUENCE_ALIGN_CASE == (4, 10, 3, 1e-3, 5)
    assert {c[1] for c in C.SEQUENCE_CASES} == {2, 3, 5, 9, 17, 127}
    assert [c[:3] for c in C.SAMPLER_JUMP_CASES] == [(3, 9, 3), (2, 3, 2), (2, 17, 16)] and all(c[3] == 0.3 for c in C.SAMPLER_JUMP_CASES)
    for c in C.SAMPLER_JUMP_CASES:                              # steps, jumps and fresh draws all occur in each
        assert set(np.unique(C.sampler_want(*c)["kind"]).tolist()) == {STEP, JUMP, FRESH}
    # at the floor of the other cases with 8 samples no jump is drawn: that is why the three above are there
    assert not any((C.sampler_want(*c)["kind"] == JUMP).any() for c in C.SEQUENCE_CASES if c[1] in (3, 9, 17))
    for G in C.ALTERNATIVES_ALIAS_GRIDS + C.ALTERNATIVES_CUT_GRIDS + C.ALTERNATIVES_SEPARATION_GRIDS:
        assert G % 2 == 1 and C.case_of(G)[1] == G
    # vb_update_kernel: the further rows of a thread are all clamped where RP = 256 / W >= G; ragged last turns at 17 and 127
    shape = {G: (1 << max(G - 1, 1).bit_length()) for G in (2, 3, 5, 9, 17, 127)}
    assert all(256 // shape[G] >= G for G in (2, 3, 5, 9)) and 256 // shape[17] == 8 and 256 // shape[127] == 2
    assert C.SAMPLER_CUT_CASE in C.SAMPLER_CASES and C.SAMPLER_NAN_CASE in C.SAMPLER_CASES and C.SAMPLER_NAN_CASE[1] == 5
    assert C.LONG_FRAMES == 65537 > 65535 and C.LONG_SPLIT <= 65535 and C.LONG_FRAMES - C.LONG_SPLIT <= 65535
    assert _lib.FILTER_MAX_RADIUS == 16 and _lib.FILTER_MAX_GRID == 128


@pytest.mark.parametrize("floor", (1e-3, C.JUMP_FLOOR))
def test_the_trajectory_samplers_law_equals_the_dense_transition_at_the_smallest_odd_grid(floor):
    """No sampling noise: at 3^3 with R = 2 = G - 1, for every frame, row and y, the 27 probabilities the model's own masses imply
    against b_t(x) D[x, y] normalised, D from blur3 itself (test_volume_sampler_host.py: at 4^3), to that file's 1e-12 of the peak."""
    rows, G, R, _, T = C.case_of(3)
    k = C.filter_inputs(rows, G, R, T)
    b, _ = S.sequence_forward(rows, G, R, floor, T)
    worst = max(conditional_law_error(b[t, row], k["taps"], floor, G) for t in range(T) for row in range(rows))
    print(f"G 3 floor {floor}: conditional law against the dense matrix, worst {worst:.3e} of the peak")
    assert worst <= 1e-12


def test_the_long_track():
    k = C.long_track_inputs()
    assert k["b"].shape == (C.LONG_FRAMES, 1, 8) and k["b"].dtype == np.float32 and k["rs"].sum() == 1 and k["rs"][0, 0] == 1
    tail = C.long_track_tail()
    assert tail["index"].shape == (2, C.LONG_TAIL, 1) and (tail["index"] >= 0).all() and (tail["index"] < 8).all()
    assert (tail["kind"][:, -1] == FRESH).all() and (tail["kind"][:, :-1] != FRESH).all()


# ------------------------------------------------------------------------------------------------------------------ pose samples
@pytest.mark.parametrize("frames,tree,G,R,floor", C.UPWARD_MODEL_CASES)
def test_skeleton_case_meets_the_sampler_models_conditions(frames, tree, G, R, floor):
    k = C.skeleton_inputs(frames, tree, G, R)
    J = len(k["parents"])
    A, s, valid = C.upward_want(frames, tree, G, R, floor)
    small = C.upward_condition(s, valid)
    want = C.pose_want(frames, tree, G, R, floor)
    kinds = C.pose_condition(want, G)
    assert want["index"].shape == (C.POSE_SAMPLES, frames, J) and A.shape == (frames, J, G ** 3)
    print(f"frames {frames} {tree} G {G} R {R} floor {floor}: smallest normaliser {small:.3g}; kinds below the root {sorted(kinds)}")
    assert 0 <= R <= min(_lib.SKELETON_MAX_RADIUS, G - 1) and 1 <= J <= _lib.SKELETON_MAX_JOINTS


def test_skeleton_cases_reach_what_they_claim():
    assert C.SKELETON_CASES == C.D.SKELETON_CASES and len(C.SKELETON_JUMP_CASES) == 7
    assert [(c[2], c[3]) for c in C.SKELETON_CASES if c[1] == "chain3"] == [(3, 2), (5, 4), (7, 3), (9, 4), (65, 4), (80, 24), (127, 6), (128, 20)]
    assert sorted(c[1] for c in C.SKELETON_JUMP_CASES if c[2] == 8) == ["chain32", "heap2_32", "heap4_32"]
    assert sum(c[2] == 127 for c in C.UPWARD_MODEL_CASES) == 1, "at 127^3 one floor only"
    assert any(R == _lib.SKELETON_MAX_RADIUS == 24 for _, _, _, R, _ in C.UPWARD_LIBRARY_CASES)
    assert all(c in C.UPWARD_MODEL_CASES or c in C.UPWARD_LIBRARY_CASES for c in C.SKELETON_CASES)
    assert sum(len(C.TREES[c[1]]) == 32 for c in C.UPWARD_LIBRARY_CASES) == 3
    assert any((2 * R + 1) ** 2 > 6 * 256 and G == 128 for _, _, G, R, _ in C.UPWARD_LIBRARY_CASES)
    # at the floor of the jump cases both branches occur in the set as a whole
    kinds = np.concatenate([C.pose_want(*c)["kind"][:, :, 1:].reshape(-1) for c in C.SKELETON_JUMP_CASES])
    assert (kinds == STEP).any() and (kinds == JUMP).any()
    assert C.SKELETON_BATCH_CASE[0] == 5 and C.SKELETON_BATCH_CASE[2] == 9 and C.SKELETON_ALIGN_CASE[2] == 9
    assert _lib.SKELETON_SUM_CHAIN == 142


@pytest.mark.parametrize("floor", (1e-3, C.JUMP_FLOOR))
def test_the_pose_samplers_conditionals_equal_the_dense_edge_factor_at_the_smallest_odd_grid(floor):
    """No sampling noise: chain3 at 3^3 with R = 2 = G - 1 (27 voxels where test_skeleton_sampler_host.py has 64): for both edges and
    every parent voxel the 27 probabilities the model's own masses imply against A_c(y) F_c(x, y) normalised, and the root's against
    A_0 normalised, to that file's 1e-12 of the peak."""
    frames, tree, G, R, _ = C.SKELETON_CASES[0]
    assert (tree, G, R) == ("chain3", 3, 2)
    k = C.skeleton_inputs(frames, tree, G, R)
    A64, s, valid = C.upward_want(frames, tree, G, R, floor)
    C.upward_condition(s, valid)
    case = {"A64": A64, "A": A64.astype(np.float32), "J": len(k["parents"]), "w": k["taps"]}
    worst = law_error(case, floor, k["taps"], G=G, R=R)
    print(f"chain3 G 3 floor {floor}: worst {worst:.3e} of the peak")
    assert worst <= 1e-12


def test_the_long_pose_sequence():
    k = C.long_pose_inputs()
    assert k["A"].shape == (C.LONG_FRAMES, 3, 8) and k["A"].dtype == np.float32 and k["taps"].shape == (3, 27)
    tail = C.long_pose_tail()
    assert tail["index"].shape == (2, C.LONG_TAIL, 3) and (tail["index"] >= 0).all() and (tail["kind"][:, :, 0] == FRESH).all()
    assert (tail["kind"][:, :, 1:] != FRESH).all()
