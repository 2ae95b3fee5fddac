"""Case lists and host helpers of the path-and-sampler domain tests (tests/test_path_sampler_domain_host.py on the CPU,
tests/test_gpu_path_sampler_domain.py on the device): the corners of the domain that include/sceneego_hip.h promises for the runner-up
trajectories (se_volume_viterbi_keep_f32, se_volume_viterbi_back_f32, se_volume_viterbi_branch_i32), the trajectory samples
(se_volume_sample_f32) and the pose samples (se_skeleton_upward_f32, se_skeleton_sample_f32), and that the operators' own test files
never enter.  No device code.

The three operators were merged after tests/sequence_domain_cases.py and have the gap that file closed for their elders: their own tests
softmax on the device with se_softargmax3d_f32, which refuses voxels & 3, so every grid there is even and every base a fresh
allocation.  The inputs here are those of tests/volume_domain_cases.py - softmaxed ON THE HOST, cached, the same arrays in the host
test and in the GPU test - and the tuples are those of the two earlier case files wherever they fit.

The forward pass behind the trajectory sampler is se_volume_filter_f32 on the device; on the host its float64 model stands in for it,
the beliefs rounded to float32 (sequence_domain_cases.sequence_forward).  The upward products behind the pose sampler are
se_skeleton_upward_f32's on the device; on the host the float64 recursion rounded to float32 (tests/test_skeleton_sampler_host.py does
the same).
"""
import functools

import numpy as np

import sequence_domain_cases as S
import volume_domain_cases as D
from skeleton_sampler_model import FRESH, JUMP, STEP, skeleton_sample_model, upward_model
from volume_domain_cases import TREES, filter_inputs, guarded, nan_banded, skeleton_inputs      # noqa: F401  (the tests take them from here)
from volume_sampler_model import volume_sampler_model
from volume_viterbi_alternatives_model import backward_model, branch_walk, margins, runner_up_anchors

SIDE = D.SIDE
SEP = 2                                      # the separation of the runner-up's window, as tests/test_gpu_volume_path_alternatives.py
JUMP_FLOOR = 0.3                             # the floor at which the samplers really jump

# ------------------------------------------------------------------------------------------------------------------ 1. sequences
# rows, G, R, floor, T: the filter's domain cases (shared, cached inputs).  What they are there for in vb_update_kernel (W the power of
# two >= G, RP = 256 / W thread rows, a thread owns the rows ir, ir + RP, ir + 2 RP, ir + 3 RP of a turn):
#   G = 2, 3, 5, 9   RP = 128 .. 16 >= G: all three further rows of every thread are clamped to G - 1 and discarded
#   G = 17, R = 16   RP = 8: the last turn of a thread is ragged; the zero padding (16 rows on either side) is as deep as the plane
#   G = 127, R = 16  W = 128, RP = 2: the thread rows 121, 123, 125, (127) - the fourth row of the last turn is clamped
SEQUENCE_CASES = list(S.SEQUENCE_CASES)
SEQUENCE_ALIGN_CASE = S.SEQUENCE_ALIGN_CASE          # (4, 10, 3, 1e-3, 5)
# the trajectory sampler: the same inputs at a floor at which jumps are drawn (at 1e-3 with 8 samples none is)
SAMPLER_JUMP_CASES = [(3, 9, 3, JUMP_FLOOR, 4), (2, 3, 2, JUMP_FLOOR, 4), (2, 17, 16, JUMP_FLOOR, 3)]
assert all((r, g, rad, 1e-3, t) in SEQUENCE_CASES for r, g, rad, _, t in SAMPLER_JUMP_CASES)
SAMPLER_CASES = SEQUENCE_CASES + SAMPLER_JUMP_CASES
SAMPLES = 8                                  # per row; 16 at JUMP_FLOOR
SAMPLER_SEED = 0

ALTERNATIVES_SEPARATION_GRIDS = (9, 3)       # separation 0, G - 1 and G + 5: a window that leaves nothing on an odd grid
ALTERNATIVES_ALIAS_GRIDS = (3, 5, 9, 127)    # succ written over scores: the clamped-row shapes
ALTERNATIVES_CUT_GRIDS = (9, 17)
ALTERNATIVES_NAN_CASE = (3, 9, 3, 1e-3, 4)
SAMPLER_CUT_CASE = (3, 9, 3, JUMP_FLOOR, 4)
SAMPLER_NAN_CASE = (4, 5, 2, 0.0, 4)
LONG_FRAMES = 65537                          # one more than two turns of grid.z = 65535 start at: frames 0, 1 take a second turn
LONG_SPLIT = 32768                           # 32768 + 32769: each call's sums launch stays within grid.z
LONG_TAIL = 8                                # the frames held to the model: the chain starts at the last one


def case_of(G, cases=None):
    """The first sequence case at grid ``G``."""
    return next(c for c in (SEQUENCE_CASES if cases is None else cases) if c[1] == G)


def samples_for(floor):
    return 16 if floor == JUMP_FLOOR else SAMPLES


def runner_up(p, f, taps, G, floor, separation=SEP):
    """The backward model on the forward model ``f`` (with its path), the margins, the anchors and the runner-up's walk: what
    test_gpu_volume_path_alternatives.model_of returns second."""
    b = backward_model(p, f, f["index"], taps, G, floor, separation)
    b["margin"] = margins(b["path_value"], b["alt_value"], b["alt_index"], f["index"])
    b["anchor"], b["runner_up_margin"] = runner_up_anchors(b["margin"], b["alt_index"], f["restarted"])
    b["runner_up_index"], b["runner_up_jumped"] = branch_walk(f["back"], b["succ"], f["restarted"], b["anchor"])
    return b


@functools.lru_cache(maxsize=None)
def alternatives_want(rows, G, R, floor, T, separation=SEP):
    """(forward model with its path, backward model with margins, anchors and the runner-up) of a sequence case."""
    k = filter_inputs(rows, G, R, T)
    f = S.viterbi_want(rows, G, R, floor, T)
    return f, runner_up(k["p"], f, k["taps"], G, floor, separation)


def alternatives_condition(f, b):
    """The asserts of test_gpu_volume_path_alternatives.test_against_the_model_bit_for_bit on the models alone: no gated maximum is
    attained twice, no backward death, only the last frame unlinked."""
    assert not f["tied"].any() and not b["tied"].any(), "a gated maximum is attained twice"
    assert b["complete"].all() and not b["death"].any()
    assert b["linked"][:-1].all() and not b["linked"][-1].any()


@functools.lru_cache(maxsize=None)
def alternatives_jump_want():
    """The teleporting lobe of sequence_domain_cases.viterbi_jump_inputs (G = 9, R = 1, floor 1e-2) through the backward model."""
    G, R, floor = S.VITERBI_JUMP_CASE
    k = S.viterbi_jump_inputs()
    return k, runner_up(k["p"], k["m"], k["taps"], G, floor)


@functools.lru_cache(maxsize=None)
def alternatives_nan_inputs():
    """ALTERNATIVES_NAN_CASE with one NaN cell in row 0 of frame 1 and a NaN frame 2 of row 1, and both models' results."""
    from volume_viterbi_model import volume_viterbi_model
    rows, G, R, floor, T = ALTERNATIVES_NAN_CASE
    k = filter_inputs(rows, G, R, T)
    p = k["p"].copy()
    p[1, 0, 400] = np.nan
    p[2, 1] = np.nan
    f = S.with_path(volume_viterbi_model(p, k["taps"], G, floor))
    return {"p": p, "taps": k["taps"], "f": f, "b": runner_up(p, f, k["taps"], G, floor)}


@functools.lru_cache(maxsize=None)
def alternatives_death_inputs():
    """The construction of test_a_backward_death_is_reported_by_complete on 9^3: frame 1 of row 0 holds one cell, the smallest
    denormal, which the backward product with a tap of 0.25 rounds to zero; row 1 lives.  729 voxels: vb_fold_kernel's fill loop runs
    over a voxel count that is no multiple of 256, with `chunks` workgroups."""
    from volume_viterbi_model import volume_viterbi_model
    G, R, floor, T = 9, 1, 0.0, 4
    taps = np.array([0.25, 1.0, 0.25], dtype=np.float32)
    at = lambda i, j, k: (i * G + j) * G + k                           # noqa: E731
    p = np.zeros((T, 2, G ** 3), dtype=np.float32)
    for r in range(2):
        p[0, r, at(7, 8, 7)], p[2, r, at(7, 8, 8)], p[3, r, at(7, 8, 8)] = 1.0, 1.0, 0.5     # the last row, the last column
    p[1, 0, at(7, 8, 7)], p[1, 1, at(7, 8, 7)] = np.float32(1e-45), 0.5
    f = S.with_path(volume_viterbi_model(p, taps, G, floor))
    return {"p": p, "taps": taps, "G": G, "R": R, "floor": floor, "f": f, "b": runner_up(p, f, taps, G, floor, 0)}


# ------------------------------------------------------------------------------------------------------------------ 2. trajectory samples
@functools.lru_cache(maxsize=None)
def sampler_want(rows, G, R, floor, T):
    """volume_sampler_model on the host's forward pass (the float64 filter model rounded to float32)."""
    k = filter_inputs(rows, G, R, T)
    b, rs = S.sequence_forward(rows, G, R, floor, T)
    return volume_sampler_model(b, rs, k["taps"], G, floor, samples_for(floor), seed=SAMPLER_SEED)


def sampler_condition(want, floor):
    """On the model alone: no invalid draw, every frame but the last is linked (kind 2 in the last frame only), and at JUMP_FLOOR steps
    and jumps both occur.  Returns the kinds of the linked frames."""
    index, kind = want["index"], want["kind"]
    assert (index >= 0).all(), "an invalid draw"
    assert (kind[:, -1] == FRESH).all() and (kind[:, :-1] != FRESH).all(), "a frame that is not linked"
    kinds = set(np.unique(kind[:, :-1]).tolist())
    assert kinds <= {STEP, JUMP} and (floor != JUMP_FLOOR or kinds == {STEP, JUMP}), kinds
    assert floor != 0.0 or kinds == {STEP}
    return kinds


@functools.lru_cache(maxsize=None)
def long_track_inputs():
    """LONG_FRAMES frames of one row at G = 2, R = 1: random normalised float32 beliefs [65537, 1, 8], restarted set in frame 0 alone,
    the taps (0.25, 0.5, 0.25).  2 MB."""
    b = np.random.default_rng(65537).random((LONG_FRAMES, 1, 8))
    rs = np.zeros((LONG_FRAMES, 1), dtype=np.int32)
    rs[0] = 1
    return {"b": (b / b.sum(axis=2, keepdims=True)).astype(np.float32), "rs": rs, "taps": np.array([0.25, 0.5, 0.25], dtype=np.float32),
            "G": 2, "R": 1, "floor": JUMP_FLOOR, "samples": 2, "seed": 3}


@functools.lru_cache(maxsize=None)
def long_track_tail():
    """The model on the last LONG_TAIL frames alone with first_frame = LONG_FRAMES - LONG_TAIL: the chain starts at the last frame, so
    the slice is self-contained."""
    k = long_track_inputs()
    t0 = LONG_FRAMES - LONG_TAIL
    return volume_sampler_model(k["b"][t0:], k["rs"][t0:], k["taps"], k["G"], k["floor"], k["samples"], seed=k["seed"], first_frame=t0)


# ------------------------------------------------------------------------------------------------------------------ 3. pose samples
# frames, tree, G, R, floor: the coupling's domain cases.  What they are there for in sks_walk_kernel:
#   (80, 24)     windows of up to 49^2 rows: the full r[SKS_WIN * SKS_WIN]
#   (128, 20)    41^2 = 1681 rows: no ni * nj loop of an unclipped window finishes in one turn of 256 threads
#   chain32      pose[] in LDS across 31 dependent joints;  heap4_32: four children read one parent's voxel
SKELETON_CASES = list(D.SKELETON_CASES)
SMALL_SKELETON_CASES = [c for c in SKELETON_CASES if c[2] <= 9]        # G <= 9 and the three J = 32 trees (G = 8)
assert len(SMALL_SKELETON_CASES) == 7 and sum(len(TREES[c[1]]) == 32 for c in SMALL_SKELETON_CASES) == 3
SKELETON_JUMP_CASES = [(f, t, G, R, JUMP_FLOOR) for f, t, G, R, _ in SMALL_SKELETON_CASES]
SKELETON_DRAW_CASES = SKELETON_CASES + SKELETON_JUMP_CASES
# the cases whose direct upward model (corr_direct) is affordable on the host: G <= 65, the J = 32 trees and (127, 6) - 6 s, one floor
UPWARD_MODEL_CASES = [c for c in SKELETON_DRAW_CASES if c[2] <= 65 or (c[2], c[3]) == (127, 6)]
UPWARD_LIBRARY_CASES = [c for c in SKELETON_CASES if c not in UPWARD_MODEL_CASES]        # (80, 24) and (128, 20)
assert [(c[2], c[3]) for c in UPWARD_LIBRARY_CASES] == [(80, 24), (128, 20)]
# ... and the three J = 32 trees as well: on a chain of depth 31 the absolute (underflow) term of the derived bound compounds by 1 / s_c
# per level and holds nothing near the root (1e20 at chain32), so those sums are also tied, bit for bit, to the coupling's own, which
# tests/test_gpu_volume_domain.py holds to float64
UPWARD_LIBRARY_CASES += [c for c in SKELETON_CASES if len(TREES[c[1]]) == 32]
SKELETON_BATCH_CASE = (5, "chain3", 9, 4, 0.0)
SKELETON_ALIGN_CASE = D.SKELETON_ALIGN_CASE          # (2, "chain3", 9, 4, 0.0)
SKELETON_HOLE_CASE = (5, "chain3", 9, 4, 0.0)        # its frames 0..2, the middle one with valid = 0
POSE_SAMPLES = 8


def pose_seed(tree, G, R):
    return D.skeleton_seed(tree, G, R)


@functools.lru_cache(maxsize=None)
def upward_want(frames, tree, G, R, floor):
    """upward_model on skeleton_inputs: (A [F, J, N] float64, s [F, J], valid [F])."""
    k = skeleton_inputs(frames, tree, G, R)
    return upward_model(k["p"], k["taps"], k["parents"], G, floor)


@functools.lru_cache(maxsize=None)
def pose_want(frames, tree, G, R, floor):
    """skeleton_sample_model on the host's upward products rounded to float32 (what the sampler takes)."""
    k = skeleton_inputs(frames, tree, G, R)
    A, _, valid = upward_want(frames, tree, G, R, floor)
    return skeleton_sample_model(A.astype(np.float32), valid.astype(np.int32), k["taps"], k["parents"], G, R, floor, POSE_SAMPLES,
                                 seed=pose_seed(tree, G, R))


def upward_condition(s, valid):
    """Every s_j >= 1e-12 and every frame valid.  Returns the smallest normaliser."""
    small = float(np.min(s))
    assert np.asarray(valid).all() and small >= 1e-12, f"a normaliser of {small}"
    return small


def pose_condition(want, G):
    """On the draws alone: every index inside the grid, the root a fresh draw, every other joint linked.  Returns the kinds of the
    joints below the root."""
    index, kind = want["index"], want["kind"]
    assert (index >= 0).all() and (index < G ** 3).all(), "an invalid draw"
    assert (kind[:, :, 0] == FRESH).all() and (kind[:, :, 1:] != FRESH).all(), "a joint that is not linked"
    kinds = set(np.unique(kind[:, :, 1:]).tolist())
    assert kinds <= {STEP, JUMP}
    return kinds


def hand_made_taps(J, R, seed):
    """The dense random blocks of test_gpu_skeleton_sampler.dense_taps (its test_draws_on_hand_made_upward_arrays), from the same
    function."""
    from test_gpu_skeleton_sampler import dense_taps
    return dense_taps(J, R, seed)


@functools.lru_cache(maxsize=None)
def long_pose_inputs():
    """LONG_FRAMES frames of chain3 at G = 2, R = 1: hand-made upward products [65537, 3, 8] as
    test_draws_on_hand_made_upward_arrays makes them, dense taps.  6 MB."""
    A = (np.random.default_rng(65538).random((LONG_FRAMES, 3, 8)) ** 2).astype(np.float32)
    return {"A": A, "taps": hand_made_taps(3, 1, 6), "parents": TREES["chain3"], "G": 2, "R": 1, "floor": JUMP_FLOOR, "samples": 2,
            "seed": 5}


@functools.lru_cache(maxsize=None)
def long_pose_tail():
    k = long_pose_inputs()
    t0 = LONG_FRAMES - LONG_TAIL
    return skeleton_sample_model(k["A"][t0:], None, k["taps"], k["parents"], k["G"], k["R"], k["floor"], k["samples"], seed=k["seed"],
                                 first_frame=t0)
