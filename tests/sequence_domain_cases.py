"""Case lists and host helpers of the sequence-domain tests (tests/test_sequence_domain_host.py on the CPU,
tests/test_gpu_sequence_domain.py on the device): the corners of the domain that include/sceneego_hip.h promises for the smoother, the
transition statistics, the Viterbi pass, the most probable pose, the runner-up poses and the edge statistics, and that the operators'
own test files never enter.  No device code.

The operators' own tests softmax on the device with se_softargmax3d_f32, which refuses voxels & 3, and copied their case lists from
the filter's and the coupling's: every grid there is even and every base a fresh allocation.  The inputs here are those of
tests/volume_domain_cases.py - softmaxed ON THE HOST (volume_filter_cases.softmax32), the same arrays in the host test and in the GPU
test, cached and shared with the filter's and the coupling's domain tests (the tuples below are theirs wherever they fit).

The forward pass behind the smoother and the statistics is se_volume_filter_f32 on the device; on the host its float64 model stands in
for it, the beliefs rounded to float32 as the kernel hands them on (tests/test_volume_smoother_host.py does the same).
"""
import functools

import numpy as np

import volume_domain_cases as D
from motion_fit_model import transition_stats_model
from sceneego_amd.skeleton_fit import cut_support, support_taps
from sceneego_amd.skeleton_prior import shell_taps
from skeleton_alternatives_model import skeleton_alternatives_model
from skeleton_fit_model import edge_stats_model
from skeleton_pose_model import skeleton_pose_model
from volume_domain_cases import TREES, filter_inputs, guarded, nan_banded, skeleton_inputs      # noqa: F401  (the tests take them from here)
from volume_filter_cases import softmax32                                        # noqa: F401  (the softmax of every input here)
from volume_smoother_model import volume_smoother_model
from volume_viterbi_model import viterbi_path, volume_viterbi_model

SIDE = D.SIDE

# ------------------------------------------------------------------------------------------------------------------ 1. sequences
# rows, G, R, floor, T: the filter's domain cases (shared, cached inputs)
SEQUENCE_CASES = [
    (2, 3, 2, 1e-3, 4),          # 27 voxels: voxels & 3 = 3, the scalar finish pass; R = G - 1; G below the four clamped rows of Viterbi
    (4, 5, 2, 0.0, 4),           # 125 voxels: voxels & 3 = 1; floor 0
    (3, 9, 3, 1e-3, 4),          # 729 voxels: voxels & 3 = 1; W = 16 lanes for 9 columns, 16 thread rows for 9 slab rows
    (2, 17, 16, 1e-3, 3),        # R = 16 = G - 1 below 128^3: the deepest padding of the Viterbi planes around the smallest plane it fits
    (1, 127, 16, 1e-3, 2),       # the largest odd grid: W = 128 lanes for 127 columns, 127^2 offset bytes behind the float slab
    (3, 2, 0, 1e-3, 3),          # the smallest grid, no taps beside the centre
    (3, 2, 1, 1e-3, 3),          # ... and R = G - 1 = 1
]
assert SEQUENCE_CASES == D.FILTER_CASES
SEQUENCE_ALIGN_CASE = D.FILTER_ALIGN_CASE    # (4, 10, 3, 1e-3, 5): 1000 voxels, voxels & 3 = 0: the vector finish pass unless a base is offset
SEQUENCE_CUT_CASES = [(3, 9, 3, 1e-3, 4), (2, 3, 2, 1e-3, 4)]
SMOOTHER_NAN_CASE = (3, 9, 3, 1e-3, 4)       # a NaN frame that cuts the chain on the scalar path
STATS_CUT_CASE = (3, 9, 3, 1e-3, 4)
VITERBI_NAN_CASE = (4, 5, 2, 0.0, 4)
VITERBI_JUMP_CASE = (9, 1, 1e-2)             # G, R, floor of the teleporting lobe: test_a_teleporting_lobe_is_reached_by_a_jump at an odd grid


@functools.lru_cache(maxsize=None)
def sequence_forward(rows, G, R, floor, T):
    """The filter's float64 model on filter_inputs, the beliefs rounded to float32: (belief [T, rows, N] float32, restarted [T, rows])."""
    wb, _, _, wr = D.filter_want(rows, G, R, floor, T)
    return wb.astype(np.float32), wr


@functools.lru_cache(maxsize=None)
def smoother_want(rows, G, R, floor, T):
    k = filter_inputs(rows, G, R, T)
    b, rs = sequence_forward(rows, G, R, floor, T)
    return volume_smoother_model(k["p"], b, rs, k["c"], k["taps"], G, floor)


def smoother_condition(want, N):
    """The asserts of test_gpu_volume_smoother.check_against_model on the model alone.  Returns the smallest agreement x N and s x N."""
    lk = want["linked"]
    assert lk[:-1].all() and not lk[-1].any() and want["smoothed"][:-1].all()
    amin, smin = float(want["agreement"][lk].min()) * N, float(want["s"][lk].min()) * N
    assert amin >= 1e-3 and smin >= 1e-3, f"agreement x N down to {amin}, s x N down to {smin}"
    return amin, smin


@functools.lru_cache(maxsize=None)
def stats_want(rows, G, R, floor, T):
    k = filter_inputs(rows, G, R, T)
    b, rs = sequence_forward(rows, G, R, floor, T)
    return transition_stats_model(k["p"], b, rs, k["taps"], G, floor)


def stats_condition(want, N):
    """The asserts of test_gpu_motion_fit.check_case on the model alone.  Returns the smallest S x N and s x N."""
    lk = want["linked"]
    assert lk[:-1].all() and not lk[-1].any()
    S, s = want["stats"][..., 0][lk] * N, want["stats"][..., 1][lk] * N
    assert (S >= 1e-3).all() and (s >= 1e-3).all(), f"S x N down to {S.min()}, s x N down to {s.min()}"
    return float(S.min()), float(s.min())


def with_path(m):
    m["index"], m["jumped"] = viterbi_path(m["back"], m["peak"], m["restarted"])
    return m


@functools.lru_cache(maxsize=None)
def viterbi_want(rows, G, R, floor, T):
    k = filter_inputs(rows, G, R, T)
    return with_path(volume_viterbi_model(k["p"], k["taps"], G, floor))


def viterbi_condition(want):
    """The asserts of test_gpu_volume_viterbi.test_against_the_model_bit_for_bit on the model alone."""
    assert not want["tied"].any(), "a frame's maximum is attained twice"
    assert want["restarted"][0].all() and not want["restarted"][1:].any() and (want["peak"] >= 0).all()
    assert (want["best"] >= 1).all() and (want["best"] < 2).all()


@functools.lru_cache(maxsize=None)
def viterbi_jump_inputs():
    """Three rows of a sharp lobe that moves one voxel, teleports across the 9^3 grid and moves one voxel again (the generator of
    tests/test_gpu_volume_viterbi.py, which softmaxes on the host already), the taps of R = 1 and the model's result."""
    from test_gpu_volume_viterbi import teleport
    from sceneego_amd.volume_filter import gaussian_taps
    G, R, floor = VITERBI_JUMP_CASE
    p = teleport(G)
    taps = gaussian_taps(R * (SIDE / G) / 3.0, R, SIDE / G)
    return {"p": p, "taps": taps, "m": with_path(volume_viterbi_model(p, taps, G, floor))}


@functools.lru_cache(maxsize=None)
def viterbi_nan_inputs():
    """VITERBI_NAN_CASE with one NaN cell in row 1 of frame 1 and a NaN frame 2 of row 3, and the model's result."""
    rows, G, R, floor, T = VITERBI_NAN_CASE
    k = filter_inputs(rows, G, R, T)
    p = k["p"].copy()
    p[1, 1, 60] = np.nan
    p[2, 3] = np.nan
    return {"p": p, "taps": k["taps"], "m": with_path(volume_viterbi_model(p, k["taps"], G, floor))}


# ------------------------------------------------------------------------------------------------------------------ 2. skeletons
# frames, tree, G, R, floor: the coupling's domain cases that a whole-tree model can afford on the host
TREE_CASES = [
    (1, "chain3", 3, 2, 1e-3),           # R = G - 1 at the smallest grid the pose generator reaches
    (1, "chain3", 5, 4, 0.0),            # R = G - 1, floor 0
    (2, "chain3", 9, 4, 0.0),            # odd G: ragged row and column tiles together
    (5, "chain3", 9, 4, 0.0),            # a group of four frames and one more
    (1, "chain3", 65, 4, 1e-3),          # ceil(G / 64) = 2: the second column tile holds one column
    (1, "chain3", 127, 6, 1e-3),         # the largest odd grid, two column tiles
    (1, "chain32", 8, 3, 1e-3),          # J = 32, depth 31: the longest walk over the levels
    (1, "heap2_32", 8, 3, 1e-3),         # J = 32, two children per joint
    (1, "heap4_32", 8, 3, 1e-3),         # J = 32, four: the general product loop
]
assert all(c in D.SKELETON_CASES or c == D.SKELETON_BATCH_CASE for c in TREE_CASES)
TREE_ALIGN_CASE = D.SKELETON_ALIGN_CASE          # (2, "chain3", 9, 4, 0.0)
TREE_BATCH_CASE = D.SKELETON_BATCH_CASE          # (5, "chain3", 9, 4, 0.0)
TREE_FALLBACK_CASE = (2, "chain3", 9, 4, 0.0)
ALTERNATIVES_CASES = [c for c in TREE_CASES if c[2] <= 65]       # the max-marginal volumes of the model: up to G = 65
# the edge statistics: every whole-tree case; the model's direct form below 64^3, its FFT form (which needs a floor) from there
EDGE_CASES = list(TREE_CASES)


def separations(G):
    """Window half-widths of the runner-up poses: none, one voxel, and one that leaves no voxel outside the window."""
    return (0, 1, G - 1)


@functools.lru_cache(maxsize=None)
def pose_want(frames, tree, G, R, floor):
    k = skeleton_inputs(frames, tree, G, R)
    return skeleton_pose_model(k["p"], k["taps"], k["parents"], G, floor)


def mirrored_k(p, G):
    """``p`` [..., G^3] mirrored along k (the fastest axis)."""
    return np.ascontiguousarray(p.reshape(p.shape[:-1] + (G, G, G))[..., ::-1]).reshape(p.shape)


def mirrored_index(index, G):
    """Flat voxel indices >= 0 mirrored along k."""
    return index - index % G + (G - 1 - index % G)


@functools.lru_cache(maxsize=None)
def alternatives_want(frames, tree, G, R, floor, separation):
    k = skeleton_inputs(frames, tree, G, R)
    return skeleton_alternatives_model(k["p"], k["taps"], k["parents"], G, floor, separation)


@functools.lru_cache(maxsize=None)
def fallback_inputs():
    """TREE_FALLBACK_CASE with a row of zeros in frame 0 (floor 0: the frame falls back) and a single NaN cell off the pose in frame 1
    (the frame stays solved)."""
    frames, tree, G, R, floor = TREE_FALLBACK_CASE
    k = skeleton_inputs(frames, tree, G, R)
    p = k["p"].copy()
    p[0, 2] = 0.0
    p[1, 1, int(np.argmin(k["p"][1, 1]))] = np.nan
    return p


@functools.lru_cache(maxsize=None)
def edge_blocks(frames, tree, G, R):
    """The three tap blocks of a case, built as test_gpu_skeleton_fit.blocks_of builds them: the first is the case's taps bit for bit."""
    k = skeleton_inputs(frames, tree, G, R)
    h = SIDE / G
    blocks = support_taps(cut_support(k["lengths"], 0.5 * h, h, R), k["lengths"], 0.5 * h)
    assert np.array_equal(blocks[0].view(np.int32), k["taps"].view(np.int32))
    return blocks


@functools.lru_cache(maxsize=None)
def edge_want(frames, tree, G, R, floor):
    k = skeleton_inputs(frames, tree, G, R)
    return edge_stats_model(k["p"], *edge_blocks(frames, tree, G, R), k["parents"], G, floor, method=D.skeleton_method(G))


def edge_condition(want, blocks, G, floor):
    """The asserts of test_gpu_skeleton_fit.compare_stats on the model alone, and that float32 can carry the sums: a term of S0 below
    2^-126 (a subnormal E(x), A(x + d) or product, each factor at most 1) is at most 2^-126, there are N nnz terms in S0 and N in a row
    sum, so all of them together stay below one rounding of the smallest sum.  Returns the smallest normaliser and the smallest S0."""
    ws, wn, wv = want
    N = G ** 3
    assert wv.all()
    small = min(float(np.nanmin(wn[:, 1:, :2])), float(wn[:, :, 2].min()))
    assert small >= 1e-12, f"a normaliser of {small}"
    assert (ws[:, 1:, :3] > 0).all() and ((ws[:, 1:, 3] > 0).all() if floor > 0 else (ws[:, 1:, 3] == 0).all())
    nnz = int(np.count_nonzero(blocks[0], axis=1).max())
    s0 = float(ws[:, 1:, 0].min())
    assert 3 * N * nnz * 2.0 ** -126 <= 2.0 ** -24 * s0 and N * 2.0 ** -126 <= 2.0 ** -24 * small, (s0, small)
    return small, s0


# ------------------------------------------------------------------------------------------------------------------ 3. stand-alone
# G, R of se_shell_maxcorr_f32 / se_shell_argmax_i32 / se_shell_moments_f32 alone, where a whole tree is too slow on the host (17 s at
# 80^3 with R = 24, 76 s at 128^3 with R = 20): full-length shells (the case's own bone lengths)
SHELL_FULL = [(80, 24), (128, 20)]
SHELL_DEEP = D.CORRELATE_DEEP                # (80, 24, (3.2, 1.6)): thin shells in the deepest tile
SHELL_ODD = (127, 4)                         # every voxel of the largest odd grid
SHELL_SMALL = D.CORRELATE_SMALL              # (9, 8): every voxel, the five rows of test_gpu_skeleton_pose.shell_rows
FULL_SAMPLE = 12288                          # voxels compared per row under a full-length shell (19,000 taps at R = 24)


def full_voxels(G):
    """The voxels compared under a full-length shell: FULL_SAMPLE of volume_domain_cases.correlate_voxels(G) - a third from the last
    plane, a third from the columns k >= 64, a third from anywhere - and the seams: the corners, k = 63 | 64 and j = 15 | 16 on the
    first and the last plane.  The direct maximum over 19,000 taps costs 0.08 ms a voxel on the host (1 s a row here): all of
    correlate_voxels(G) (110,000 voxels at 80^3, a million at 128^3) would take 9 s and 80 s a row."""
    rng = np.random.default_rng(5 + G)
    all_v = D.correlate_voxels(G)
    last = all_v[all_v // (G * G) == G - 1]
    right = all_v[all_v % G >= 64]
    third = FULL_SAMPLE // 3
    seams = [(i * G + j) * G + k for i in (0, G - 1) for j in (0, 15, 16, G - 1) for k in (0, 63, 64, G - 1)]
    return np.unique(np.concatenate([rng.choice(last, third, replace=False), rng.choice(right, third, replace=False),
                                     rng.choice(all_v, third, replace=False), seams]))


@functools.lru_cache(maxsize=None)
def shell_inputs(G, R, bones=None, tau_voxels=0.5):
    """Volumes and blocks for the stand-alone kernels at a grid of SKELETON_CASES: a [3, N] float32 (the chain3 case's three joints),
    the three tap blocks [3, (2R+1)^3] (``bones`` in voxels, default: the case's own bone lengths) and the moment pairs (e, a, tap_row):
    parent and child of the two edges, and one pair of uniform random volumes."""
    frames, tree, _, pose_r, _ = next(c for c in D.SKELETON_CASES if c[1] == "chain3" and c[2] == G and (bones is not None or c[3] == R))
    h = SIDE / G
    k = skeleton_inputs(frames, tree, G, pose_r)
    lengths = k["lengths"] if bones is None else np.concatenate([[0.0], np.asarray(bones, dtype=np.float64) * h])
    blocks = support_taps(cut_support(lengths, tau_voxels * h, h, R), lengths, tau_voxels * h)
    assert np.array_equal(blocks[0].view(np.int32), shell_taps(lengths, tau_voxels * h, h, R).view(np.int32))
    a = np.ascontiguousarray(k["p"][0])
    rng = np.random.default_rng(11 * G + R)
    u = rng.uniform(0.05, 1.0, size=(2, G ** 3)).astype(np.float32)
    return {"a": a, "blocks": blocks, "taps": blocks[0], "lengths": lengths,
            "e": np.stack([a[0], a[1], u[0]]), "m": np.stack([a[1], a[2], u[1]]), "tap_row": np.array([1, 2, 2], dtype=np.int32)}


def small_shell_taps():
    """The two shells of test_max_correlation_and_argument_at_every_voxel at SHELL_SMALL."""
    G, R = SHELL_SMALL
    h = SIDE / G
    return shell_taps([0.0, (R - 1.51) * h, min(1.6, R - 1.6) * h], 0.5 * h, h, R)
