"""CPU: the numpy model of the pose sampler (tests/skeleton_sampler_model.py) draws from the law it claims to: every conditional equals
the dense edge factor's, the product of the conditionals is the brute-force posterior over whole poses and its marginals are the
coupling's beliefs, the sample frequencies agree with those beliefs and with the pairwise posterior, the results do not depend on how
the work is cut, the edge rules hold, and the Python surface refuses bad arguments before anything touches a device."""
import functools

import numpy as np
import pytest
import torch

from sceneego_amd import _lib, metrics
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, SkeletonPrior
from skeleton_prior_cases import CHAIN3, STAR5, lengths_for, make_logits, taps_for, voxel_coord
from skeleton_prior_model import skeleton_couple_model
from skeleton_sampler_model import (FRESH, JUMP, STEP, Volume, conditional_masses, edge_factor, skeleton_sample_model, upward_model,
                                    window)
from volume_filter_cases import softmax32

G, R, S = 4, 3, 4096
N = G ** 3
FLOORS = (0.0, 1e-3, 0.3)
FREQ_SCALE = 2.0          # the logits of the frequency test (its docstring says why)
TREES = {"chain3": CHAIN3, "star5": STAR5, "tree15": KINEMATIC_PARENTS}


def asymmetric_taps(J, R, seed, zeros=0.0):
    """Blocks with w(d) != w(-d): random positive taps (a share ``zeros`` of them exactly 0), each block normalised; block 0 is zero."""
    rng = np.random.default_rng(seed)
    w = rng.random((J, (2 * R + 1) ** 3)) + 0.05
    w *= rng.random(w.shape) >= zeros
    w[0] = 0.0
    w[1:] /= w[1:].sum(axis=1, keepdims=True)
    return w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(tree, floor, asym=False, frames=1, scale=1.0):
    """One tree at G = 4, R = 3 (every window is clipped): the volumes, the taps, the exact upward products and what the sampler takes,
    those products rounded to float32.  ``scale`` multiplies the logits.  Shared; nothing below modifies it."""
    parents = TREES[tree]
    J = len(parents)
    L = lengths_for(parents, G, R, seed=31)
    w = asymmetric_taps(J, R, seed=7) if asym else taps_for(L, G, R)
    p = softmax32(scale * make_logits(frames, parents, L, G, seed=37)[0])
    A64, s, valid = upward_model(p, w, parents, G, floor)
    assert valid.all() and (s >= 1e-12).all()
    return {"parents": parents, "J": J, "p": p, "w": w, "A64": A64, "A": A64.astype(np.float32), "s": s}


def law_error(k, floor, taps, exact=False, G=G, R=R):
    """Worst |model's probabilities - A_c(y) F_c(x, y) / sum_y|, as a share of the peak, over every edge and parent voxel, and the
    root's against A_0 / sum.  ``taps``: the blocks handed to the MODEL; the reference uses the case's own.  ``G``, ``R``: another
    grid than this file's (tests/test_path_sampler_domain_host.py takes it at 3^3)."""
    N = G ** 3
    A = k["A64"][0] if exact else k["A"][0]
    worst = 0.0
    root = A[0].astype(np.float64)
    got = conditional_masses(A[0], None, None, G, R, floor)["law"]
    worst = max(worst, float(np.abs(got - root / root.sum()).max() / (root / root.sum()).max()))
    for c in range(1, k["J"]):
        F = edge_factor(k["w"][c], G, R, floor)
        a = A[c].astype(np.float64)
        for x in range(N):
            want = a * F[x]
            want /= want.sum()
            m = conditional_masses(A[c], x, taps[c], G, R, floor)
            assert m["mass"] > 0
            worst = max(worst, float(np.abs(m["law"] - want).max() / want.max()))
    return worst


def reversed_taps(w):
    W = 2 * R + 1
    return np.ascontiguousarray(w.reshape(-1, W, W, W)[:, ::-1, ::-1, ::-1]).reshape(w.shape)


# ------------------------------------------------------------------------------------------------------------------ the law
@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("tree", sorted(TREES))
def test_every_conditional_equals_the_dense_edge_factor(tree, floor):
    """No sampling noise: for every edge and every parent voxel x the N probabilities the model's own masses imply against
    A_c(y) F_c(x, y) normalised, F the dense 64 x 64 factor; the root's against A_0 normalised.  To 1e-12 of the peak."""
    for asym in (False, True):
        k = case(tree, floor, asym)
        worst = law_error(k, floor, k["w"])
        print(f"{tree} floor {floor} asym {asym}: worst {worst:.3e} of the peak")
        assert worst <= 1e-12


@pytest.mark.parametrize("floor", FLOORS)
def test_a_reversed_tap_model_is_visibly_wrong_with_asymmetric_taps(floor):
    """Both directions: the model with the taps as given is exact (above), with the taps reversed it is off by more than 1e-3 of the
    peak on every tree; with the symmetric shell taps the reversal changes nothing."""
    for tree in sorted(TREES):
        k = case(tree, floor, True)
        assert law_error(k, floor, k["w"]) <= 1e-12
        assert law_error(k, floor, reversed_taps(k["w"])) > 1e-3
    k = case("chain3", floor, False)
    assert np.array_equal(reversed_taps(k["w"]), k["w"])


@pytest.mark.parametrize("floor", FLOORS)
def test_the_product_of_the_conditionals_is_the_posterior_over_whole_poses(floor):
    """A 3-chain at G = 3: the model's root law times its two conditionals, for each of the 27^3 poses, against the brute-force posterior
    prod p_j prod F_c normalised, to 1e-12 of the peak; the marginals of that product against skeleton_couple_model's beliefs to 1e-12.
    The upward products go in unrounded (float64): rounding A_j to float32 is the sampler's input format, not part of the law."""
    g, r = 3, 2
    n = g ** 3
    rng = np.random.default_rng(11)
    p = softmax32(2.0 * rng.standard_normal((1, 3, n)))
    q = p[0].astype(np.float64)
    # the shell taps are symmetric, as the coupling's one operator for both directions needs them; the asymmetric blocks (three taps
    # in ten exactly 0) test the orientation of the joint law, which the coupling's beliefs cannot
    for w, symmetric in ((taps_for(lengths_for(CHAIN3, g, r, seed=31), g, r), True), (asymmetric_taps(3, r, seed=13, zeros=0.3), False)):
        # the definition's constants (formed in float32) for the joint law; for the marginals skeleton_couple_model's own (the same
        # two formed in float64), on both sides: the two sets differ by a float32 rounding, 6e-8, which is no part of the law
        for wide in ((False, True) if symmetric else (False,)):
            A, s, valid = upward_model(p, w, CHAIN3, g, floor, wide=wide)
            assert valid.all()
            root = conditional_masses(A[0, 0], None, None, g, r, floor)["law"]
            C = [None] + [np.stack([conditional_masses(A[0, c], x, w[c], g, r, floor, wide=wide)["law"] for x in range(n)]) for c in (1, 2)]
            got = root[:, None, None] * C[1][:, :, None] * C[2][None, :, :]
            F1, F2 = edge_factor(w[1], g, r, floor, wide=wide), edge_factor(w[2], g, r, floor, wide=wide)
            want = q[0][:, None, None] * q[1][None, :, None] * q[2][None, None, :] * F1[:, :, None] * F2[None, :, :]
            want /= want.sum()
            assert np.abs(got - want).max() <= 1e-12 * want.max()
            if wide:
                beliefs = skeleton_couple_model(p, voxel_coord(g), w, CHAIN3, g, floor)[0][0]
                for j, axes in enumerate(((1, 2), (0, 2), (0, 1))):
                    assert np.abs(got.sum(axis=axes) - beliefs[j]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ the statistics
def count_bound(prob):
    return 5.0 * np.sqrt(S * prob * (1.0 - prob)) + 1.0


@pytest.mark.parametrize("floor", FLOORS)
def test_sample_frequencies_match_the_beliefs_and_the_pairwise_posterior(floor):
    """S = 4096 poses, seed 0, CHAIN3 at G = 4: |count - S prob| <= 5 sqrt(S prob (1 - prob)) + 1 for every joint and voxel against the
    coupled belief, and for every (parent, child) pair of voxels of both edges against the dense pairwise posterior
    b_parent(x) A_c(y) F_c(x, y) / sum_y.  A condition on the sampler, not a knob; the seed is not tuned.

    What the bound is worth.  It is a five-sigma bound where the expected count is large; a cell that expects well under one count
    is Poisson and fails with a probability of up to about 1e-4 (expected 0.2, observed 4).  The exact binomial probability that a
    CORRECT sampler fails, summed over the cells of a case from the reference laws alone (the coupling model's beliefs, the dense pair
    posterior; the binomial tails of every cell, summed), is 3.0e-3 / 3.1e-3 / 2.5e-3 for the marginals and 7.1e-3 / 7.1e-3 / 6.8e-3
    for the pairs at floor 0 / 1e-3 / 0.3: 1.0e-2 per case.  That is with the case generator's logits times FREQ_SCALE = 2; unscaled
    they leave more cells in the Poisson band, 1.1e-2 and 6.9e-2 to 9.0e-2, above the 2e-2 the test allows itself; times 3 it is
    1.8e-3 and 2.6e-3 to 4.3e-3, but fewer cells hold any count.  The scale was chosen from these figures, which come from the
    reference laws, not from what the sampler gives.  The law itself is tested without noise above."""
    k = case("chain3", floor, scale=FREQ_SCALE)
    parents = k["parents"]
    got = skeleton_sample_model(k["A"], None, k["w"], parents, G, R, floor, S, seed=0)
    assert (got["index"] >= 0).all() and (got["kind"][:, 0, 0] == FRESH).all() and (got["kind"][:, 0, 1:] != FRESH).all()
    beliefs = skeleton_couple_model(k["p"], voxel_coord(G), k["w"], parents, G, floor)[0][0]
    for j in range(3):
        count = np.bincount(got["index"][:, 0, j], minlength=N)
        excess = np.abs(count - S * beliefs[j]) - count_bound(beliefs[j])
        assert excess.max() <= 0.0, f"a count of joint {j} is {excess.max():.3f} beyond the bound"
    for c in (1, 2):
        a = k["A64"][0, c]
        cond = a[None, :] * edge_factor(k["w"][c], G, R, floor)
        pair = (beliefs[parents[c]][:, None] * cond / cond.sum(axis=1, keepdims=True)).reshape(-1)
        count = np.bincount(got["index"][:, 0, parents[c]].astype(np.int64) * N + got["index"][:, 0, c], minlength=N * N)
        excess = np.abs(count - S * pair) - count_bound(pair)
        assert excess.max() <= 0.0, f"a pair count of edge {c} is {excess.max():.3f} beyond the bound"
    if floor == 0.0:
        assert not (got["kind"] == JUMP).any()
    if floor == 0.3:
        assert (got["kind"] == JUMP).any() and (got["kind"] == STEP).any()


# ------------------------------------------------------------------------------------------------------------------ invariance
def test_results_do_not_depend_on_how_frames_and_samples_are_cut():
    floor = 1e-3
    k = case("tree15", floor, frames=5)
    par, A, w = k["parents"], k["A"], k["w"]
    whole = skeleton_sample_model(A, None, w, par, G, R, floor, 64, seed=7)
    few = skeleton_sample_model(A, None, w, par, G, R, floor, 16, seed=7)
    for key in ("index", "kind"):
        assert np.array_equal(few[key], whole[key][:16]), key                      # sample s of 16 is sample s of 64
    five = skeleton_sample_model(A, None, w, par, G, R, floor, 5, seed=7)
    for cut in (1, 2):
        head = skeleton_sample_model(A[:cut], None, w, par, G, R, floor, 5, seed=7)
        tail = skeleton_sample_model(A[cut:], None, w, par, G, R, floor, 5, seed=7, first_frame=cut)
        for key in ("index", "kind"):
            assert np.array_equal(np.concatenate([head[key], tail[key]], axis=1), five[key]), (cut, key)
    lo = skeleton_sample_model(A, None, w, par, G, R, floor, 2, seed=7)
    hi = skeleton_sample_model(A, None, w, par, G, R, floor, 3, seed=7, first_sample=2)
    for key in ("index", "kind"):
        assert np.array_equal(np.concatenate([lo[key], hi[key]], axis=0), five[key]), key
    other = skeleton_sample_model(A, None, w, par, G, R, floor, 5, seed=8)
    assert not np.array_equal(other["index"], five["index"]) and five["index"].dtype == np.int32
    # frames are independent draws: frame 1 is not frame 0 drawn again
    same = skeleton_sample_model(np.stack([A[0], A[0]]), None, w, par, G, R, floor, 64, seed=7)
    assert not np.array_equal(same["index"][:, 0], same["index"][:, 1])


# ------------------------------------------------------------------------------------------------------------------ the edge rules
def test_a_zero_is_never_drawn_and_no_floor_never_jumps():
    k = case("star5", 0.3)
    rng = np.random.default_rng(9)
    sparse = k["A"] * (rng.random(k["A"].shape) > 0.6)
    assert (sparse == 0).mean() > 0.5
    got = skeleton_sample_model(sparse, None, k["w"], k["parents"], G, R, 0.3, 512, seed=2)
    assert {STEP, JUMP, FRESH} <= set(np.unique(got["kind"]).tolist())
    for j in range(k["J"]):
        x = got["index"][:, 0, j]
        assert (x >= 0).all() and (sparse[0, j, x] > 0).all()
    zero = skeleton_sample_model(k["A"], None, k["w"], k["parents"], G, R, 0.0, 512, seed=2)
    assert (zero["kind"][:, :, 1:] == STEP).all() and (zero["kind"][:, :, 0] == FRESH).all()
    one = skeleton_sample_model(k["A"], None, k["w"], k["parents"], G, R, 1.0, 64, seed=2)
    assert (one["kind"][:, :, 1:] == JUMP).all() and (one["index"] >= 0).all()
    # a joint without mass has no draw, and its children are drawn afresh
    dead = case("chain3", 1e-3)["A"].copy()
    dead[0, 1] = 0.0
    got = skeleton_sample_model(dead, None, case("chain3", 1e-3)["w"], CHAIN3, G, R, 1e-3, 32, seed=2)
    assert (got["index"][:, 0, 1] == -1).all() and (got["kind"][:, 0, 1] == FRESH).all()
    assert (got["kind"][:, 0, 2] == FRESH).all() and (got["index"][:, 0, [0, 2]] >= 0).all()


def test_uniform_volumes_at_u_zero_draw_index_zero():
    flat = np.full(N, 1.0 / N, dtype=np.float32)
    vol = Volume(flat, G)
    z = np.zeros(3)
    assert vol.global_draw(z, z, z).tolist() == [0, 0, 0]
    from volume_sampler_model import window_draw
    w = taps_for(lengths_for(CHAIN3, G, R, seed=31), G, R)
    W = 2 * R + 1
    w3 = w[1].astype(np.float64).reshape(W, W, W)
    for x in (0, 21, N - 1):
        win = window(vol, x, w3, R)
        got = int(window_draw(win, G, z[:1], z[:1], z[:1])[0])
        # the first cell of the clipped window, in ascending (i, j, k), that lies under a non-zero tap
        xi, xj, xk = x // 16, (x // 4) % 4, x % 4
        cells = [(i * 4 + j) * 4 + kk for i in range(4) for j in range(4) for kk in range(4) if w3[i - xi + R, j - xj + R, kk - xk + R] != 0]
        assert got == cells[0]


def test_a_nan_under_a_tap_and_under_a_zero_tap():
    """A NaN cell under a NON-ZERO tap of a child's window: the window mass is NaN, the child is drawn as an unlinked joint (kind 2),
    that global draw has no total, so the child is invalid and ITS children are fresh draws.  A NaN under a ZERO tap is passed over:
    r, q and Wsum - the step's mass and all three levels of its draw - are bit for bit those of the clean volume.  (The joint's own
    global total still holds the NaN, and the definition forms the jump mass from it: in the chain such a joint has no usable mass
    either.  A frame with a NaN in A_c has a NaN s_c and arrives with valid = 0 from the upward call.)"""
    floor = 1e-3
    k = case("chain3", floor, True)                              # asymmetric blocks: every tap non-zero, R = G - 1 covers the grid
    assert (k["w"][1:] > 0).all()
    A = k["A"].copy()
    A[0, 1, 17] = np.nan
    got = skeleton_sample_model(A, None, k["w"], CHAIN3, G, R, floor, 64, seed=5)
    clean = skeleton_sample_model(k["A"], None, k["w"], CHAIN3, G, R, floor, 64, seed=5)
    assert (got["index"][:, 0, 1] == -1).all() and (got["kind"][:, 0, 1] == FRESH).all()
    assert (got["kind"][:, 0, 2] == FRESH).all() and (got["index"][:, 0, 2] >= 0).all()
    assert np.array_equal(got["index"][:, 0, 0], clean["index"][:, 0, 0])
    # under a zero tap: the taps of the child vanish wherever dk != 0, the NaN sits in another column than the parent
    W = 2 * R + 1
    w3 = k["w"][1].astype(np.float64).reshape(W, W, W).copy()
    w3[:, :, np.arange(W) != R] = 0.0
    x = (1 * G + 2) * G + 1                                      # parent voxel (1, 2, 1)
    dirty = k["A"][0, 1].copy()
    dirty[(2 * G + 0) * G + 3] = np.nan                          # (2, 0, 3): dk = 2, a zero tap
    a, b = window(Volume(k["A"][0, 1], G), x, w3, R), window(Volume(dirty, G), x, w3, R)
    for key in ("tk", "ck", "tj", "cj", "ti", "ci"):
        assert np.array_equal(a[key], b[key]), key
    assert a["Wsum"] == b["Wsum"] and np.isfinite(a["Wsum"]) and a["Wsum"] > 0
    dirty[(2 * G + 0) * G + 1] = np.nan                          # (2, 0, 1): dk = 0, a non-zero tap
    assert np.isnan(window(Volume(dirty, G), x, w3, R)["Wsum"])


def test_an_invalid_frame_writes_no_draw():
    k = case("tree15", 1e-3, frames=5)
    valid = np.array([1, 0, 1, 1, 0])
    got = skeleton_sample_model(k["A"], valid, k["w"], k["parents"], G, R, 1e-3, 8, seed=3)
    whole = skeleton_sample_model(k["A"], None, k["w"], k["parents"], G, R, 1e-3, 8, seed=3)
    assert (got["index"][:, [1, 4]] == -1).all() and (got["kind"][:, [1, 4]] == FRESH).all()
    for key in ("index", "kind"):
        assert np.array_equal(got[key][:, [0, 2, 3]], whole[key][:, [0, 2, 3]])


# ------------------------------------------------------------------------------------------------------------------ the surface
def test_best_pose_of_samples_on_a_hand_made_case():
    gt = np.zeros((3, 2, 3))
    est = gt + np.array([0.3, 0.0, 0.0])                                             # the estimate: 0.3 off on every joint
    coord = np.zeros((3, 2, 2, 3))                                                   # [T, S, J, 3]
    valid = np.ones((3, 2, 2), dtype=bool)
    coord[0, 0, :, 0] = (0.1, 0.5)                                                   # frame 0: poses with mean errors 0.3 and 0.2
    coord[0, 1, :, 0] = (0.4, 0.0)
    coord[1, 0, :, 0] = (0.0, 0.0)                                                   # frame 1: the perfect pose lacks a joint
    valid[1, 0, 1] = False
    coord[1, 1, :, 0] = (0.2, 0.6)
    valid[2] = False                                                                 # frame 2: no whole pose, the estimate's 0.3
    coord[2] = np.nan
    frames = [{"coord": coord[t], "valid": valid[t], "spread": np.array([0.1 + t, 0.2 + t])} for t in range(3)]
    got = metrics.best_pose_of_samples(frames, est, gt)
    assert got["best_pose_of_n_mpjpe"] == pytest.approx((0.2 + 0.4 + 0.3) / 3, abs=1e-15)
    assert got["estimate_mpjpe"] == pytest.approx(0.3) and got["whole_poses"] == 3 and got["poses"] == 6
    assert got["frames_without_pose"] == 1 and got["samples_per_frame"] == 2
    # per joint the figure may pick the joints of different poses apart, so it is never above the whole-pose one
    assert metrics.best_of_samples(frames, est, gt)["best_of_n_mpjpe"] == pytest.approx((0.05 + 0.3 + 0.3) / 3, abs=1e-15)
    with pytest.raises(ValueError, match="shape mismatch"):
        metrics.best_pose_of_samples(frames[:2], est, gt)


def test_binding_and_scratch_sizes():
    for name, args in (("se_skeleton_upward_f32", 15), ("se_skeleton_upward_scratch_bytes", 4), ("se_skeleton_sample_f32", 20),
                       ("se_skeleton_sample_scratch_bytes", 3)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == args
    assert _lib.ABI_VERSION >= 39
    lib = _lib.load()
    assert lib.se_skeleton_sample_scratch_bytes(3, 15, 64) == 3 * 15 * (64 * 64 + 64) * 8
    for bad in ((0, 15, 64), (1, 0, 64), (1, 33, 64), (1, 15, 1), (1, 15, 129)):
        assert lib.se_skeleton_sample_scratch_bytes(*bad) == 0
    assert lib.se_skeleton_sample_scratch_bytes(2 ** 31 - 1, 32, 128) == (2 ** 31 - 1) * 32 * (128 * 128 + 128) * 8
    # the upward call: U alone per frame in flight, against the coupling's A, U and D; at most four frames in flight
    up, couple = lib.se_skeleton_upward_scratch_bytes(1, 15, 64, 18), lib.se_skeleton_couple_scratch_bytes(1, 15, 64, 18)
    assert couple - up == 2 * 15 * 64 ** 3 * 4
    assert lib.se_skeleton_upward_scratch_bytes(9, 15, 64, 18) == lib.se_skeleton_upward_scratch_bytes(4, 15, 64, 18)
    for bad in ((0, 15, 64, 18), (1, 0, 64, 18), (1, 33, 64, 18), (1, 15, 1, 0), (1, 15, 129, 18), (1, 15, 64, 25), (1, 15, 8, 8)):
        assert lib.se_skeleton_upward_scratch_bytes(*bad) == 0


def test_lib_refuses_cpu_tensors_and_bad_ranges():
    a = torch.zeros((1, 1, 8))
    i = torch.zeros((1, 1, 1), dtype=torch.int32)
    taps = torch.ones((1, 1))
    with pytest.raises(_lib.HipExtensionError, match="HIP device"):
        _lib.skeleton_sample(a, None, taps, (0,), i, i.clone(), 1, 8, 2, 0, 1e-3, 1)
    with pytest.raises(_lib.HipExtensionError, match="HIP device"):
        _lib.skeleton_upward(a, taps, (0,), a.clone(), torch.zeros((1, 1)), torch.zeros(1, dtype=torch.int32), 1, 8, 2, 0, 1e-3)
    for kw in ({"samples": 0}, {"first_sample": -1}, {"first_frame": 2 ** 32}, {"first_sample": 2 ** 32}, {"seed": -1}, {"seed": 2 ** 64}):
        args = {"samples": 1, "first_sample": 0, "first_frame": 0, "seed": 0}
        args.update(kw)
        with pytest.raises(_lib.HipExtensionError, match="expected"):
            _lib.skeleton_sample(a, None, taps, (0,), i, i.clone(), 1, 8, 2, 0, 1e-3, **args)
    for parents in ((1,), (0, 1), (0,) * 33, ()):
        with pytest.raises(_lib.HipExtensionError, match="parents"):
            _lib.skeleton_sample(a, None, taps, parents, i, i.clone(), 1, 8, 2, 0, 1e-3, 1)
    for grid, radius, floor in ((1, 0, 0.0), (129, 0, 0.0), (2, 2, 0.0), (2, 0, -0.1), (2, 0, 1.5)):
        with pytest.raises(_lib.HipExtensionError):
            _lib.skeleton_sample(a, None, taps, (0,), i, i.clone(), 1, grid ** 3, grid, radius, floor, 1)


def test_sample_refuses_bad_arguments_without_a_device():
    coord = np.zeros((8, 8, 8, 3), dtype=np.float32)
    s = SkeletonPrior(coord=coord, grid=8, cuboid_side=2.0, bone_lengths=[0.5] * 14)
    vol = torch.zeros((2, 15, 8, 8, 8))
    for bad in (vol[0], vol[:, :14], vol.double(), vol[:0], vol.numpy(), torch.zeros((2, 15, 8, 8, 4))):
        with pytest.raises(ValueError, match="sample: volumes"):
            s.sample(bad)
    with pytest.raises(ValueError, match="sample: joints"):
        s.sample(vol, joints=torch.zeros((2, 14, 3)))
    for kw in ({"samples": 0}, {"samples": -3}, {"seed": -1}, {"seed": 2 ** 64}, {"first_frame": -1}, {"first_sample": -1},
               {"first_frame": 2 ** 32 - 1}, {"first_sample": 2 ** 32 - 15}, {"samples": "many"}):
        with pytest.raises(ValueError, match="sample:"):
            s.sample(vol, **kw)
    with pytest.raises(_lib.HipExtensionError):                                       # checked, and then: the volumes are on the CPU
        s.sample(vol, samples=4, seed=2 ** 64 - 1, first_frame=2 ** 32 - 2, first_sample=2 ** 32 - 4)
