"""GPU: the pose sampler (csrc/skeleton_sample.hip: se_skeleton_upward_f32, se_skeleton_sample_f32) against its numpy model
(tests/skeleton_sampler_model.py): the upward products within a derived bound of the float64 recursion and bit for bit against the
library's own coupling, every drawn voxel and branch bit for bit, independence of how frames and samples are cut, the argument checks,
the public surface and the command line.

Inputs: the eight shapes of tests/test_gpu_skeleton_prior.py (its CASES, built from tests/skeleton_prior_cases.py the same way),
softmaxed by se_softargmax3d_f32 on the device.

TOLERANCE of the upward products (derived, not measured).  u = 2^-24.  test_gpu_skeleton_prior.py derives for one message
e_msg = (T(R) + L + c) u and, every term being non-negative, for a product fed by one message per edge of a tree of J - 1 edges a
relative error of at most B = 1.01 (2 (J - 1) + 1) e_msg.  A_j = p_j prod U_c is fed by one message per edge of j's SUBTREE, at most
J - 1 of them, so B bounds it too; s_j = sum A_j adds its own chain, L u.
The absolute term is float32 underflow, which the upward products - un-normalised, unlike the beliefs - can reach.  With d = 2^-126
(the smallest normal number: what one operation can lose, denormals flushed or not), U <= 1 and p <= 1:
    a correlation's chain of T(R) fused multiply-adds loses at most T(R) d, so a message into j from child c is off by at most
        m_c = (delta_c + T(R) d) / s_c + 2 d        (the quotient and the final fused multiply-add once each)
    and the product A_j, whose other factors are at most 1, by
        delta_j = sum over the children c of (m_c + d)            (delta of a leaf is 0: A_j = p_j, copied)
with the s_c of the model.  So
    upward   |got - want| <= B want + delta_j          sums   |got - want| <= (B + L u) want + N delta_j          valid   exact
The model's condition on the inputs is asserted with every case: each s_j is >= 1e-12 and no frame is invalid.
"""
import ctypes
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD, synthetic_state_dict
from sceneego_amd import _lib, load_config, metrics, op, synth
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, SAMPLE_GROUP, shell_taps
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
from skeleton_prior_cases import CHAIN3, SIDE, STAR5, lengths_for, make_logits, taps_for
from skeleton_prior_model import children
from skeleton_sampler_model import FRESH, JUMP, STEP, skeleton_sample_model, upward_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TINY = 2.0 ** -126
L = _lib.SKELETON_SUM_CHAIN
TREE = KINEMATIC_PARENTS
TREES = {"chain3": CHAIN3, "tree15": TREE, "star5": STAR5, "one": (0,)}
FLOORS = (0.0, 1e-3, 0.3)
S = 5

# frames, tree, G, R: the eight shapes of tests/test_gpu_skeleton_prior.py: CASES (two of them differ there by the floor alone)
SHAPES = [
    (1, "chain3", 8, 3),
    (2, "tree15", 8, 4),
    (1, "tree15", 6, 5),            # R = G - 1: every window clipped on both sides
    (3, "tree15", 10, 4),           # G % 4 = 2
    (2, "tree15", 16, 6),
    (2, "tree15", 16, 6),
    (1, "star5", 8, 3),             # four children
    (1, "one", 8, 0),
]
SHAPE_IDS = [f"{n}-{f}x{t}-G{g}-R{r}" for n, (f, t, g, r) in enumerate(SHAPES)]


def belief_bound(parents, R):
    kids = max(sum(1 for c in range(1, len(parents)) if parents[c] == j) for j in range(len(parents)))
    return 1.01 * (2 * (len(parents) - 1) + 1) * (_lib.SHELL_CHAIN(R) + L + 8 + kids) * U


# ------------------------------------------------------------------------------------------------------------------ inputs, launch
def softmax_on_device(logits, coord):
    F, J, N = logits.shape
    x = torch.from_numpy(logits).to(DEV).reshape(F * J, N)
    prob = torch.empty_like(x)
    joints = torch.empty((F * J, 3), device=DEV, dtype=torch.float32)
    _lib.softargmax3d(x, coord, prob, joints, F * J, N, 1)
    torch.cuda.synchronize()
    return prob.view(F, J, N)


@functools.lru_cache(maxsize=None)
def case(frames, tree, G, R):
    """Softmaxed volumes [frames, J, N] on the device and on the host, the taps and the coordinates, computed once and shared (nothing
    below modifies them).  Seeds, lengths and logits as tests/test_gpu_skeleton_prior.py: case builds them."""
    parents = TREES[tree]
    N = G ** 3
    seed = 1000 * G + 10 * len(parents) + R
    lengths = lengths_for(parents, G, R, seed)
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    prob = softmax_on_device(make_logits(frames, parents, lengths, G, seed)[0], coord)
    taps = taps_for(lengths, G, R) if len(parents) > 1 else np.zeros((1, (2 * R + 1) ** 3), dtype=np.float32)
    return {"prob": prob, "coord": coord, "p": prob.cpu().numpy(), "taps": taps, "parents": parents,
            "taps_dev": torch.from_numpy(taps).to(DEV), "lengths": lengths}


def upward_dev(prob, taps_dev, parents, G, R, floor):
    """One _lib-level call over all frames of ``prob`` [F, J, N]: device tensors (upward, sums, valid), pre-filled with sentinels."""
    F, J, N = prob.shape
    A = torch.full((F, J, N), float("nan"), device=DEV)
    sums = torch.full((F, J), float("nan"), device=DEV)
    valid = torch.full((F,), -1, device=DEV, dtype=torch.int32)
    _lib.skeleton_upward(prob.contiguous(), taps_dev, parents, A, sums, valid, F, N, G, R, floor)
    torch.cuda.synchronize()
    return A, sums, valid


def sample_dev(A, valid, taps_dev, parents, G, R, floor, samples, first_sample=0, first_frame=0, seed=0):
    """One se_skeleton_sample_f32 call: host arrays (index, kind) [samples, F, J]."""
    F, J, N = A.shape
    index = torch.full((samples, F, J), -7, device=DEV, dtype=torch.int32)
    kind = torch.full((samples, F, J), -7, device=DEV, dtype=torch.int32)
    _lib.skeleton_sample(A, valid, taps_dev, parents, index, kind, F, N, G, R, floor, samples, first_sample=first_sample,
                         first_frame=first_frame, seed=seed)
    torch.cuda.synchronize()
    return index.cpu().numpy(), kind.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_draws(A, valid, taps, parents, G, R, floor, samples, what, **kw):
    """Device against model on the host array ``A`` [F, J, N] float32, bit for bit; returns the model's dict."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    v_dev = None if valid is None else torch.from_numpy(np.asarray(valid, dtype=np.int32)).to(DEV)
    gi, gk = sample_dev(torch.from_numpy(A).to(DEV), v_dev, torch.from_numpy(taps).to(DEV), parents, G, R, floor, samples, **kw)
    want = skeleton_sample_model(A, valid, taps, parents, G, R, floor, samples, **kw)
    wrong = int((gi != want["index"]).sum()), int((gk != want["kind"]).sum())
    assert wrong == (0, 0), f"{what}: {wrong[0]} voxels and {wrong[1]} kinds of {gi.size} differ from the model"
    return want


# ------------------------------------------------------------------------------------------------------------------ 1. upward, float64
def underflow_term(parents, s, R):
    """delta [F, J] of the docstring, from the model's sums ``s`` [F, J]."""
    J = len(parents)
    ch = children(parents)
    delta = np.zeros(s.shape)
    for j in range(J - 1, -1, -1):
        for c in ch[j]:
            delta[:, j] += (delta[:, c] + _lib.SHELL_CHAIN(R) * TINY) / s[:, c] + 3 * TINY
    return delta


@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("frames,tree,G,R", SHAPES[:5] + SHAPES[6:], ids=SHAPE_IDS[:5] + SHAPE_IDS[6:])
def test_upward_against_the_model(frames, tree, G, R, floor):
    k = case(frames, tree, G, R)
    N = G ** 3
    wA, ws, wv = upward_model(k["p"], k["taps"], k["parents"], G, floor)
    assert wv.all() and ws.min() >= 1e-12, f"a sum of {ws.min()}"                 # the condition on the inputs, on the model
    A, sums, valid = (x.cpu().numpy() for x in upward_dev(k["prob"], k["taps_dev"], k["parents"], G, R, floor))
    assert valid.tolist() == [1] * frames
    B = belief_bound(k["parents"], R)
    assert B < 0.01
    delta = underflow_term(k["parents"], ws, R)
    err = np.abs(A.astype(np.float64) - wA)
    tol = B * wA + delta[:, :, None]
    serr = np.abs(sums.astype(np.float64) - ws)
    print(f"{tree} G {G} R {R} floor {floor}: bound {B / U:.0f} u; worst upward {float((err / (wA + 2.0 ** -100)).max()) / U:.2f} u, "
          f"sums {float((serr / ws).max()) / U:.2f} u; smallest sum {ws.min():.3g}; largest underflow term {delta.max():.3g}")
    assert (err <= tol).all(), f"an upward product is off by {float((err - tol).max()):.3e} beyond the bound"
    assert (serr <= (B + L * U) * ws + N * delta).all(), f"a sum is off by {float((serr / ws).max()):.3e} relative"


# ------------------------------------------------------------------------------------------------------------------ 2. upward, library
@pytest.mark.parametrize("floor", (0.0, 1e-3))
@pytest.mark.parametrize("frames,tree,G,R", SHAPES[:5] + SHAPES[6:], ids=SHAPE_IDS[:5] + SHAPE_IDS[6:])
def test_upward_sums_are_the_couplings_own_bit_for_bit(frames, tree, G, R, floor):
    k = case(frames, tree, G, R)
    J, N = len(k["parents"]), G ** 3
    _, sums, valid = upward_dev(k["prob"], k["taps_dev"], k["parents"], G, R, floor)
    joints, evidence = torch.empty((frames, J, 3), device=DEV), torch.empty((frames, J), device=DEV)
    coupled = torch.empty((frames,), device=DEV, dtype=torch.int32)
    _lib.skeleton_couple(k["prob"], k["coord"], k["taps_dev"], k["parents"], None, joints, evidence, coupled, frames, N, G, R, floor)
    stats, norms = torch.empty((frames, J, 4), device=DEV), torch.empty((frames, J, 3), device=DEV)
    ok = torch.empty((frames,), device=DEV, dtype=torch.int32)
    _lib.skeleton_edge_stats(k["prob"], k["taps_dev"], k["taps_dev"], k["taps_dev"], k["parents"], stats, norms, ok, frames, N, G, R, floor)
    torch.cuda.synchronize()
    sums, valid, coupled = sums.cpu().numpy(), valid.cpu().numpy(), coupled.cpu().numpy()
    assert same_bits(sums[:, 1:], np.ascontiguousarray(norms.cpu().numpy()[:, 1:, 0]))
    assert same_bits(sums[:, 0], np.ascontiguousarray(evidence.cpu().numpy()[:, 0]))
    assert (valid[coupled == 1] == 1).all() and coupled.all()


def test_a_nan_stays_in_its_frame():
    """A NaN in one volume reaches the sums of its joint and of every ancestor: its frame is invalid, and no other frame changes."""
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    clean = [x.cpu().numpy() for x in upward_dev(k["prob"], k["taps_dev"], TREE, G, R, 1e-3)]
    prob = k["prob"].clone()
    prob[1, 9, 345] = float("nan")
    A, sums, valid = (x.cpu().numpy() for x in upward_dev(prob, k["taps_dev"], TREE, G, R, 1e-3))
    assert valid.tolist() == [1, 0, 1] and np.isnan(sums[1, 9]) and np.isnan(sums[1, 0])
    assert same_bits(A[[0, 2]], clean[0][[0, 2]]) and same_bits(sums[[0, 2]], clean[1][[0, 2]])
    # a frame that is invalid draws nothing; the frames beside it are those of the clean call
    gi, gk = sample_dev(torch.from_numpy(A).to(DEV), torch.from_numpy(valid).to(DEV), k["taps_dev"], TREE, G, R, 1e-3, 4, seed=3)
    ci, ck = sample_dev(torch.from_numpy(clean[0]).to(DEV), None, k["taps_dev"], TREE, G, R, 1e-3, 4, seed=3)
    assert (gi[:, 1] == -1).all() and (gk[:, 1] == FRESH).all()
    assert np.array_equal(gi[:, [0, 2]], ci[:, [0, 2]]) and np.array_equal(gk[:, [0, 2]], ck[:, [0, 2]])


# ------------------------------------------------------------------------------------------------------------------ 3. draws
@functools.lru_cache(maxsize=None)
def drawn(n, floor):
    """The device's own upward products of shape ``n`` at ``floor``, read back, and the model's draws on them (checked against the
    device's)."""
    frames, tree, G, R = SHAPES[n]
    k = case(frames, tree, G, R)
    A, _, valid = upward_dev(k["prob"], k["taps_dev"], k["parents"], G, R, floor)
    assert valid.cpu().numpy().all()
    return check_draws(A.cpu().numpy(), None, k["taps"], k["parents"], G, R, floor, S, f"shape {n} floor {floor}", seed=n)


@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("n", range(len(SHAPES)), ids=SHAPE_IDS)
def test_draws_bit_for_bit(n, floor):
    want = drawn(n, floor)
    J = len(TREES[SHAPES[n][1]])
    assert want["index"].shape == (S, SHAPES[n][0], J) and (want["index"] >= 0).all() and (want["kind"][:, :, 0] == FRESH).all()


def test_every_branch_occurs_in_the_set():
    kinds = np.concatenate([drawn(n, floor)["kind"].reshape(-1) for n in range(len(SHAPES)) for floor in FLOORS])
    count = {name: int((kinds == v).sum()) for name, v in (("step", STEP), ("jump", JUMP), ("fresh", FRESH))}
    print(f"over the set: {count}")
    assert min(count.values()) > 0


def dense_taps(J, R, seed, zeros=0.0):
    rng = np.random.default_rng(seed)
    w = rng.random((J, (2 * R + 1) ** 3)) + 0.05
    w *= rng.random(w.shape) >= zeros
    w[0] = 0.0
    if J > 1:
        w[1:] /= w[1:].sum(axis=1, keepdims=True)
    return w.astype(np.float32)


def test_draws_on_hand_made_upward_arrays():
    rng = np.random.default_rng(17)
    G, R = 6, 2
    N = G ** 3
    w = dense_taps(5, R, 3, zeros=0.4)
    base = (rng.random((2, 5, N)) ** 4).astype(np.float32)
    # uniform volumes
    check_draws(np.full((2, 5, N), 1.0 / N), None, w, STAR5, G, R, 0.3, 16, "uniform")
    # exact zeros: six cells in ten
    sparse = base * (rng.random(base.shape) > 0.6)
    got = check_draws(sparse, None, w, STAR5, G, R, 0.3, 16, "exact zeros", seed=1)
    for f in range(2):
        for j in range(5):
            x = got["index"][:, f, j]
            assert (sparse[f, j, x[x >= 0]] > 0).all()
    # values scaled into the float32 denormals: the float64 sums keep them
    small = (base * np.float32(2.0 ** -140)).astype(np.float32)
    assert 0 < small.max() < 2.0 ** -126
    got = check_draws(small, None, w, STAR5, G, R, 1e-3, 16, "denormals", seed=2)
    assert (got["index"] >= 0).all()
    # a NaN under a non-zero tap of every window (the taps of joint 1 made dense) and one under a zero tap
    full = dense_taps(3, G - 1, 5)
    nan = base[:1, :3].copy()
    nan[0, 1, 77] = np.nan
    got = check_draws(nan, None, full, CHAIN3, G, G - 1, 1e-3, 16, "NaN under a tap", seed=3)
    assert (got["index"][:, 0, 1] == -1).all() and (got["kind"][:, 0, 1:] == FRESH).all() and (got["index"][:, 0, 2] >= 0).all()
    column = full.reshape(3, 2 * G - 1, 2 * G - 1, 2 * G - 1).copy()
    column[:, :, :, np.arange(2 * G - 1) != G - 1] = 0.0               # taps only where dk = 0
    # (this holds the device to the model where a NaN lies under zero taps; it cannot show the zero-tap rule itself: the joint's
    # total holds the NaN too, so the joint has no draw whatever the window sums are - the rule is tested on the model's sums,
    # tests/test_skeleton_sampler_host.py)
    check_draws(nan, None, column.reshape(3, -1), CHAIN3, G, G - 1, 1e-3, 16, "NaN under a zero tap or none", seed=4)
    # a valid = 0 frame among valid ones reads nothing: its volumes are NaN throughout
    holes = base.copy()
    holes[1] = np.nan
    got = check_draws(np.concatenate([holes, base[:1]]), [1, 0, 1], w, STAR5, G, R, 1e-3, 8, "an invalid frame", seed=5)
    assert (got["index"][:, 1] == -1).all() and (got["index"][:, [0, 2]] >= 0).all()
    # G = 2, with R = 1 = G - 1
    check_draws((rng.random((3, 3, 8)) ** 2).astype(np.float32), None, dense_taps(3, 1, 6), CHAIN3, 2, 1, 0.3, 32, "G = 2", seed=6)
    # J = 1: one global draw per pose
    got = check_draws(base[:, :1], None, np.zeros((1, 1), dtype=np.float32), (0,), G, 0, 0.0, 16, "J = 1", seed=7)
    assert (got["kind"] == FRESH).all()
    # a 32-joint chain at G = 4, R = 1
    chain = tuple([0] + list(range(31)))
    check_draws((rng.random((1, 32, 64)) ** 3).astype(np.float32), None, dense_taps(32, 1, 8, zeros=0.3), chain, 4, 1, 1e-3, 8,
                "a chain of 32", seed=8)
    # R = G - 1: every window is clipped on both sides
    check_draws(base[:, :3], None, full, CHAIN3, G, G - 1, 0.0, 16, "R = G - 1", seed=9)


# ------------------------------------------------------------------------------------------------------------------ 4. production
def test_the_production_shape_once():
    """G = 64, R = 18, the 15-joint tree, one frame, S = 2: tau 0.03 m, bone lengths 0.15-0.45 m, as the coupling's production test."""
    G, R, tau = 64, 18, 0.03
    N, h = G ** 3, SIDE / G
    lengths = np.concatenate([[0.0], np.random.default_rng(64).permutation(np.linspace(0.15, 0.45, 14))])
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    prob = softmax_on_device(make_logits(1, TREE, lengths, G, 6418)[0], coord)
    taps = shell_taps(lengths, tau, h, R)
    A, sums, valid = upward_dev(prob, torch.from_numpy(taps).to(DEV), TREE, G, R, 1e-3)
    assert valid.cpu().numpy().tolist() == [1] and (sums > 0).all()
    want = check_draws(A.cpu().numpy(), None, taps, TREE, G, R, 1e-3, 2, "production shape")
    assert (want["index"] >= 0).all() and (want["kind"][:, 0, 1:] != FRESH).all()


# ------------------------------------------------------------------------------------------------------------------ 5. splits
def test_splits_and_determinism():
    G, R, floor = 8, 4, 1e-3
    k = case(2, "tree15", G, R)
    logits = make_logits(5, TREE, k["lengths"], G, 99)[0]
    prob = softmax_on_device(logits, k["coord"])
    keep = prob.clone()
    A, sums, valid = upward_dev(prob, k["taps_dev"], TREE, G, R, floor)
    A2, sums2, valid2 = upward_dev(prob, k["taps_dev"], TREE, G, R, floor)
    assert torch.equal(prob, keep)
    assert same_bits(A.cpu().numpy(), A2.cpu().numpy()) and same_bits(sums.cpu().numpy(), sums2.cpu().numpy()) and torch.equal(valid, valid2)
    # five frames walk two groups inside the call: each frame is that of a call of its own
    for f in (0, 3, 4):
        a1, s1, _ = upward_dev(prob[f:f + 1], k["taps_dev"], TREE, G, R, floor)
        assert same_bits(a1.cpu().numpy(), A[f:f + 1].cpu().numpy()) and same_bits(s1.cpu().numpy(), sums[f:f + 1].cpu().numpy())
    before = A.clone()
    args = (k["taps_dev"], TREE, G, R, floor)
    whole = sample_dev(A, valid, *args, 64, seed=7)
    again = sample_dev(A, valid, *args, 64, seed=7)
    assert torch.equal(A, before)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    few = sample_dev(A, valid, *args, 16, seed=7)
    assert all(np.array_equal(a, b[:16]) for a, b in zip(few, whole))                     # sample s of 16 is sample s of 64
    five = sample_dev(A, valid, *args, 5, seed=7)
    for cut in (1, 2):
        head = sample_dev(A[:cut].contiguous(), valid[:cut].contiguous(), *args, 5, seed=7)
        tail = sample_dev(A[cut:].contiguous(), valid[cut:].contiguous(), *args, 5, seed=7, first_frame=cut)
        assert all(np.array_equal(np.concatenate([a, b], axis=1), c) for a, b, c in zip(head, tail, five)), cut
    lo = sample_dev(A, valid, *args, 2, seed=7)
    hi = sample_dev(A, valid, *args, 3, seed=7, first_sample=2)
    assert all(np.array_equal(np.concatenate([a, b], axis=0), c) for a, b, c in zip(lo, hi, five))
    other = sample_dev(A, valid, *args, 5, seed=8)
    assert not np.array_equal(other[0], five[0])
    far = sample_dev(A, valid, *args, 5, seed=2 ** 64 - 1, first_sample=2 ** 32 - 5, first_frame=2 ** 32 - 5)
    want = skeleton_sample_model(A.cpu().numpy(), None, k["taps"], TREE, G, R, floor, 5, seed=2 ** 64 - 1, first_sample=2 ** 32 - 5,
                                 first_frame=2 ** 32 - 5)
    assert np.array_equal(far[0], want["index"]) and np.array_equal(far[1], want["kind"])


# ------------------------------------------------------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments_raise_and_do_not_launch():
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    N, J, F = G ** 3, 15, 2
    prob = k["prob"][:F].contiguous()
    A, sums, valid = upward_dev(prob, k["taps_dev"], TREE, G, R, 1e-3)
    bad_tree = list(TREE)
    bad_tree[5] = 5
    both = torch.empty((3, J, N), device=DEV)
    out = {"upward": torch.full((F, J, N), -5.0, device=DEV), "sums": torch.full((F, J), -5.0, device=DEV),
           "valid": torch.full((F,), -5, device=DEV, dtype=torch.int32), "index": torch.full((S, F, J), -5, device=DEV, dtype=torch.int32),
           "kind": torch.full((S, F, J), -5, device=DEV, dtype=torch.int32)}

    def up(**kw):
        a = {"prob": prob, "taps": k["taps_dev"], "parents": TREE, "upward": out["upward"], "sums": out["sums"], "valid": out["valid"],
             "frames": F, "voxels": N, "grid": G, "radius": R, "floor": 1e-3}
        a.update(kw)
        return _lib.skeleton_upward(**a)

    def sm(**kw):
        a = {"upward": A, "valid": valid, "taps": k["taps_dev"], "parents": TREE, "index": out["index"], "kind": out["kind"], "frames": F,
             "voxels": N, "grid": G, "radius": R, "floor": 1e-3, "samples": S}
        a.update(kw)
        return _lib.skeleton_sample(**a)

    shared = ({"radius": 25}, {"radius": -1}, {"radius": G}, {"floor": -0.1}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0},
              {"frames": 3}, {"grid": G + 1}, {"voxels": N + 1}, {"grid": 1, "voxels": 1, "radius": 0}, {"parents": bad_tree},
              {"parents": [1] + list(TREE[1:])}, {"parents": list(TREE) + [3]}, {"parents": [0] * 33}, {"parents": []}, {"parents": None},
              {"taps": k["taps_dev"][:-1]}, {"taps": k["taps"]}, {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)})
    for kw in shared + ({"prob": prob.cpu()}, {"prob": prob.double()}, {"prob": prob[:, :, ::2]}, {"upward": prob}, {"upward": None},
                        {"prob": both[:2], "upward": both[1:]}, {"upward": torch.empty((1, J, N), device=DEV)},
                        {"sums": torch.empty((F, J + 1), device=DEV)}, {"sums": None}, {"valid": torch.empty((F,), device=DEV)},
                        {"valid": None}):
        with pytest.raises(_lib.HipExtensionError):
            up(**kw)
    for kw in shared + ({"upward": A.cpu()}, {"upward": A.double()}, {"upward": A[:, :, ::2]}, {"upward": None}, {"samples": 0},
                        {"first_sample": -1}, {"first_frame": -1}, {"first_sample": 2 ** 32 - S + 1}, {"first_frame": 2 ** 32 - F + 1},
                        {"seed": -1}, {"seed": 2 ** 64}, {"index": out["kind"]}, {"index": None}, {"kind": None},
                        {"index": out["index"].float()}, {"kind": torch.empty((S, F, J + 1), device=DEV, dtype=torch.int32)},
                        {"valid": valid.float()}, {"valid": torch.empty((F + 1,), device=DEV, dtype=torch.int32)},
                        {"index": A.view(torch.int32)[0, 0, :S * F * J].view(S, F, J)}):
        with pytest.raises(_lib.HipExtensionError):
            sm(**kw)
    torch.cuda.synchronize()
    assert all(bool((t == -5).all()) for t in out.values())

    # the C entry points refuse on their own what the wrappers check first
    lib = _lib.load()
    P = _lib._ptr
    ws = torch.empty(_lib.skeleton_upward_scratch_bytes(F, J, G, R), device=DEV, dtype=torch.uint8)
    ss = torch.empty(_lib.skeleton_sample_scratch_bytes(F, J, G) + 8, device=DEV, dtype=torch.uint8)
    ss = ss[(-ss.data_ptr()) % 8:]
    need = _lib.skeleton_sample_scratch_bytes(F, J, G)

    def vp(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def raw_up(radius=R, floor=1e-3, frames=F, grid=G, voxels=N, scratch_bytes=ws.numel(), parents=TREE, n=J, src=prob, taps=k["taps_dev"],
               upward=out["upward"], sums_=out["sums"], valid_=out["valid"], scratch=ws, no_tree=False):
        par = (ctypes.c_int * max(len(parents), 1))(*parents)
        return lib.se_skeleton_upward_f32(vp(src), vp(taps), None if no_tree else ctypes.cast(par, ctypes.c_void_p), vp(upward), vp(sums_),
                                          vp(valid_), vp(scratch), scratch_bytes, frames, n, voxels, grid, radius, floor, _lib._stream())

    assert raw_up(radius=25) == raw_up(radius=G) == raw_up(radius=-1) == raw_up(floor=2.0) == raw_up(floor=float("nan")) == -1
    assert raw_up(frames=0) == raw_up(voxels=N + 4) == raw_up(grid=129) == raw_up(grid=1) == raw_up(n=0) == raw_up(n=33) == -1
    assert raw_up(parents=bad_tree) == raw_up(scratch_bytes=ws.numel() - 1) == raw_up(scratch=ws[1:], scratch_bytes=ws.numel() - 1) == -1
    assert raw_up(src=None) == raw_up(taps=None) == raw_up(no_tree=True) == raw_up(upward=None) == raw_up(sums_=None) == -1
    assert raw_up(valid_=None) == raw_up(scratch=None) == raw_up(upward=prob) == -1
    assert raw_up(sums_=out["sums"].view(torch.uint8).reshape(-1)[1:]) == -1                     # misaligned

    def raw_sm(radius=R, floor=1e-3, frames=F, grid=G, voxels=N, scratch_bytes=need, parents=TREE, n=J, samples=S, first_sample=0,
               first_frame=0, upward=A, valid_=valid, taps=k["taps_dev"], index=out["index"], kind=out["kind"], scratch=ss, no_tree=False):
        par = (ctypes.c_int * max(len(parents), 1))(*parents)
        return lib.se_skeleton_sample_f32(vp(upward), vp(valid_), vp(taps), None if no_tree else ctypes.cast(par, ctypes.c_void_p), vp(index),
                                          vp(kind), vp(scratch), scratch_bytes, frames, n, voxels, grid, radius, floor, samples,
                                          first_sample, first_frame, 0, 0, _lib._stream())

    assert raw_sm(radius=25) == raw_sm(radius=G) == raw_sm(radius=-1) == raw_sm(floor=2.0) == raw_sm(floor=float("nan")) == -1
    assert raw_sm(frames=0) == raw_sm(samples=0) == raw_sm(voxels=N + 4) == raw_sm(grid=129) == raw_sm(grid=1) == raw_sm(n=0) == -1
    assert raw_sm(n=33) == raw_sm(parents=bad_tree) == raw_sm(parents=[1] + list(TREE[1:])) == raw_sm(scratch_bytes=need - 1) == -1
    assert raw_sm(first_sample=-1) == raw_sm(first_frame=-1) == raw_sm(first_sample=2 ** 32 - S + 1) == -1
    assert raw_sm(first_frame=2 ** 32 - F + 1) == -1
    assert raw_sm(upward=None) == raw_sm(taps=None) == raw_sm(no_tree=True) == raw_sm(index=None) == raw_sm(kind=None) == -1
    assert raw_sm(scratch=None) == raw_sm(scratch=ss[4:], scratch_bytes=need) == -1                          # 4-byte aligned: not enough
    assert raw_sm(index=out["index"].view(torch.uint8).reshape(-1)[2:]) == -1                                            # misaligned
    torch.cuda.synchronize()
    assert all(bool((t == -5).all()) for t in out.values())
    # ... and take what is in range: the last offsets, valid = NULL
    assert raw_sm(first_sample=2 ** 32 - S, first_frame=2 ** 32 - F, valid_=None) == 0 and raw_up() == 0
    torch.cuda.synchronize()
    assert not bool((out["index"] == -5).any()) and not bool((out["kind"] == -5).any()) and bool((out["valid"] == 1).all())
    assert same_bits(out["upward"].cpu().numpy(), A.cpu().numpy()) and same_bits(out["sums"].cpu().numpy(), sums.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ 7. public surface
BONES = np.linspace(0.15, 0.45, 14)
KEYS = ("index", "coord", "kind", "valid", "sampled", "mean", "spread", "bone_error")


@pytest.fixture(scope="module")
def net64():
    net = VoxelNetwork_depth(load_config(), device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def two_forwards(net64):
    """Two B = 2 forwards: [(joints, volumes)] cloned."""
    out = []
    for seed in (31, 32):
        img, depth = synth.make_inputs(seed, 2, "floor")
        with torch.no_grad():
            kp, _, vols, _ = net64(img.to(DEV), net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth.to(DEV))
        out.append((kp.clone(), vols.clone()))
    torch.cuda.synchronize()
    return out


def test_module_sample_equals_the_library_calls(net64, two_forwards):
    G, J = net64.volume_size, 15
    N = G ** 3
    sp = net64.skeleton_prior(BONES)
    res = [sp.sample(vols, samples=4, seed=11, first_frame=2 * n, joints=kp, return_upward=True)
           for n, (kp, vols) in enumerate(two_forwards)]
    torch.cuda.synchronize()
    for r in res:
        assert tuple(r) == KEYS + ("shift", "upward", "sums")
        assert tuple(r["index"].shape) == tuple(r["kind"].shape) == tuple(r["valid"].shape) == (4, 2, J) and r["index"].dtype == torch.int32
        assert tuple(r["coord"].shape) == (4, 2, J, 3) and tuple(r["mean"].shape) == (2, J, 3) and tuple(r["spread"].shape) == (2, J)
        assert tuple(r["bone_error"].shape) == (4, 2, J - 1) and tuple(r["shift"].shape) == (2, J) and r["sampled"].dtype == torch.bool
        assert tuple(r["upward"].shape) == (2, J, G, G, G) and tuple(r["sums"].shape) == (2, J) and r["valid"].dtype == torch.bool
    vols = torch.cat([v for _, v in two_forwards]).reshape(4, J, N)
    taps = torch.from_numpy(shell_taps(np.concatenate([[0.0], BONES]), 0.03, net64.cuboid_side / G, sp.radius)).to(DEV)
    A, sums, valid = upward_dev(vols, taps, TREE, G, sp.radius, 1e-3)
    gi, gk = sample_dev(A, valid, taps, TREE, G, sp.radius, 1e-3, 4, seed=11)
    assert same_bits(torch.cat([r["upward"] for r in res]).reshape(4, J, N).cpu().numpy(), A.cpu().numpy())
    assert same_bits(torch.cat([r["sums"] for r in res]).cpu().numpy(), sums.cpu().numpy())
    index = torch.cat([r["index"] for r in res], dim=1).cpu().numpy()
    assert np.array_equal(index, gi) and np.array_equal(torch.cat([r["kind"] for r in res], dim=1).cpu().numpy(), gk)
    assert np.array_equal(torch.cat([r["sampled"] for r in res]).cpu().numpy(), valid.cpu().numpy() != 0) and valid.cpu().numpy().all()
    # what is formed from the index, in numpy float64 from the float32 voxel centres
    coord = net64.coord_volumes[0].reshape(N, 3).float().cpu().numpy().astype(np.float64)
    ok = index >= 0
    assert ok.all() and np.array_equal(torch.cat([r["valid"] for r in res], dim=1).cpu().numpy(), ok)
    xyz = coord[index]
    got = {key: torch.cat([r[key] for r in res], dim=1 if key in ("coord", "bone_error") else 0).cpu().numpy()
           for key in ("coord", "mean", "spread", "bone_error", "shift")}
    assert np.array_equal(got["coord"].astype(np.float64), xyz)
    # float32 arithmetic on coordinates below 2 m: a sum of four and a division, 16 roundings of 2^-24 x 2 m at the most; the
    # differences, squares and root behind the spread and the bone error keep that absolute size (a root halves a relative error)
    tol = 16 * U * 2.0
    assert np.abs(got["mean"] - xyz.mean(axis=0)).max() <= tol
    spread = np.sqrt(((xyz - xyz.mean(axis=0)) ** 2).sum(axis=-1).sum(axis=0) / 3.0)
    assert np.abs(got["spread"] - spread).max() <= 4 * tol
    bone = np.abs(np.linalg.norm(xyz[:, :, 1:] - xyz[:, :, list(TREE[1:])], axis=-1) - BONES.astype(np.float32))
    assert np.abs(got["bone_error"] - bone).max() <= 4 * tol
    kp = torch.cat([k for k, _ in two_forwards]).cpu().numpy().astype(np.float64)
    assert np.abs(got["shift"] - np.linalg.norm(xyz.mean(axis=0) - kp, axis=-1)).max() <= 4 * tol
    frames = op.skeleton_samples_to_numpy(res[0])
    assert len(frames) == 2 and tuple(frames[0]) == ("index", "coord", "kind", "valid", "bone_error", "mean", "spread", "sampled", "shift")
    assert frames[1]["coord"].shape == (4, J, 3) and frames[1]["valid"].shape == (4, J) and frames[1]["spread"].shape == (J,)
    assert frames[1]["bone_error"].shape == (4, J - 1) and bool(frames[1]["sampled"])
    centre = xyz.mean(axis=0)[:2]
    both = metrics.best_pose_of_samples(frames, kp[:2], centre)
    each = metrics.best_of_samples(frames, kp[:2], centre)
    assert each["best_of_n_mpjpe"] <= both["best_pose_of_n_mpjpe"] and both["whole_poses"] == 8
    print(f"synthetic weights: mean spread {float(got['spread'].mean()):.4f} m, mean bone error {float(got['bone_error'].mean()):.4f} m, "
          f"kinds {np.bincount(gk.reshape(-1), minlength=3).tolist()}")


def test_nine_frames_in_one_call_are_eight_and_one(net64, two_forwards):
    """B = 9 walks two groups inside SkeletonPrior.sample: the bits of B = 8 and B = 1 with first_frame = 8."""
    assert SAMPLE_GROUP == 8
    sp = net64.skeleton_prior(BONES)
    four = torch.cat([v for _, v in two_forwards])
    nine = torch.cat([four, four, four[:1]]).contiguous()
    whole = sp.sample(nine, samples=3, seed=5)
    head = sp.sample(nine[:8], samples=3, seed=5)
    tail = sp.sample(nine[8:], samples=3, seed=5, first_frame=8)
    torch.cuda.synchronize()
    assert tuple(whole) == KEYS and tuple(whole["index"].shape) == (3, 9, 15)
    for key in ("index", "kind", "coord", "bone_error", "valid"):
        assert torch.equal(whole[key], torch.cat([head[key], tail[key]], dim=1)), key
    for key in ("sampled", "mean", "spread"):
        assert torch.equal(whole[key], torch.cat([head[key], tail[key]], dim=0)), key
    # the same volumes at another frame number are other draws
    assert not torch.equal(whole["index"][:, 0], whole["index"][:, 4])


def test_run_sequence_pose_samples(tmp_path, capsys):
    import evaluate
    import run_sequence
    demo_exr = os.path.join(GOLD, "demo", "img_001000.jpg.exr")
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 3, [demo_exr], estimated_depth_name="est_depth", seed=5)
    cfg_path = tmp_path / "batch2.yaml"
    with open(os.path.join(os.path.dirname(GOLD), "..", "experiments", "sceneego", "test", "sceneego.yaml")) as f:
        text = f.read()
    assert text.count("  batch_size: 8\n") == 1
    cfg_path.write_text(text.replace("  batch_size: 8\n", "  batch_size: 2\n"))
    np.save(tmp_path / "bones.npy", BONES)
    common = ["--config", str(cfg_path), "--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth",
              "--weights", "synthetic"]
    res = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl"), "--pose_samples_output", str(tmp_path / "s" / "ps.pkl"),
                                      "--pose_samples", "4", "--pose_sample_seed", "3", "--bone_lengths", str(tmp_path / "bones.npy")])
    out = capsys.readouterr().out
    assert "pose samples" in out.splitlines()[-1] and "best-of-4" in out.splitlines()[-1]
    with open(tmp_path / "s" / "ps.pkl", "rb") as f:
        frames = pickle.load(f)
    summary = res["pose_samples_summary"]
    assert len(frames) == 3 and res["pose_samples"] is not None and np.isfinite(summary["best_pose_of_n_mpjpe"])
    assert "best_of_n_mpjpe" not in res                                               # the trajectory sampler's names stay its own
    for fr in frames:
        assert tuple(fr) == ("index", "coord", "kind", "valid", "bone_error", "mean", "spread", "sampled", "shift")
        assert fr["coord"].shape == (4, 15, 3) and fr["valid"].shape == (4, 15) and fr["spread"].shape == (15,) and fr["valid"].all()
    assert summary["best_of_n_mpjpe"] <= summary["best_pose_of_n_mpjpe"] and np.isfinite(summary["mean_bone_error"])
    # driving SkeletonPrior.sample by hand on the same volumes with the running frame count gives the same draws
    from sceneego_amd.jpeg_device import JpegFile
    runner = run_sequence.SequenceRunner(load_config(str(cfg_path)), weights="synthetic")
    images, _, depths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    sp = runner.net.skeleton_prior(BONES, tau=0.03, floor=1e-3)
    by_hand = []
    for i in range(0, 3, 2):
        img = runner._images([JpegFile(p) for p in images[i:i + 2]])
        depth = runner._depths(depths[i:i + 2])
        with torch.no_grad():
            kp, _, vol, _ = runner.net(img, runner.net.grid_coord_proj_batch, runner.net.coord_volumes, depth_map_batch=depth)
        by_hand.extend(op.skeleton_samples_to_numpy(sp.sample(vol, samples=4, seed=3, first_frame=i, joints=kp)))
    assert len(by_hand) == 3 and all(np.array_equal(a["index"], b["index"]) for a, b in zip(by_hand, frames))
    # evaluate.py --pose_samples reads the pickle, without and with a ground truth
    alone = evaluate.main(["--pred_dir", str(tmp_path / "plain.pkl"), "--pose_samples", str(tmp_path / "s" / "ps.pkl")])
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((3, 15, 3)), f)
    both = evaluate.main(["--pred_dir", str(tmp_path / "plain.pkl"), "--gt", str(tmp_path / "gt.pkl"), "--pose_samples",
                          str(tmp_path / "s" / "ps.pkl")])
    text = capsys.readouterr().out
    assert "pose samples" in text and "per whole pose" in text
    assert alone["pose_samples"]["samples_per_frame"] == 4 and np.isfinite(alone["pose_samples"]["mean_sample_spread"])
    assert np.isclose(alone["pose_samples"]["mean_bone_error"], np.mean([fr["bone_error"] for fr in frames]), rtol=1e-6)
    assert both["pose_samples"]["best_of_n_mpjpe"] <= both["pose_samples"]["best_pose_of_n_mpjpe"]
    with pytest.raises(SystemExit):
        run_sequence.main(common + ["--pose_samples", "4"])
    with pytest.raises(SystemExit):
        run_sequence.main(common + ["--pose_samples_output", str(tmp_path / "x.pkl"), "--pose_samples", "0"])
