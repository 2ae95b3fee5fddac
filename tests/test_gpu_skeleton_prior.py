"""GPU: the skeleton-coupled joints (csrc/skeleton_prior.hip: se_skeleton_couple_f32, se_shell_correlate_f32) against their float64
model (tests/skeleton_prior_model.py), their independence of how frames are batched, the fallback, the public surface and the command
line.

Inputs (tests/skeleton_prior_cases.py): a random pose with the case's bone lengths, one bump of logits per joint, odd joints with a
second static bump, 0.01 noise, softmaxed by se_softargmax3d_f32 on the device.

TOLERANCE (derived, not measured).  u = 2^-24.  Every term of the recursion is non-negative, so relative errors add and never cancel
badly.  One message  M = (1 - floor) corr(A, w) / sum A + floor / N  computed from given factors costs at most
    e_msg = (T(R) + L + c) u
relative: T(R) = _lib.SHELL_CHAIN(R) roundings on the longest chain of one correlation output (the kernel's header states the order),
L = _lib.SKELETON_SUM_CHAIN for the row sum, c = 8 + the largest number of children for the products (one rounding per factor), the
division, 1 - floor, floor / N and the final fused multiply-add.
How the errors of the incoming messages pass through one: write the computed A as A (1 + alpha(x)).  Both corr(A, w)(x) and sum A are
averages of A with non-negative weights, so their relative errors kappa(x) and sigma lie between min alpha and max alpha, and the error
of the quotient, kappa(x) - sigma, is bounded by the SPREAD max alpha - min alpha: a factor common to all voxels - the scalar error of
a normaliser - cancels.  The spread of a product of messages is at most the sum of their spreads, and mixing with the floor (whose own
error is one rounding) keeps the error of a value between that of the shell term and 0, which the interval [min, max] of kappa -
sigma already holds up to the L u of the sum.  With osc(M) the spread of a message's error this gives
    osc(M_j) <= sum over the incoming messages of osc + 2 e_msg        |error(M_j)| <= sum over the incoming of osc + e_msg
(the rounding errors themselves enter a spread with both signs: 2 e_msg).  The tree has J - 1 edges and every belief is fed by exactly
one message per edge, so T_j = p_j D_j prod U_c carries a spread of at most 2 (J - 1) e_msg, and b_j = T_j / Z_j - once more a value
over an average - is off by at most that spread plus its own sum and division, below one more e_msg:
    beliefs    |got - want| <= B want + 2^-90,   B = 1.01 (2 (J - 1) + 1) e_msg       (k = 2: the constant of this derivation; 1.01
               covers the second-order terms, B stays below 0.01; the absolute term: float32 underflow, denormals flushed or not)
    evidence   relative B: the magnitudes |error(M)| of the messages into j sum to at most (2 (J - 1) - deg j) e_msg over their
               disjoint subtrees, plus L u for the sum Z_j itself
    joints     absolute (B + (L + 2) u) sum b |c| per axis, the sum b |c| form of the filter test: the beliefs' bound and the
               joint's own float32 sum and division
    coupled    exact
se_shell_correlate_f32 alone: (nnz + 2) u relative, componentwise, nnz the non-zero taps of the row's block (T(R) <= nnz; the division
and the fused multiply-add).
The model's condition on the inputs is asserted with every case: each s, t, Z is >= 1e-12 and no frame falls back.
"""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD, synthetic_state_dict
from sceneego_amd import _lib, load_config, op, synth
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, SkeletonPrior, shell_taps
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
from skeleton_prior_cases import CHAIN3, SIDE, STAR5, lengths_for, make_logits, taps_for
from skeleton_prior_model import corr_direct, skeleton_couple_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
L = _lib.SKELETON_SUM_CHAIN
TREE = KINEMATIC_PARENTS
TREES = {"chain3": CHAIN3, "tree15": TREE, "star5": STAR5, "one": (0,)}

# frames, tree, G, R, floor
CASES = [
    (1, "chain3", 8, 3, 0.0),
    (2, "tree15", 8, 4, 1e-3),
    (1, "tree15", 6, 5, 1e-3),          # R = G - 1: every window clipped on both sides
    (3, "tree15", 10, 4, 1e-3),         # G % 4 = 2
    (2, "tree15", 16, 6, 0.0),
    (2, "tree15", 16, 6, 1e-3),
    (1, "star5", 8, 3, 1e-3),           # four children: the general product loop
    (1, "one", 8, 0, 0.0),
]


def e_msg(parents, R):
    kids = max(sum(1 for c in range(1, len(parents)) if parents[c] == j) for j in range(len(parents)))
    return (_lib.SHELL_CHAIN(R) + L + 8 + kids) * U


def belief_bound(parents, R):
    return 1.01 * (2 * (len(parents) - 1) + 1) * e_msg(parents, R)


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
    below modifies them)."""
    parents = TREES[tree]
    N = G ** 3
    seed = 1000 * G + 10 * len(parents) + R
    lengths = lengths_for(parents, G, R, seed)
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    prob = softmax_on_device(make_logits(frames, parents, lengths, G, seed)[0], coord)
    taps = taps_for(lengths, G, R) if len(parents) > 1 else np.zeros((1, (2 * R + 1) ** 3), dtype=np.float32)
    return {"prob": prob, "coord": coord, "p": prob.cpu().numpy(), "c": coord.cpu().numpy(), "taps": taps, "parents": parents,
            "taps_dev": torch.from_numpy(taps).to(DEV), "lengths": lengths}


def launch(prob, coord, taps, parents, G, R, floor, beliefs=True):
    """One _lib-level call over all frames of ``prob`` [F, J, N]: host arrays (beliefs, joints, evidence, coupled)."""
    F, J, N = prob.shape
    out = torch.empty_like(prob) if beliefs else None
    joints = torch.full((F, J, 3), float("nan"), device=DEV)
    evidence = torch.full((F, J), float("nan"), device=DEV)
    coupled = torch.full((F,), -1, device=DEV, dtype=torch.int32)
    _lib.skeleton_couple(prob.contiguous(), coord, taps, parents, out, joints, evidence, coupled, F, N, G, R, floor)
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), joints.cpu().numpy(), evidence.cpu().numpy(), coupled.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_condition(norms, coupled):
    """The condition on the inputs, on the model: a bad seed cannot hide."""
    small = min(float(np.nanmin(norms[k])) for k in ("s", "t", "Z") if np.isfinite(norms[k]).any())
    assert coupled.all() and small >= 1e-12, f"a normaliser of {small}"
    return small


def compare(k, got, want, R, what, beliefs=True):
    gb, gj, ge, gc = got
    wb, wj, we, wc, norms = want
    small = check_condition(norms, wc)
    assert np.array_equal(gc, wc.astype(np.int32))
    B = belief_bound(k["parents"], R)
    assert B < 0.01
    sabs = np.einsum("fjn,na->fja", wb, np.abs(k["c"].astype(np.float64)))
    worst = {}
    if beliefs:
        err = np.abs(gb.astype(np.float64) - wb)
        worst["belief"] = float((err / (wb + 2.0 ** -60)).max()) / U
    rel = np.abs(ge.astype(np.float64) - we) / we
    worst["evidence"] = float(rel.max()) / U
    jerr = np.abs(gj.astype(np.float64) - wj)
    worst["joints"] = float((jerr / sabs).max()) / U
    print(f"{what}: bound {B / U:.0f} u; worst (units of 2^-24) {worst}; smallest normaliser {small:.3g}")
    if beliefs:
        tol = B * wb + 2.0 ** -90
        assert (err <= tol).all(), f"belief off by up to {float((err - tol).max()):.3e} beyond the bound"
    assert (rel <= B).all(), f"evidence relative error {float(rel.max()):.3e} > {B:.3e}"
    assert (jerr <= (B + (L + 2) * U) * sabs).all(), f"joints off by {float((jerr / sabs).max()):.3e} sum b|c|"


# ------------------------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("frames,tree,G,R,floor", CASES)
def test_against_the_model(frames, tree, G, R, floor):
    k = case(frames, tree, G, R)
    want = skeleton_couple_model(k["p"], k["c"], k["taps"], k["parents"], G, floor)
    got = launch(k["prob"], k["coord"], k["taps_dev"], k["parents"], G, R, floor)
    compare(k, got, want, R, f"frames {frames} {tree} G {G} R {R} floor {floor}")
    # without the beliefs the other outputs are the same bits
    _, gj, ge, gc = launch(k["prob"], k["coord"], k["taps_dev"], k["parents"], G, R, floor, beliefs=False)
    assert same_bits(gj, got[1]) and same_bits(ge, got[2]) and np.array_equal(gc, got[3])


@functools.lru_cache(maxsize=None)
def production():
    """One frame of the 15-joint tree at 64^3: tau 0.03 m, bone lengths 0.15-0.45 m, R = 18."""
    G, R, tau = 64, 18, 0.03
    N, h = G ** 3, SIDE / G
    lengths = np.concatenate([[0.0], np.random.default_rng(64).permutation(np.linspace(0.15, 0.45, 14))])
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    prob = softmax_on_device(make_logits(1, TREE, lengths, G, 6418)[0], coord)
    taps = shell_taps(lengths, tau, h, R)
    assert int(np.ceil((0.45 + 3 * tau) / h)) == R
    return {"prob": prob, "coord": coord, "p": prob.cpu().numpy(), "c": coord.cpu().numpy(), "taps": taps, "parents": TREE,
            "taps_dev": torch.from_numpy(taps).to(DEV), "lengths": lengths}


def test_against_the_model_at_the_production_shape():
    """1 frame, 15-tree, 64^3, R = 18, floor 1e-3, against the FFT form of the model: joints, evidence and coupled."""
    k = production()
    want = skeleton_couple_model(k["p"], k["c"], k["taps"], TREE, 64, 1e-3, method="fft")
    got = launch(k["prob"], k["coord"], k["taps_dev"], TREE, 64, 18, 1e-3, beliefs=False)
    compare(k, got, want, 18, "production shape", beliefs=False)


# ------------------------------------------------------------------------------------------------------------------ 2. the correlation
def correlate(a, taps, tap_row, s, G, R, scale_mul, add):
    out = torch.full_like(a, float("nan"))
    _lib.shell_correlate(a, taps, tap_row, s, out, a.shape[0], G, R, scale_mul, add)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def dots(a, w, G, R, voxels):
    """corr(a, w) at the flat ``voxels`` as float64 dot products over the non-zero taps."""
    S = G + 2 * R
    pad = np.zeros((S, S, S))
    pad[R:R + G, R:R + G, R:R + G] = a.reshape(G, G, G)
    pad = pad.reshape(-1)
    W = 2 * R + 1
    w3 = np.asarray(w, dtype=np.float64).reshape(W, W, W)
    di, dj, dk = np.nonzero(w3)
    off = (di * S + dj) * S + dk                     # the tap's offset from the padded voxel (i, j, k): (i + di - R) + R
    wv = w3[di, dj, dk]
    i, j, kk = voxels // (G * G), voxels // G % G, voxels % G
    base = (i * S + j) * S + kk
    out = np.empty(len(voxels))
    for lo in range(0, len(voxels), 256):
        out[lo:lo + 256] = pad[base[lo:lo + 256, None] + off[None, :]] @ wv
    return out


def test_shell_correlation_at_the_production_shape():
    """2 rows at 64^3, R = 18, two different shells: 4096 sampled voxels and every voxel of eight whole k-rows, corner and face rows
    among them, against float64 dot products within (nnz + 2) u."""
    G, R = 64, 18
    k = production()
    N = G ** 3
    long_, short = int(np.argmax(k["lengths"])), int(np.argmin(k["lengths"][1:])) + 1
    a = k["prob"][0, :2].contiguous()
    tap_row = torch.tensor([long_, short], device=DEV, dtype=torch.int32)
    s = torch.tensor([0.37, 2.5], device=DEV)
    scale = np.float32(0.999)
    got = correlate(a, k["taps_dev"], tap_row, s, G, R, float(scale), 0.0)
    rng = np.random.default_rng(3)
    rows = [(0, 0), (0, G - 1), (G - 1, 0), (G - 1, G - 1), (0, 31), (40, G - 1), (31, 0), (20, 45)]       # (i, j): four corner rows,
    whole = np.concatenate([(i * G + j) * G + np.arange(G) for i, j in rows])                                # three face rows, one inside
    voxels = np.concatenate([rng.choice(N, size=4096, replace=False), whole])
    for r, tr in enumerate((long_, short)):
        nnz = int(np.count_nonzero(k["taps"][tr]))
        want = float(scale) * dots(k["p"][0, r].astype(np.float64), k["taps"][tr], G, R, voxels) / float(np.float32(s[r].item()))
        err = np.abs(got[r, voxels].astype(np.float64) - want)
        print(f"row {r}: {nnz} taps, chain {_lib.SHELL_CHAIN(R)}; worst {float((err / want).max()) / U:.1f} u of the {nnz + 2} u allowed")
        assert (want > 0).all() and (err <= (nnz + 2) * U * want).all()


def test_shell_correlation_every_voxel_of_a_clipped_grid():
    """G = 10, R = 9: every window is clipped; every voxel; a floor added; a tap row out of range gives NaN."""
    G, R = 10, 9
    N, h = G ** 3, SIDE / G
    taps = shell_taps([0.0, 7.4 * h, 3.2 * h], 0.5 * h, h, R)
    k = case(3, "tree15", 10, 4)
    a = k["prob"][0, :3].contiguous()
    tap_row = torch.tensor([1, 2, 3], device=DEV, dtype=torch.int32)
    s = torch.tensor([0.5, 1.5, 1.0], device=DEV)
    add = np.float32(1e-3 / N)
    got = correlate(a, torch.from_numpy(taps).to(DEV), tap_row, s, G, R, 0.75, float(add))
    assert np.isnan(got[2]).all()
    for r in (0, 1):
        nnz = int(np.count_nonzero(taps[r + 1]))
        want = 0.75 * corr_direct(k["p"][0, r].astype(np.float64), taps[r + 1], G, R) / float(np.float32(s[r].item())) + float(add)
        err = np.abs(got[r].astype(np.float64) - want)
        print(f"row {r}: {nnz} taps; worst {float((err / want).max()) / U:.1f} u of the {nnz + 2} u allowed")
        assert (err <= (nnz + 2) * U * want).all()


# ------------------------------------------------------------------------------------------------------------------ 3. batching
def test_results_do_not_depend_on_how_frames_are_batched():
    G, R = 8, 4
    k = case(6, "tree15", G, R)
    args = (k["coord"], k["taps_dev"], TREE, G, R, 1e-3)
    four = launch(k["prob"][:4], *args)
    again = launch(k["prob"][:4], *args)
    for cuts in ((1, 3), (2, 2)):
        parts, t = [], 0
        for n in cuts:
            parts.append(launch(k["prob"][t:t + n], *args))
            t += n
        for x in range(3):
            assert same_bits(np.concatenate([p[x] for p in parts]), four[x]), (cuts, x)
        assert np.array_equal(np.concatenate([p[3] for p in parts]), four[3])
    assert all(same_bits(again[x], four[x]) for x in range(3)) and four[3].all()
    # six frames walk two groups inside one call
    six = launch(k["prob"], *args)
    tail = launch(k["prob"][4:], *args)
    for x in range(3):
        assert same_bits(six[x][:4], four[x]) and same_bits(six[x][4:], tail[x]), x
    # ... and the class is the _lib-level call
    sp = SkeletonPrior(k["coord"], G, SIDE, k["lengths"], tau=0.5 * SIDE / G, floor=1e-3)
    assert sp.radius == R
    r = sp.couple(k["prob"][:4].view(4, 15, G, G, G), return_beliefs=True)
    torch.cuda.synchronize()
    assert same_bits(r["beliefs"].reshape(4, 15, -1).cpu().numpy(), four[0]) and same_bits(r["joints"].cpu().numpy(), four[1])


# ------------------------------------------------------------------------------------------------------------------ 4. fallback
def test_a_nan_makes_its_own_frame_fall_back():
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    args = (k["coord"], k["taps_dev"], TREE, G, R, 1e-3)
    clean = launch(k["prob"], *args)
    prob = k["prob"].clone()
    prob[1, 9, 345] = float("nan")
    gb, gj, ge, gc = launch(prob, *args)
    assert gc.tolist() == [1, 0, 1]
    p = prob.cpu().numpy()
    assert same_bits(gb[1], p[1])
    for x, y in zip((gb, gj, ge), clean[:3]):
        assert same_bits(x[[0, 2]], y[[0, 2]])
    c64 = k["c"].astype(np.float64)
    others = [j for j in range(15) if j != 9]
    want = p[1, others].astype(np.float64) @ c64
    sabs = p[1, others].astype(np.float64) @ np.abs(c64)
    assert (np.abs(gj[1, others] - want) <= (L + 2) * U * sabs).all() and np.isnan(gj[1, 9]).all()


def test_floor_zero_without_mass_on_the_parents_shell_falls_back():
    """floor = 0: the root's volume is a compact box and the volume of joint 1, a child of the root, is exactly zero wherever the
    root's shell reaches: Z_0 and Z_1 are exactly +0 and the frame falls back; the frame beside it is untouched."""
    G, R = 10, 4
    N = G ** 3
    k = case(3, "tree15", G, R)
    args = (k["coord"], k["taps_dev"], TREE, G, R, 0.0)
    prob = k["prob"][:2].clone()
    box = torch.zeros((G, G, G), device=DEV)
    box[4:6, 4:6, 4:6] = 0.125
    prob[0, 0] = box.reshape(-1)
    reach = corr_direct((box.reshape(1, N) > 0).double().cpu().numpy(), k["taps"][1], G, R)[0] > 0
    assert 0 < reach.sum() < N
    prob[0, 1][torch.from_numpy(reach).to(DEV)] = 0.0
    p = prob.cpu().numpy()
    assert (p[0, 1] > 0).any()
    _, _, we, wc, _ = skeleton_couple_model(p, k["c"], k["taps"], TREE, G, 0.0)
    assert wc.tolist() == [False, True] and we[0, 0] == 0.0 and we[0, 1] == 0.0
    gb, gj, ge, gc = launch(prob, *args)
    assert gc.tolist() == [0, 1]
    assert bits(ge[0, :2]).tolist() == [0, 0]                                     # exactly +0
    assert same_bits(gb[0], p[0])
    clean = launch(k["prob"][1:2], *args)
    assert all(same_bits(x[1:], y) for x, y in zip((gb, gj, ge), clean[:3]))


def test_bad_arguments_raise_and_do_not_launch():
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    N, J = G ** 3, 15
    prob = k["prob"][:2].contiguous()

    def call(**kw):
        a = {"prob": prob, "coord": k["coord"], "taps": k["taps_dev"], "parents": TREE, "beliefs": None,
             "joints": torch.empty((2, J, 3), device=DEV), "evidence": torch.empty((2, J), device=DEV),
             "coupled": torch.empty((2,), device=DEV, dtype=torch.int32), "frames": 2, "voxels": N, "grid": G, "radius": R, "floor": 1e-3}
        a.update(kw)
        return _lib.skeleton_couple(**a)

    call()
    bad_tree = list(TREE)
    bad_tree[5] = 5
    both = torch.empty((3, J, N), device=DEV)
    for kw in ({"radius": 25}, {"radius": -1}, {"radius": G}, {"floor": -0.1}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0},
               {"frames": 3}, {"grid": G + 1}, {"voxels": N + 1}, {"grid": 1, "voxels": 1, "radius": 0}, {"parents": bad_tree},
               {"parents": [1] + list(TREE[1:])}, {"parents": list(TREE) + [3]}, {"parents": [0] * 33}, {"parents": []}, {"parents": None},
               {"prob": prob.cpu()}, {"prob": prob.double()}, {"prob": prob[:, :, ::2]}, {"taps": k["taps_dev"][:-1]},
               {"taps": k["taps"]}, {"beliefs": prob}, {"beliefs": torch.empty((1, J, N), device=DEV)},
               {"prob": both[:2], "beliefs": both[1:]},
               {"coupled": torch.empty((2,), device=DEV)}, {"joints": torch.empty((2, J, 2), device=DEV)},
               {"evidence": torch.empty((2, J + 1), device=DEV)}, {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)},
               {"coord": k["coord"][:-1]}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    a = prob[0, :2].contiguous()
    tr, s, out = torch.zeros(2, device=DEV, dtype=torch.int32), torch.ones(2, device=DEV), torch.empty((2, N), device=DEV)
    _lib.shell_correlate(a, k["taps_dev"], tr, s, out, 2, G, R)
    for kw in ({"radius": 25}, {"radius": G}, {"grid": G + 1}, {"rows": 3}, {"rows": 0}, {"out": a}, {"tap_row": tr.float()},
               {"a": both[0, :2], "out": both[0, 1:3]}, {"s": s[:1]}, {"taps": k["taps_dev"].reshape(-1)}, {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        b = {"a": a, "taps": k["taps_dev"], "tap_row": tr, "s": s, "out": out, "rows": 2, "grid": G, "radius": R}
        b.update(kw)
        with pytest.raises(_lib.HipExtensionError):
            _lib.shell_correlate(**b)
    torch.cuda.synchronize()
    # the C entry points refuse on their own what the wrappers check first
    import ctypes
    lib = _lib.load()
    j, e, c = torch.empty((2, J, 3), device=DEV), torch.empty((2, J), device=DEV), torch.empty((2,), device=DEV, dtype=torch.int32)
    ws = torch.empty(_lib.skeleton_couple_scratch_bytes(2, J, G, R), device=DEV, dtype=torch.uint8)
    P = _lib._ptr

    def raw(radius=R, floor=1e-3, frames=2, grid=G, voxels=N, scratch_bytes=ws.numel(), parents=TREE, joints=j, scratch=ws, n=J):
        par = (ctypes.c_int * len(parents))(*parents)
        return lib.se_skeleton_couple_f32(P(prob), P(k["coord"]), P(k["taps_dev"]), ctypes.cast(par, ctypes.c_void_p), None, P(joints), P(e),
                                          P(c), ctypes.c_void_p(scratch.data_ptr()) if scratch is not None else None, scratch_bytes,
                                          frames, n, voxels, grid, radius, floor, _lib._stream())
    assert raw() == 0
    assert raw(radius=25) == raw(radius=G) == raw(floor=2.0) == raw(floor=float("nan")) == raw(frames=0) == raw(voxels=N + 4) == -1
    assert raw(grid=129) == raw(scratch_bytes=ws.numel() - 1) == raw(joints=None) == raw(parents=bad_tree) == raw(n=0) == raw(n=33) == -1
    assert raw(scratch=ws[1:], scratch_bytes=ws.numel() - 1) == -1               # misaligned
    assert lib.se_skeleton_couple_scratch_bytes(2, 33, G, R) == 0 and lib.se_skeleton_couple_scratch_bytes(2, J, G, G) == 0
    rs = torch.empty(_lib.shell_correlate_scratch_bytes(J, R), device=DEV, dtype=torch.uint8)

    def raw_c(radius=R, grid=G, rows=2, out_=out, scratch_bytes=rs.numel()):
        return lib.se_shell_correlate_f32(P(a), P(k["taps_dev"]), P(tr), P(s), P(out_), P(rs), scratch_bytes, rows, J, grid, radius, 1.0, 0.0,
                                          _lib._stream())
    assert raw_c() == 0
    assert raw_c(radius=25) == raw_c(radius=G) == raw_c(grid=1) == raw_c(rows=0) == raw_c(out_=a) == raw_c(scratch_bytes=8) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 5. public surface
BONES = np.linspace(0.15, 0.45, 14)


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


def test_module_prior_equals_the_library_call(net64, two_forwards):
    G, J = net64.volume_size, 15
    assert G == 64
    N = G ** 3
    sp = net64.skeleton_prior(BONES)
    assert isinstance(sp, SkeletonPrior) and sp.tau == 0.03 and sp.floor == 1e-3 and sp.parents == TREE
    assert sp.radius == int(np.ceil((0.45 + 0.09) / (net64.cuboid_side / G))) <= 24
    res = [sp.couple(vols, joints=kp, return_beliefs=True) for kp, vols in two_forwards]
    torch.cuda.synchronize()
    for r in res:
        assert tuple(r) == ("joints", "evidence", "coupled", "bone_error", "beliefs", "shift", "bone_error_before")
        assert tuple(r["joints"].shape) == (2, J, 3) and tuple(r["evidence"].shape) == (2, J) and tuple(r["beliefs"].shape) == (2, J, G, G, G)
        assert r["coupled"].dtype == torch.bool and tuple(r["coupled"].shape) == (2,) and tuple(r["shift"].shape) == (2, J)
        assert tuple(r["bone_error"].shape) == tuple(r["bone_error_before"].shape) == (2, J - 1)
        assert r["joints"].dtype == r["evidence"].dtype == r["beliefs"].dtype == r["bone_error"].dtype == torch.float32
    coord = net64.coord_volumes[0].reshape(N, 3).float().contiguous().to(DEV)
    vols = torch.cat([v for _, v in two_forwards]).reshape(4, J, N)
    taps = shell_taps(np.concatenate([[0.0], BONES]), 0.03, net64.cuboid_side / G, sp.radius)
    gb, gj, ge, gc = launch(vols, coord, torch.from_numpy(taps).to(DEV), TREE, G, sp.radius, 1e-3)
    assert same_bits(torch.cat([r["beliefs"] for r in res]).reshape(4, J, N).cpu().numpy(), gb)
    assert same_bits(torch.cat([r["joints"] for r in res]).cpu().numpy(), gj)
    assert same_bits(torch.cat([r["evidence"] for r in res]).cpu().numpy(), ge)
    assert np.array_equal(torch.cat([r["coupled"] for r in res]).cpu().numpy(), gc != 0)
    kp = torch.cat([k for k, _ in two_forwards])
    joints = torch.from_numpy(gj).to(DEV)
    assert torch.equal(torch.cat([r["shift"] for r in res]), (joints - kp).norm(dim=-1))
    par = list(TREE[1:])
    want = ((joints[:, 1:] - joints[:, par]).norm(dim=-1) - torch.from_numpy(BONES.astype(np.float32)).to(DEV)).abs()
    assert torch.equal(torch.cat([r["bone_error"] for r in res]), want)
    before, after = torch.cat([r["bone_error_before"] for r in res]), torch.cat([r["bone_error"] for r in res])
    print(f"synthetic weights: coupled {gc.tolist()}, evidence x N {ge.min() * N:.3g} .. {ge.max() * N:.3g}, "
          f"mean bone error {float(before.mean()):.4f} -> {float(after.mean()):.4f} m")
    assert gc.all() and np.isfinite(gj).all() and (ge > 0).all()
    frames = op.skeleton_couple_to_numpy(res[0])
    assert len(frames) == 2 and tuple(frames[0]) == ("joints", "evidence", "coupled", "bone_error", "shift", "bone_error_before")
    assert frames[1]["joints"].shape == (J, 3) and frames[1]["coupled"].dtype == np.bool_ and frames[1]["bone_error"].shape == (J - 1,)

    # the beliefs are volumes: the per-frame tools and the filter take them unchanged
    b = res[0]["beliefs"]
    stats = net64.joint_statistics(b, res[0]["joints"])
    modes = net64.joint_modes(b, k=4, radius=2)
    filt = net64.volume_filter().step(b)
    torch.cuda.synchronize()
    assert torch.isfinite(stats["entropy"]).all() and (modes["count"] >= 1).all()
    assert torch.equal(modes["index"][..., 0], stats["peak_index"])
    assert torch.isfinite(filt["joints"]).all() and filt["restarted"][0].all() and not filt["restarted"][1].any()


# ------------------------------------------------------------------------------------------------------------------ 6. command line
def test_run_sequence_skeleton_outputs(tmp_path, capsys):
    import evaluate
    import run_sequence
    from sceneego_amd.jpeg_device import JpegFile
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
    res = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl"), "--skeleton_output", str(tmp_path / "s" / "coupled.pkl"),
                                      "--skeleton_info_output", str(tmp_path / "s" / "info.pkl"), "--bone_lengths",
                                      str(tmp_path / "bones.npy")])
    out = capsys.readouterr().out
    assert "skeleton-coupled joints" in out.splitlines()[-1]
    with open(tmp_path / "s" / "coupled.pkl", "rb") as f:
        coupled = pickle.load(f)
    with open(tmp_path / "s" / "info.pkl", "rb") as f:
        info = pickle.load(f)
    with open(tmp_path / "plain.pkl", "rb") as f:
        preds = pickle.load(f)
    assert type(coupled) is type(preds) and len(coupled) == len(preds) == len(info) == 3
    for a, b, fr in zip(coupled, preds, info):
        assert type(a) is type(b) and a.dtype == b.dtype == np.float32 and a.shape == b.shape == (15, 3) and np.isfinite(a).all()
        assert tuple(fr) == ("joints", "evidence", "coupled", "bone_error", "shift", "bone_error_before") and np.array_equal(fr["joints"], a)
        assert np.allclose(fr["shift"], np.linalg.norm(a.astype(np.float64) - b, axis=1), rtol=1e-5, atol=1e-7)
        assert fr["coupled"] and (fr["evidence"] > 0).all()
    assert np.isfinite(res["coupled_mpjpe"]) and len(res["coupled"]) == 3 == len(res["skeleton"])
    # evaluate.py --bones reads both pickles, with and without the lengths and a ground truth
    ev = evaluate.main(["--pred_dir", str(tmp_path / "s" / "coupled.pkl"), "--bones", str(tmp_path / "bones.npy")])
    raw = evaluate.main(["--pred_dir", str(tmp_path / "plain.pkl"), "--bones", str(tmp_path / "bones.npy")])
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((3, 15, 3)), f)
    both = evaluate.main(["--pred_dir", str(tmp_path / "s" / "coupled.pkl"), "--gt", str(tmp_path / "gt.pkl"), "--bones"])
    capsys.readouterr()
    assert ev["frames"] == 3 and ev["bones"]["std"].shape == (14,) and np.isfinite(ev["bones"]["mean_deviation"])
    assert np.isclose(ev["bones"]["mean_deviation"], np.mean([fr["bone_error"] for fr in info]), rtol=1e-4)
    assert np.isclose(raw["bones"]["mean_deviation"], np.mean([fr["bone_error_before"] for fr in info]), rtol=1e-4)
    assert np.isfinite(both["mpjpe"]) and "deviation" not in both["bones"]
    # driving SkeletonPrior.couple by hand on the same volumes gives the same joints, bit for bit
    from sceneego_amd import load_config as load
    runner = run_sequence.SequenceRunner(load(str(cfg_path)), weights="synthetic")
    images, _, depths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    sp = runner.net.skeleton_prior(BONES, tau=0.03, floor=1e-3)
    by_hand = []
    for i in range(0, 3, 2):
        img = runner._images([JpegFile(p) for p in images[i:i + 2]])
        depth = runner._depths(depths[i:i + 2])
        with torch.no_grad():
            kp, _, vol, _ = runner.net(img, runner.net.grid_coord_proj_batch, runner.net.coord_volumes, depth_map_batch=depth)
        by_hand.extend(sp.couple(vol, joints=kp)["joints"].cpu().numpy())
    assert len(by_hand) == 3 and all(same_bits(a, b) for a, b in zip(by_hand, coupled))
