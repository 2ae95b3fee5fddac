"""GPU: the edge statistics of the skeleton model (csrc/skeleton_prior.hip: se_shell_moments_f32, se_skeleton_edge_stats_f32) against
their float64 model (tests/skeleton_fit_model.py), their bitwise agreement with se_skeleton_couple_f32, their independence of how
frames are batched, the invalid frame, the bad arguments, SkeletonModelFit and the command line.

TOLERANCE (derived as the header of tests/test_gpu_skeleton_prior.py derives its own; u = 2^-24).  All inputs are non-negative, so
relative errors add and never cancel.
se_shell_moments_f32 alone, from given volumes and taps: each of the three correlation values is a chain of at most T(R) =
_lib.SHELL_CHAIN(R) fused multiply-adds, the reduction behind it one of at most M = _lib.MOMENT_CHAIN(G) roundings (the lane's four
fused multiply-adds with e(x), the workgroup fold, the fold of the records; the header states the order), and 2 more cover the
conversion of the result:
    |got - want| <= (T(R) + M + 2) u want.
se_skeleton_edge_stats_f32: s, t, Z are that file's normalisers, within its bound B = belief_bound(parents, R) (the evidence bound: the
magnitudes of the errors of the messages into a joint sum to at most 2 (J - 1) e_msg over their disjoint subtrees).  S0, S1, S2 are
sums over pairs of E_c(x) w(d) A_c(x + d): E_c and A_c are products of messages from the two disjoint sides of edge c, so the same
sum over edges bounds their error by B, and the moment's own arithmetic adds (T(R) + M + 2) u.  SJ = (uniform t) s carries the errors
of t and s (each within B's sum over its own side of the edge, together within B) and three roundings.  So every entry of stats and
norms is held to
    B_fit = B + (T(R) + M + 2) u
relative, and so is identity one, (1 - floor) S0 + SJ = s_c Z_parent(c), formed in float64 from the float32 outputs.
"""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD
from sceneego_amd import _lib, skeleton_fit, synth
from sceneego_amd.skeleton_fit import SkeletonModelFit, cut_support, support_taps
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS
from skeleton_fit_model import edge_stats_model, shell_moments_model
from skeleton_prior_cases import CHAIN3, SIDE, make_logits
from test_gpu_skeleton_prior import CASES, TREES, belief_bound, case, launch, production, same_bits, softmax_on_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TREE = KINEMATIC_PARENTS


def moment_bound(G, R):
    return (_lib.SHELL_CHAIN(R) + _lib.MOMENT_CHAIN(G) + 2) * U


def fit_bound(parents, G, R):
    return belief_bound(parents, R) + moment_bound(G, R)


def test_the_chain_length_mirrors_the_header():
    with open(os.path.join(os.path.dirname(GOLD), "..", "include", "sceneego_hip.h")) as f:
        text = f.read()
    assert "#define SE_SK_MOMENT_CHAIN(G) (18 + ((G) * (((G) + 15) / 16) * (((G) + 63) / 64) + 63) / 64)" in text
    assert _lib.MOMENT_CHAIN(64) == 22 and _lib.MOMENT_CHAIN(128) == 50 and _lib.MOMENT_CHAIN(6) == 19 and _lib.ABI_VERSION >= 39


# ------------------------------------------------------------------------------------------------------------------ 1. the moments
def three_blocks(lengths_vox, tau_vox, G, R):
    h = SIDE / G
    lengths = np.concatenate([[0.0], np.asarray(lengths_vox, dtype=np.float64) * h])
    return support_taps(cut_support(lengths, tau_vox * h, h, R), lengths, tau_vox * h)


def moments(e, a, blocks, tap_row, G, R):
    rows = e.shape[0]
    out = torch.full((rows, 3), float("nan"), device=DEV)
    dev = [torch.from_numpy(np.ascontiguousarray(b)).to(DEV) for b in blocks]
    _lib.shell_moments(torch.from_numpy(e).to(DEV), torch.from_numpy(a).to(DEV), dev[0], dev[1], dev[2],
                       torch.tensor(tap_row, device=DEV, dtype=torch.int32), out, rows, G, R)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_moments(got, e, a, blocks, tap_row, G, R, what, method="direct"):
    bound = moment_bound(G, R)
    worst = 0.0
    for r, tr in enumerate(tap_row):
        want = np.array(shell_moments_model(e[r].astype(np.float64), a[r].astype(np.float64), blocks[0][tr], blocks[1][tr], blocks[2][tr],
                                            G, R, method))
        assert (want[[0, 2]] > 0).all() and want[1] >= 0
        err = np.abs(got[r].astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(want, 1e-300)).max()) / bound)
        assert (err <= bound * want).all(), (what, r, got[r], want)
    print(f"{what}: bound {bound / U:.0f} u; worst case {worst:.4f} of the bound")


# G, R, bone lengths in voxels (one block each), tau in voxels
MOMENT_SHAPES = [(6, 5, (3.4, 1.2), 0.5), (10, 4, (2.4, 1.0), 0.5), (17, 6, (4.4, 2.0, 0.4), 0.5), (68, 3, (1.4, 0.9), 0.5)]


@pytest.mark.parametrize("G,R,bones,tau", MOMENT_SHAPES)
def test_shell_moments_against_float64(G, R, bones, tau):
    """Positive inputs; G = 6, R = 5: every window clipped; G = 17: a ragged 16-row tile; G = 68: a second column chunk."""
    rng = np.random.default_rng(100 * G + R)
    blocks = three_blocks(bones, tau, G, R)
    tap_row = [1 + r % len(bones) for r in range(len(bones) + 1)]
    e = rng.uniform(0.05, 1.0, size=(len(tap_row), G ** 3)).astype(np.float32)
    a = rng.uniform(0.05, 1.0, size=(len(tap_row), G ** 3)).astype(np.float32)
    got = moments(e, a, blocks, tap_row, G, R)
    check_moments(got, e, a, blocks, tap_row, G, R, f"G {G} R {R}")


def test_shell_moments_at_the_production_shape():
    """One row at 64^3 with R = 18 and the longest shell of the production case, against the FFT form of the model."""
    G, R = 64, 18
    k = production()
    h = SIDE / G
    blocks = support_taps(cut_support(k["lengths"], 0.03, h, R), k["lengths"], 0.03)
    assert np.array_equal(blocks[0].view(np.int32), k["taps"].view(np.int32))
    rng = np.random.default_rng(6418)
    e = rng.uniform(0.05, 1.0, size=(1, G ** 3)).astype(np.float32)
    a = rng.uniform(0.05, 1.0, size=(1, G ** 3)).astype(np.float32)
    tap_row = [int(np.argmax(k["lengths"]))]
    got = moments(e, a, blocks, tap_row, G, R)
    check_moments(got, e, a, blocks, tap_row, G, R, "G 64 R 18", method="fft")


def test_shell_moments_between_the_runs_at_the_centre_and_out_of_range():
    """Block 1: a shell with a lone tap in the hollow of its central columns and another one zeroed inside a run's neighbourhood - the
    between-runs path, where every tap is tested and an exact zero of w is skipped in all three blocks although w1 and w2 are not
    zero there.  Block 2: a bone shorter than half a voxel, so that d = 0 lies inside the shell: w1 = w2 = 0 where w != 0.  Row 3
    names a block that does not exist: NaN."""
    G, R = 10, 4
    W = 2 * R + 1
    blocks = [b.copy() for b in three_blocks((3.0, 0.4), 0.3, G, R)]
    centre = ((R * W) + R) * W + R
    assert blocks[0][1, centre] == 0 and blocks[0][2, centre] != 0 and blocks[1][2, centre] == 0 and blocks[2][2, centre] == 0
    lone = ((R * W) + R + 1) * W + R                                       # d = (0, 1, 0): inside the hollow of a 3-voxel shell
    gap = ((R * W) + R - 1) * W + R                                        # d = (0, -1, 0): stays an exact zero of w
    assert blocks[0][1, lone] == 0 and blocks[0][1, gap] == 0
    blocks[0][1, lone], blocks[1][1, lone], blocks[2][1, lone] = 0.01, 0.002, 0.0004
    blocks[1][1, gap], blocks[2][1, gap] = 0.5, 0.25                       # must be skipped: w is zero here
    rng = np.random.default_rng(5)
    e = rng.uniform(0.05, 1.0, size=(3, G ** 3)).astype(np.float32)
    a = rng.uniform(0.05, 1.0, size=(3, G ** 3)).astype(np.float32)
    got = moments(e, a, blocks, [1, 2, 3], G, R)
    assert np.isnan(got[2]).all()
    check_moments(got[:2], e[:2], a[:2], blocks, [1, 2], G, R, "between the runs, d = 0")


# ------------------------------------------------------------------------------------------------------------------ 2. the tree
def blocks_of(k, tree, G, R):
    """The three blocks that go with the taps of a case of tests/test_gpu_skeleton_prior.py."""
    if len(TREES[tree]) == 1:
        z = np.zeros((1, (2 * R + 1) ** 3), dtype=np.float32)
        return z, z, z
    h = SIDE / G
    blocks = support_taps(cut_support(k["lengths"], 0.5 * h, h, R), k["lengths"], 0.5 * h)
    assert np.array_equal(blocks[0].view(np.int32), k["taps"].view(np.int32))
    return blocks


def edge_stats(prob, blocks, parents, G, R, floor, **kw):
    F, J, N = prob.shape
    stats = torch.full((F, J, 4), float("nan"), device=DEV)
    norms = torch.full((F, J, 3), float("nan"), device=DEV)
    valid = torch.full((F,), -1, device=DEV, dtype=torch.int32)
    dev = [torch.from_numpy(np.ascontiguousarray(b)).to(DEV) for b in blocks]
    _lib.skeleton_edge_stats(prob.contiguous(), dev[0], dev[1], dev[2], parents, stats, norms, valid, F, N, G, R, floor, **kw)
    torch.cuda.synchronize()
    return stats.cpu().numpy(), norms.cpu().numpy(), valid.cpu().numpy()


def compare_stats(got, want, parents, G, R, floor, what):
    gs, gn, gv = got
    ws, wn, wv = want
    J = len(parents)
    bound = fit_bound(parents, G, R)
    assert wv.all() and np.array_equal(gv, wv.astype(np.int32))
    assert (gs[:, 0] == 0).all() and np.isnan(gn[:, 0, :2]).all()
    worst = 0.0
    if J > 1:
        assert np.nanmin(wn[:, 1:, :2]) >= 1e-12 and wn[:, :, 2].min() >= 1e-12
        assert (ws[:, 1:, :3] > 0).all() and ((ws[:, 1:, 3] > 0).all() if floor > 0 else (ws[:, 1:, 3] == 0).all())
        err = np.abs(gs[:, 1:].astype(np.float64) - ws[:, 1:])               # floor = 0: SJ is exactly 0 on both sides
        errn = np.abs(gn[:, 1:].astype(np.float64) - wn[:, 1:])
        worst = max(float((err[..., :3] / ws[:, 1:, :3]).max()), float((errn / wn[:, 1:]).max()))
        assert (err <= bound * ws[:, 1:]).all(), (what, float((err / np.maximum(ws[:, 1:], 1e-300)).max()), bound)
        assert (errn <= bound * wn[:, 1:]).all(), (what, float((errn / wn[:, 1:]).max()), bound)
        keep = float(np.float32(1.0) - np.float32(floor))
        g = gs.astype(np.float64)
        lhs = keep * g[:, 1:, 0] + g[:, 1:, 3]
        rhs = gn[:, 1:, 0].astype(np.float64) * gn[:, list(parents[1:]), 2].astype(np.float64)
        ident = np.abs(lhs - rhs) / rhs
        worst = max(worst, float(ident.max()))
        assert (ident <= bound).all(), (what, float(ident.max()), bound)
    relz = np.abs(gn[:, :, 2].astype(np.float64) - wn[:, :, 2]) / wn[:, :, 2]
    assert (relz <= bound).all()
    print(f"{what}: bound {bound / U:.0f} u; worst case {max(worst, float(relz.max())) / bound:.4f} of the bound")


@pytest.mark.parametrize("frames,tree,G,R,floor", CASES)
def test_edge_stats_against_the_model_and_the_coupling(frames, tree, G, R, floor):
    k = case(frames, tree, G, R)
    parents = k["parents"]
    blocks = blocks_of(k, tree, G, R)
    got = edge_stats(k["prob"], blocks, parents, G, R, floor)
    want = edge_stats_model(k["p"], *blocks, parents, G, floor)
    compare_stats(got, want, parents, G, R, floor, f"frames {frames} {tree} G {G} R {R} floor {floor}")
    _, _, evidence, coupled = launch(k["prob"], k["coord"], k["taps_dev"], parents, G, R, floor, beliefs=False)
    assert same_bits(got[1][:, :, 2], evidence) and np.array_equal(got[2], coupled)


def test_edge_stats_do_not_depend_on_how_frames_are_batched():
    G, R = 8, 4
    k = case(6, "tree15", G, R)
    blocks = blocks_of(k, "tree15", G, R)
    five = edge_stats(k["prob"][:5], blocks, TREE, G, R, 1e-3)
    one, four = edge_stats(k["prob"][:1], blocks, TREE, G, R, 1e-3), edge_stats(k["prob"][1:5], blocks, TREE, G, R, 1e-3)
    for x in range(3):
        assert same_bits(np.concatenate([one[x], four[x]]), five[x]), x
    assert five[2].all()


def test_a_nan_makes_only_its_own_frame_invalid():
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    blocks = blocks_of(k, "tree15", G, R)
    clean = edge_stats(k["prob"], blocks, TREE, G, R, 1e-3)
    prob = k["prob"].clone()
    prob[1, 9, 345] = float("nan")
    got = edge_stats(prob, blocks, TREE, G, R, 1e-3)
    assert got[2].tolist() == [1, 0, 1] and clean[2].tolist() == [1, 1, 1]
    for x in range(3):
        assert same_bits(got[x][[0, 2]], clean[x][[0, 2]]), x
    assert np.isnan(got[0][1]).any()                                         # written as computed
    _, _, evidence, coupled = launch(prob, k["coord"], k["taps_dev"], TREE, G, R, 1e-3, beliefs=False)
    assert same_bits(got[1][:, :, 2], evidence) and np.array_equal(got[2], coupled)


def test_bad_arguments_raise_and_do_not_launch():
    import ctypes
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    N, J = G ** 3, 15
    prob = k["prob"][:2].contiguous()
    dev = [torch.from_numpy(np.ascontiguousarray(b)).to(DEV) for b in blocks_of(k, "tree15", G, R)]

    def call(**kw):
        a = {"prob": prob, "taps": dev[0], "taps_r": dev[1], "taps_r2": dev[2], "parents": TREE,
             "stats": torch.empty((2, J, 4), device=DEV), "norms": torch.empty((2, J, 3), device=DEV),
             "valid": torch.empty((2,), device=DEV, dtype=torch.int32), "frames": 2, "voxels": N, "grid": G, "radius": R, "floor": 1e-3}
        a.update(kw)
        return _lib.skeleton_edge_stats(**a)

    call()
    bad_tree = list(TREE)
    bad_tree[5] = 5
    for kw in ({"radius": 25}, {"radius": G}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0}, {"frames": 3}, {"grid": G + 1},
               {"voxels": N + 1}, {"parents": bad_tree}, {"parents": []}, {"prob": prob.cpu()}, {"prob": prob.double()},
               {"taps_r": dev[1][:-1]}, {"taps_r2": dev[2].cpu()}, {"taps": dev[0].double()}, {"stats": torch.empty((2, J, 3), device=DEV)},
               {"norms": torch.empty((2, J, 4), device=DEV)}, {"valid": torch.empty((2,), device=DEV)},
               {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    e = prob[0, :2].contiguous()
    tr, out = torch.ones(2, device=DEV, dtype=torch.int32), torch.empty((2, 3), device=DEV)
    for kw in ({}, {"radius": 25}, {"radius": G}, {"grid": G + 1}, {"rows": 3}, {"rows": 0}, {"tap_row": tr.float()}, {"out": out[:1]},
               {"taps_r": dev[1][:-1]}, {"taps": dev[0].reshape(-1)}, {"a": e.cpu()}, {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        b = {"e": e, "a": prob[1, :2].contiguous(), "taps": dev[0], "taps_r": dev[1], "taps_r2": dev[2], "tap_row": tr, "out": out,
             "rows": 2, "grid": G, "radius": R}
        b.update(kw)
        if not kw:
            _lib.shell_moments(**b)
            continue
        with pytest.raises(_lib.HipExtensionError):
            _lib.shell_moments(**b)
    torch.cuda.synchronize()
    # the C entry points refuse on their own what the wrappers check first
    lib, P = _lib.load(), _lib._ptr
    st, no, va = torch.empty((2, J, 4), device=DEV), torch.empty((2, J, 3), device=DEV), torch.empty((2,), device=DEV, dtype=torch.int32)
    ws = torch.empty(_lib.skeleton_edge_stats_scratch_bytes(2, J, G, R), device=DEV, dtype=torch.uint8)
    assert ws.numel() > _lib.skeleton_couple_scratch_bytes(2, J, G, R) + 2 * J * N * 4

    def raw(radius=R, floor=1e-3, frames=2, grid=G, voxels=N, scratch_bytes=ws.numel(), parents=TREE, stats=st, scratch=ws, n=J, w2=dev[2]):
        par = (ctypes.c_int * len(parents))(*parents)
        return lib.se_skeleton_edge_stats_f32(P(prob), P(dev[0]), P(dev[1]), P(w2), ctypes.cast(par, ctypes.c_void_p), P(stats), P(no), P(va),
                                              ctypes.c_void_p(scratch.data_ptr()), scratch_bytes, frames, n, voxels, grid, radius, floor,
                                              _lib._stream())
    assert raw() == 0
    assert raw(radius=25) == raw(radius=G) == raw(floor=2.0) == raw(floor=float("nan")) == raw(frames=0) == raw(voxels=N + 4) == -1
    assert raw(grid=129) == raw(scratch_bytes=ws.numel() - 1) == raw(stats=None) == raw(parents=bad_tree) == raw(n=0) == raw(n=33) == -1
    assert raw(w2=None) == raw(scratch=ws[1:], scratch_bytes=ws.numel() - 1) == -1
    assert lib.se_skeleton_edge_stats_scratch_bytes(2, 33, G, R) == 0 and lib.se_skeleton_edge_stats_scratch_bytes(2, J, G, G) == 0
    ms = torch.empty(_lib.shell_moments_scratch_bytes(2, J, G, R), device=DEV, dtype=torch.uint8)

    def raw_m(radius=R, grid=G, rows=2, out_=out, scratch_bytes=ms.numel(), w1=dev[1]):
        return lib.se_shell_moments_f32(P(e), P(prob[1]), P(dev[0]), P(w1), P(dev[2]), P(tr), P(out_), P(ms), scratch_bytes, rows, J, grid,
                                        radius, _lib._stream())
    assert raw_m() == 0
    assert raw_m(radius=25) == raw_m(radius=G) == raw_m(grid=1) == raw_m(rows=0) == raw_m(out_=None) == raw_m(scratch_bytes=8) == -1
    assert raw_m(w1=None) == -1 and lib.se_shell_moments_scratch_bytes(0, J, G, R) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 3. the fit
@functools.lru_cache(maxsize=None)
def fit_case(name):
    """chain16: the host tests' 3-chain at 16^3 (bones of 4.3 and 4.9 voxels started 0.46 and 0.66 off, tau0 one voxel, R = 9, four
    frames).  tree64: two frames of the 15-joint tree at 64^3, tau 0.03 m, bones 0.15 - 0.45 m, R = 18."""
    if name == "chain16":
        G, h, parents = 16, SIDE / 16, CHAIN3
        truth = np.array([0.0, 4.3, 4.9]) * h
        start, tau, frames, method = truth + np.array([0.0, 0.46, 0.66]) * h, h, 4, "direct"
    else:
        G, parents, tau, frames, method = 64, TREE, 0.03, 2, "fft"
        truth = start = production()["lengths"]
    coord = production()["coord"] if G == 64 else None
    logits = make_logits(frames, parents, truth, G, 1604)[0]
    if coord is None:
        from sceneego_amd import op
        coord = op.build_coord_volume(G, SIDE).reshape(G ** 3, 3).contiguous().to(DEV)
    prob = softmax_on_device(logits, coord)
    fit = SkeletonModelFit(G, SIDE, start, tau=tau, floor=1e-3, parents=parents)
    return {"G": G, "parents": parents, "start": start, "tau": tau, "prob": prob, "p": prob.cpu().numpy(), "method": method,
            "vol": prob.view(frames, len(parents), G, G, G), "fit": fit}


@pytest.mark.parametrize("name", ["chain16", "tree64"])
def test_model_fit(name):
    k = fit_case(name)
    G, parents, m = k["G"], k["parents"], k["fit"]
    J, F = len(parents), k["p"].shape[0]
    m.reset()
    m.push(k["vol"])
    assert m.frames_stored == F and m.bytes_stored == F * J * G ** 3 * 4
    # one iteration's statistics against the model
    sup = cut_support(k["start"], k["tau"], SIDE / G)
    assert sup.radius == m.radius == (9 if name == "chain16" else 18)
    blocks = support_taps(sup, k["start"], k["tau"])
    got = m.e_step(blocks, 1e-3)
    n = F if name == "chain16" else 1                     # frames are independent (and batching is tested bitwise): one is enough at 64^3
    want = edge_stats_model(k["p"][:n], *blocks, parents, G, 1e-3, method=k["method"])
    compare_stats(tuple(x[:n] for x in got), want, parents, G, m.radius, 1e-3, name)
    assert got[2].all()
    # three iterations do not lower the likelihood beyond what the bound on s and Z allows
    fit = m.fit(iterations=3, tol=0.0)
    ll = fit["log_likelihood"]
    slack = 2 * F * J * fit_bound(parents, G, m.radius)
    print(name, "log-likelihood", ll, "tau", fit["tau"], "floor", fit["floor"], "lengths", fit["bone_lengths"][1:])
    assert sorted(fit) == sorted(skeleton_fit.FIT_KEYS) and len(ll) == 4 and fit["frames_used"] == F
    for a, b in zip(ll, ll[1:]):
        assert b >= a - slack, ll
    assert ll[-1] > ll[0]
    # the result does not depend on how the frames were pushed
    m.reset()
    for f in range(F):
        m.push(k["vol"][f:f + 1])
    again = m.fit(iterations=1, tol=0.0)
    assert again["log_likelihood"] == ll[:2] and again["tau"] == fit["history"][1]["tau"] and again["floor"] == fit["history"][1]["floor"]
    assert again["bone_lengths"][1:].tolist() == fit["history"][1]["bone_lengths"]
    m.reset()
    assert m.frames_stored == 0


def test_a_push_over_the_budget_is_refused_with_nothing_allocated():
    k = fit_case("chain16")
    frame = 3 * 16 ** 3 * 4
    m = SkeletonModelFit(16, SIDE, k["start"], tau=k["tau"], parents=CHAIN3, max_bytes=2 * frame)
    m.push(k["vol"][:2])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="max_bytes"):
        m.push(k["vol"][2:3])
    assert torch.cuda.memory_allocated() == before and m.frames_stored == 2
    with pytest.raises(ValueError):
        m.push(k["vol"][:1, :2])


# ------------------------------------------------------------------------------------------------------------------ 4. command line
def test_run_sequence_skeleton_fit(tmp_path, capsys):
    import run_sequence
    from sceneego_amd import load_config
    from sceneego_amd.jpeg_device import JpegFile
    bones = np.linspace(0.15, 0.45, 14)
    demo_exr = os.path.join(GOLD, "demo", "img_001000.jpg.exr")
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 3, [demo_exr], estimated_depth_name="est_depth", seed=5)
    cfg_path = tmp_path / "batch2.yaml"
    with open(os.path.join(os.path.dirname(GOLD), "..", "experiments", "sceneego", "test", "sceneego.yaml")) as f:
        text = f.read()
    assert text.count("  batch_size: 8\n") == 1
    cfg_path.write_text(text.replace("  batch_size: 8\n", "  batch_size: 2\n"))
    np.save(tmp_path / "bones.npy", bones)
    common = ["--config", str(cfg_path), "--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth",
              "--weights", "synthetic", "--bone_lengths", str(tmp_path / "bones.npy")]
    plain = run_sequence.main(common + ["--skeleton_output", str(tmp_path / "a" / "coupled.pkl"),
                                        "--skeleton_info_output", str(tmp_path / "a" / "info.pkl")])
    res = run_sequence.main(common + ["--skeleton_output", str(tmp_path / "b" / "coupled.pkl"), "--skeleton_info_output",
                                      str(tmp_path / "b" / "info.pkl"), "--map_info_output", str(tmp_path / "b" / "map.pkl"),
                                      "--skeleton_fit_frames", "3", "--skeleton_fit_iterations", "2", "--skeleton_fit_output",
                                      str(tmp_path / "b" / "fit.json")])
    out = capsys.readouterr().out
    assert "skeleton model fitted to 3 frames" in out and "bone lengths fitted:" in out
    with open(tmp_path / "b" / "fit.json") as f:
        fit = json.load(f)
    assert set(skeleton_fit.FIT_KEYS) | {"frames", "start"} == set(fit) and fit["frames"] == 3 and fit["frames_used"] == 3
    assert fit["start"]["bone_lengths"] == bones.tolist() and fit["start"]["tau"] == 0.03 and fit["start"]["floor"] == 1e-3
    assert len(fit["log_likelihood"]) == 3 and len(fit["bone_lengths"]) == 15 and fit["radius"] == 18
    assert fit["log_likelihood"][-1] > fit["log_likelihood"][0]
    assert "skeleton_fit" not in plain and res["skeleton_fit"]["tau"] == fit["tau"]
    # the main pass ran on the fitted values and the info pickles record them; without the flag nothing is recorded
    with open(tmp_path / "a" / "info.pkl", "rb") as f:
        info_a = pickle.load(f)
    with open(tmp_path / "b" / "info.pkl", "rb") as f:
        info_b = pickle.load(f)
    with open(tmp_path / "b" / "map.pkl", "rb") as f:
        info_map = pickle.load(f)
    assert tuple(info_a[0]) == ("joints", "evidence", "coupled", "bone_error", "shift", "bone_error_before")
    for fr in info_b + info_map:
        assert fr["tau"] == fit["tau"] and fr["floor"] == fit["floor"] and fr["bone_lengths"].tolist() == fit["bone_lengths"][1:]
    # both passes equal SkeletonPrior.couple driven by hand on the same volumes, bit for bit: on the start and on the fitted values
    runner = run_sequence.SequenceRunner(load_config(str(cfg_path)), weights="synthetic")
    images, _, depths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    priors = (runner.net.skeleton_prior(bones, tau=0.03, floor=1e-3),
              runner.net.skeleton_prior(fit["bone_lengths"], tau=fit["tau"], floor=fit["floor"]))
    by_hand = ([], [])
    for i in range(0, 3, 2):
        img = runner._images([JpegFile(p) for p in images[i:i + 2]])
        depth = runner._depths(depths[i:i + 2])
        with torch.no_grad():
            kp, _, vol, _ = runner.net(img, runner.net.grid_coord_proj_batch, runner.net.coord_volumes, depth_map_batch=depth)
        for sp, acc in zip(priors, by_hand):
            acc.extend(sp.couple(vol, joints=kp)["joints"].cpu().numpy())
    for name, want in zip("ab", by_hand):
        with open(tmp_path / name / "coupled.pkl", "rb") as f:
            got = pickle.load(f)
        assert len(got) == 3 and all(same_bits(g, w) for g, w in zip(got, want)), name
    assert not all(same_bits(a, b) for a, b in zip(*by_hand))
    with pytest.raises(SystemExit):
        run_sequence.main(common + ["--skeleton_fit_iterations", "2"])
