"""GPU: the runner-up poses (csrc/skeleton_pose.hip: se_skeleton_alternatives_f32) against their float32 numpy model
(tests/skeleton_alternatives_model.py), BIT FOR BIT: no tolerance, no case left out, every output array compared, the max-marginal
volumes included.  Then the upward outputs against se_skeleton_pose_f32's, the independence of how frames are batched, the fallback, the
production shape against the float64 score of every alternative pose, bad arguments, the public surface and the command line.

Inputs: those of tests/test_gpu_skeleton_pose.py (its cases, softmaxed on the device, computed once and shared).
"""
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD
from sceneego_amd import _lib, op
from sceneego_amd.skeleton_pose import SkeletonPose
from sceneego_amd.skeleton_prior import shell_taps
from skeleton_alternatives_model import derive, skeleton_alternatives_model
from skeleton_pose_model import pose_log_score
from skeleton_prior_cases import SIDE, make_logits
from test_gpu_skeleton_pose import BONES, CASES, DEV, TREE, case, net64, same_bits, softmax_on_device, two_forwards  # noqa: F401
from test_gpu_skeleton_pose import launch as launch_pose
from volume_viterbi_model import refine_model

pytestmark = pytest.mark.gpu
INT_KEYS = ("index", "jumped", "exponent", "solved", "down_exponent", "mm_peak", "alt_index", "alt_pose", "alt_jumped", "complete")
FLOAT_KEYS = ("best_root", "mm_best", "pose_value", "alt_value")
KEYS = INT_KEYS + FLOAT_KEYS + ("max_marginals",)


def outputs(F, J, N, fill=-7, volumes=True):
    shape = {"solved": (F,), "complete": (F,), "best_root": (F,), "alt_pose": (F, J, J), "alt_jumped": (F, J, J)}
    out = {k: torch.full(shape.get(k, (F, J)), fill, device=DEV, dtype=torch.int32) for k in INT_KEYS}
    out.update({k: torch.full(shape.get(k, (F, J)), float(fill), device=DEV) for k in FLOAT_KEYS})
    out["max_marginals"] = torch.full((F, J, N), float(fill), device=DEV) if volumes else None
    return out


def launch(prob, taps, parents, G, R, floor, separation, volumes=True):
    """One _lib-level call over all frames of ``prob`` [F, J, N]: a dict of host arrays."""
    F, J, N = prob.shape
    out = outputs(F, J, N, volumes=volumes)
    _lib.skeleton_alternatives(prob.contiguous(), taps, parents, separation, frames=F, voxels=N, grid=G, radius=R, floor=floor, **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def same_values(a, b):
    """The same bits, but for NaN cells, which only have to be NaN on both sides (the payload of a NaN product is not defined)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(np.where(np.isnan(a), 0, a).view(np.int32), np.where(np.isnan(b), 0, b).view(np.int32))


def equals_model(got, want):
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k].astype(np.int32)), (k, got[k].tolist(), want[k].tolist())
    for k in FLOAT_KEYS + (("max_marginals",) if "max_marginals" in got else ()):
        assert want[k].dtype == np.float32 and same_values(got[k], want[k]), k


def check(prob, k, G, R, floor, separation):
    want = skeleton_alternatives_model(prob.cpu().numpy(), k["taps"], k["parents"], G, floor, separation)
    got = launch(prob, k["taps_dev"], k["parents"], G, R, floor, separation)
    equals_model(got, want)
    return got, want


# ------------------------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("frames,tree,G,R,floor", CASES)
def test_against_the_model(frames, tree, G, R, floor):
    k = case(frames, tree, G, R)
    got, want = check(k["prob"], k, G, R, floor, 1)
    print(f"frames {frames} {tree} G {G} R {R} floor {floor}: complete {got['complete'].tolist()}, alternatives "
          f"{int((got['alt_index'] >= 0).sum())} of {got['alt_index'].size}, jumps {int(got['alt_jumped'].sum())}, smallest margin "
          f"{np.nanmin(want['margin']):.4f}, log score spread {np.abs(want['log_mm_best'] - want['log_score'][:, None]).max():.2e}")
    assert want["solved"].all() and want["complete"].all()
    assert np.abs(want["log_mm_best"] - want["log_score"][:, None]).max() < 1e-4          # every joint's best is the pose's score


@pytest.mark.parametrize("separation", [0, 9])
def test_separation_zero_and_a_window_that_leaves_nothing(separation):
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    got, _ = check(k["prob"], k, G, R, 1e-3, separation)
    if separation == G - 1:
        assert (got["alt_index"] == -1).all() and (got["alt_pose"] == -1).all() and (got["alt_value"] == 0).all() and got["complete"].all()
    else:
        assert (got["alt_index"] >= 0).all() and (got["alt_index"] != got["index"]).all()


@pytest.mark.parametrize("floor", [0.5, 1.0])
def test_jumps_on_both_kinds_of_edge(floor):
    """A high floor makes edges jump: on the way up from the anchor (the downward messages) and on the way down (the upward ones)."""
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    got, _ = check(k["prob"], k, G, R, floor, 1)
    up = np.array([[a != j and j in ancestors_and_self(a) for j in range(15)] for a in range(15)])      # edge j lies on the way up from a
    print(f"floor {floor}: {int(got['alt_jumped'].sum())} jumps, {int(got['alt_jumped'][:, up].sum())} of them on the way up")
    assert got["alt_jumped"].any() and got["complete"].all()
    if floor == 1.0:                                                     # keep = 0: every edge of every alternative pose jumps
        assert (got["alt_jumped"][:, :, 1:] == 1).all() and not got["alt_jumped"][:, :, 0].any()
        assert got["alt_jumped"][:, up].any() and got["alt_jumped"][:, ~up].any()


def ancestors_and_self(a):
    out = [a]
    while a > 0:
        a = TREE[a]
        out.append(a)
    return out[:-1]                                                      # the edges are named by their child: the root has none


def test_floor_zero_leaves_anchors_without_an_alternative():
    """floor 0 and compact volumes: outside the reach of the shells every message is zero, so is the max-marginal."""
    G, R = 8, 3
    k = case(1, "chain3", G, R)
    prob = k["prob"].clone()
    box = torch.zeros((G, G, G), device=DEV)
    box[3:5, 3:5, 3:5] = 0.125
    prob[0, 0] = box.reshape(-1)
    got, want = check(prob, k, G, R, 0.0, 2)
    print("alt_index", got["alt_index"].tolist(), "complete", got["complete"].tolist())
    assert want["complete"][0] and got["alt_index"][0, 0] == -1 and (got["alt_pose"][0, 0] == -1).all()       # the root's box lies inside the window
    assert (got["alt_index"][0, 1:] >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ 2. ties, subnormals, NaN
def test_uniform_volumes_resolve_every_tie_to_the_lowest_index():
    G, R = 8, 3
    k = case(1, "star5", G, R)
    prob = torch.full_like(k["prob"], 1.0 / G ** 3)
    got, _ = check(prob, k, G, R, 1e-3, 1)
    assert got["complete"].all() and (got["alt_index"] >= 0).all()


def test_volumes_scaled_into_the_subnormals():
    G, R = 8, 3
    k = case(5, "chain3", G, R)
    prob = k["prob"][:3].clone()
    prob[1] = prob[1] * 1e-38                                            # subnormal inputs
    prob[2, 1] = prob[2, 1] * 1e-30                                      # products that underflow on the way
    got, want = check(prob, k, G, R, 1e-3, 1)
    print("complete", got["complete"].tolist(), "exponents", got["exponent"].tolist(), got["down_exponent"].tolist())
    assert (want["exponent"][1] < -126).any()


def test_a_nan_cell_is_passed_over_and_bad_frames_fall_back():
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    clean = launch(k["prob"], k["taps_dev"], TREE, G, R, 1e-3, 1)
    prob = k["prob"].clone()
    prob[2, 5, int(np.argmin(k["p"][2, 5]))] = float("nan")              # a single NaN cell: frame 2 stays complete
    got, want = check(prob, k, G, R, 1e-3, 1)
    assert want["complete"].all() and np.isnan(got["max_marginals"][2, 5]).sum() == 1
    for key in INT_KEYS + FLOAT_KEYS:
        assert same_values(got[key][:2], clean[key][:2]), key
    prob = k["prob"].clone()
    prob[0] = float("nan")                                               # a NaN frame and an all-zero frame among good ones
    prob[2] = 0.0
    got, want = check(prob, k, G, R, 1e-3, 1)
    assert want["complete"].tolist() == [False, True, False] and got["solved"].tolist() == [0, 1, 0]
    for f in (0, 2):
        assert (got["alt_index"][f] == -1).all() and (got["mm_peak"][f] == -1).all() and (got["alt_pose"][f] == -1).all()
        assert np.isnan(got["alt_value"][f]).all() and np.isnan(got["mm_best"][f]).all() and np.isnan(got["pose_value"][f]).all()
        assert not got["down_exponent"][f].any() and not got["alt_jumped"][f].any()
        assert np.array_equal(got["max_marginals"][f].view(np.int32), prob[f].cpu().numpy().view(np.int32))     # p, bit for bit
    for key in KEYS:
        assert same_values(got[key][1], clean[key][1]), key              # the frame between them is untouched
    # floor 0 and a row of zeros: not solved, so not complete
    prob = k["prob"][:1].clone()
    prob[0, 9] = 0.0
    got, want = check(prob, k, G, R, 0.0, 1)
    assert not want["complete"][0] and not want["solved"][0]


# ------------------------------------------------------------------------------------------------------------------ 3. the pose, batching
@pytest.mark.parametrize("frames,tree,G,R,floor", [CASES[1], CASES[3], CASES[8]])
def test_the_upward_outputs_are_those_of_the_pose(frames, tree, G, R, floor):
    k = case(frames, tree, G, R)
    got = launch(k["prob"], k["taps_dev"], k["parents"], G, R, floor, 1, volumes=False)
    pose = launch_pose(k["prob"], k["taps_dev"], k["parents"], G, R, floor)
    for key, want in zip(("index", "jumped", "exponent", "best_root", "solved"), pose):
        assert same_bits(got[key], want), key


def test_results_do_not_depend_on_how_frames_are_batched():
    G, R = 8, 3
    k = case(5, "chain3", G, R)
    args = (k["taps_dev"], k["parents"], G, R, 1e-3, 1)
    five = launch(k["prob"], *args)
    for cut in (1, 2):
        parts = [launch(k["prob"][:cut], *args), launch(k["prob"][cut:], *args)]
        for key in KEYS:
            assert same_bits(np.concatenate([p[key] for p in parts]), five[key]), (cut, key)
    assert five["complete"].all()


# ------------------------------------------------------------------------------------------------------------------ 4. production shape
def test_production_shape_against_the_float64_score_of_every_alternative_pose():
    """64^3, R = 18, 15 joints, one frame: too slow for the full numpy model, so the outputs are held to what they mean.

    BOUND.  The float32 value behind a pose (alt_value, mm_best or best_root with their exponents) is a product of 3J - 2 factors: J
    values p_j(x_j), J - 1 taps w_j and J - 1 weights (keep, or uniform for a jump).  The taps and the p are exact inputs; keep =
    1 - floor and uniform = floor / N carry one rounding each (J - 1 in all); the 3J - 3 multiplications that join the factors carry one
    each, whatever order the passes take them in; the rescalings by powers of two are exact as long as nothing underflows (asserted: the
    scaled values are > 2^-60 and every other scaled factor is < 2, so no partial product drops below 2^-60-J).  That is fewer than 4J
    roundings of relative size u = 2^-24, so | ln float32 - ln exact | <= 4 J u / (1 - 4 J u) = 3.6e-6 for every pose.  The float64
    evaluation (pose_log_score) adds less than 1e-12.  Two float32 maxima of the same exact maximum (ln mm_best of two joints, or of a
    joint and the pose's log score) each lie within the bound of it: they differ by at most twice the bound."""
    G, R, tau, J, floor = 64, 18, 0.03, 15, 1e-3
    N, h = G ** 3, SIDE / G
    lengths = np.concatenate([[0.0], BONES])
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    prob = softmax_on_device(make_logits(1, TREE, lengths, G, 6418)[0], coord)
    taps = shell_taps(lengths, tau, h, R)
    taps_dev = torch.from_numpy(taps).to(DEV)
    got = launch(prob, taps_dev, TREE, G, R, floor, 2, volumes=False)
    for key, want in zip(("index", "jumped", "exponent", "best_root", "solved"), launch_pose(prob, taps_dev, TREE, G, R, floor)):
        assert same_bits(got[key], want), key
    assert got["solved"].all() and got["complete"].all() and (got["alt_index"] >= 0).all()
    assert (got["alt_value"] > 2.0 ** -60).all() and (got["mm_best"] > 2.0 ** -60).all()
    d = derive(got, TREE)
    p = prob[0].cpu().numpy()
    u = 2.0 ** -24
    bound = 4 * J * u / (1 - 4 * J * u)
    spread = np.abs(d["log_mm_best"][0] - d["log_score"][0]).max()
    errs = [abs(pose_log_score(p, taps, TREE, G, floor, [int(v) for v in got["alt_pose"][0, a]]) - d["alt_log_score"][0, a]) for a in range(J)]
    own = abs(pose_log_score(p, taps, TREE, G, floor, [int(v) for v in got["index"][0]]) - d["log_score"][0])
    print(f"64^3: log score {d['log_score'][0]:.6f}, |ln mm_best - log score| max {spread:.3e} (bound {2 * bound:.3e}), alternative poses "
          f"max {max(errs):.3e}, the pose {own:.3e} (bound {bound:.3e}); margins {d['margin'][0].round(3).tolist()}")
    assert spread <= 2 * bound and max(errs) <= bound and own <= bound
    far = np.abs(np.stack(np.unravel_index(got["alt_index"][0], (G, G, G))) - np.stack(np.unravel_index(got["index"][0], (G, G, G)))).max(axis=0)
    assert (far > 2).all() and (got["alt_pose"][0][np.arange(J), np.arange(J)] == got["alt_index"][0]).all()
    assert (d["margin"][0] >= -2 * bound).all()


# ------------------------------------------------------------------------------------------------------------------ 5. bad arguments
def test_bad_arguments_raise_and_do_not_launch():
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    N, J = G ** 3, 15
    prob = k["prob"][:2].contiguous()
    outs = outputs(2, J, N)

    def call(**kw):
        a = {"prob": prob, "taps": k["taps_dev"], "parents": TREE, "separation": 1, **outs, "frames": 2, "voxels": N, "grid": G, "radius": R,
             "floor": 1e-3}
        a.update(kw)
        return _lib.skeleton_alternatives(**a)

    bad_tree = list(TREE)
    bad_tree[5] = 5
    for kw in ({"separation": -1}, {"separation": 1.5}, {"separation": True}, {"separation": None}, {"radius": 25}, {"radius": G},
               {"floor": -0.1}, {"floor": float("nan")}, {"frames": 0}, {"frames": 3}, {"grid": G + 1}, {"voxels": N + 1},
               {"parents": bad_tree}, {"parents": None}, {"prob": prob.cpu()}, {"prob": prob.double()}, {"taps": k["taps_dev"][:-1]},
               {"index": outs["index"].float()}, {"alt_pose": outs["alt_pose"][:, :, :-1]}, {"alt_jumped": outs["alt_index"]},
               {"mm_best": outs["mm_peak"]}, {"complete": None}, {"down_exponent": outs["down_exponent"][:1]}, {"max_marginals": prob},
               {"max_marginals": outs["max_marginals"][:1]}, {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    # the C entry point refuses on its own what the wrapper checks first
    import ctypes
    lib = _lib.load()
    ws = torch.empty(_lib.skeleton_alternatives_scratch_bytes(2, J, G, R), device=DEV, dtype=torch.uint8)
    assert ws.numel() > _lib.skeleton_pose_scratch_bytes(2, J, G, R)
    P = _lib._ptr
    order = ("index", "jumped", "exponent", "best_root", "solved", "down_exponent", "mm_best", "pose_value", "alt_value", "mm_peak",
             "alt_index", "alt_pose", "alt_jumped", "complete", "max_marginals")

    def raw(separation=1, radius=R, floor=1e-3, frames=2, grid=G, voxels=N, scratch_bytes=ws.numel(), parents=TREE, scratch=ws, n=J, **kw):
        par = (ctypes.c_int * len(parents))(*parents)
        o = {**outs, **kw}
        return lib.se_skeleton_alternatives_f32(P(prob), P(k["taps_dev"]), ctypes.cast(par, ctypes.c_void_p), separation,
                                                *[P(o[key]) for key in order], P(scratch), scratch_bytes, frames, n, voxels, grid, radius,
                                                floor, _lib._stream())
    assert raw(separation=-1) == raw(radius=25) == raw(radius=G) == raw(floor=2.0) == raw(floor=float("nan")) == raw(frames=0) == -1
    assert raw(voxels=N + 4) == raw(grid=129) == raw(scratch_bytes=ws.numel() - 1) == raw(index=None) == raw(complete=None) == -1
    assert raw(parents=bad_tree) == raw(n=0) == raw(n=33) == raw(max_marginals=prob) == -1
    assert raw(scratch=ws[1:], scratch_bytes=ws.numel() - 1) == -1       # misaligned
    assert lib.se_skeleton_alternatives_scratch_bytes(2, 33, G, R) == 0 and lib.se_skeleton_alternatives_scratch_bytes(2, J, G, G) == 0
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in outs.values())                   # nothing was launched
    call()
    assert raw(max_marginals=None) == 0
    torch.cuda.synchronize()
    assert (outs["complete"] == 1).all() and (outs["max_marginals"] != -7).all() and (outs["alt_pose"] != -7).all()
    # the module checks its own arguments before anything touches the device
    sp = SkeletonPose(np.zeros((G, G, G, 3), dtype=np.float32), G, SIDE, [0.3] * 14)
    vols = torch.zeros((1, J, G, G, G), device=DEV)
    for kw in ({"separation": -1}, {"separation": 1.0}, {"separation": False}, {"joints": torch.zeros((2, J, 3))}):
        with pytest.raises(ValueError):
            sp.alternatives(vols, **kw)
    with pytest.raises(ValueError):
        sp.alternatives(vols[:, :14])
    with pytest.raises(_lib.HipExtensionError):
        sp.alternatives(vols.cpu())


# ------------------------------------------------------------------------------------------------------------------ 6. public surface
def test_module_alternatives_equal_the_library_call(net64, two_forwards):
    G, J = net64.volume_size, 15
    N = G ** 3
    sp = net64.skeleton_pose(BONES)
    kp, vols = two_forwards[0]
    res = sp.alternatives(vols, separation=2, joints=kp, return_max_marginals=True)
    solved = sp.solve(vols, joints=kp)
    torch.cuda.synchronize()
    assert tuple(res)[:len(solved)] == tuple(solved) and tuple(res)[len(solved):] == op.ALTERNATIVES_KEYS + ("max_marginals",)
    for key, v in solved.items():
        assert res[key].dtype == v.dtype and np.array_equal(res[key].cpu().numpy(), v.cpu().numpy(), equal_nan=v.is_floating_point()), key
    taps = shell_taps(np.concatenate([[0.0], BONES]), 0.03, net64.cuboid_side / G, sp.radius)
    raw = launch(vols.reshape(2, J, N), torch.from_numpy(taps).to(DEV), TREE, G, sp.radius, 1e-3, 2)
    d = derive(raw, TREE)
    host = {key: v.cpu().numpy() for key, v in res.items()}
    assert np.array_equal(host["complete"], raw["complete"] != 0) and raw["complete"].all()
    assert np.array_equal(host["alt_index"], raw["alt_index"]) and np.array_equal(host["alt_pose_index"], raw["alt_pose"])
    assert np.array_equal(host["alt_pose_jumped"], raw["alt_jumped"] != 0) and np.array_equal(host["max_marginal_peak_index"], raw["mm_peak"])
    assert np.array_equal(host["pose_is_peak"], raw["mm_peak"] == raw["index"])
    assert host["margin"].dtype == np.float64 and np.allclose(host["margin"], d["margin"], rtol=1e-12, atol=1e-12)
    assert np.allclose(host["alt_log_score"], d["alt_log_score"], rtol=1e-13, atol=0)
    c = net64.coord_volumes[0].reshape(N, 3).float().cpu().numpy()
    assert same_bits(host["alt_coord"], c[raw["alt_index"]])
    p = vols.reshape(2, J, N).cpu().numpy()
    for a in range(J):
        assert same_bits(host["alt_pose_joints"][:, a], refine_model(p, c, raw["alt_pose"][:, a], G, 1)), a
    runner = np.argmax(d["alt_log_score"], axis=1)                       # the first of equal maxima
    assert np.array_equal(host["runner_up"], runner) and host["runner_up"].shape == (2,)
    rows = np.arange(2)
    assert same_bits(host["runner_up_joints"], host["alt_pose_joints"][rows, runner])
    assert np.allclose(host["runner_up_margin"], d["margin"][rows, runner], rtol=1e-12, atol=1e-12) and (host["runner_up_margin"] >= -1e-5).all()
    rj = torch.from_numpy(host["runner_up_joints"])
    want_err = ((rj[:, 1:] - rj[:, list(TREE[1:])]).norm(dim=-1) - torch.from_numpy(BONES.astype(np.float32))).abs().numpy()
    assert np.allclose(host["runner_up_bone_error"], want_err, rtol=1e-5, atol=1e-6)
    mm = host["max_marginals"].reshape(2, J, N)
    assert mm.shape == (2, J, N) and (mm >= 0).all() and np.allclose(mm.max(axis=2), 1.0, rtol=1e-6)
    assert np.allclose(mm, raw["max_marginals"] / raw["mm_best"][..., None], rtol=1e-6, atol=0)
    print(f"synthetic weights: runner-up anchors {host['runner_up'].tolist()}, margins {host['runner_up_margin'].round(4).tolist()}, "
          f"pose_is_peak {host['pose_is_peak'].all(axis=1).tolist()}")
    frames = op.skeleton_alternatives_to_numpy(res)
    assert len(frames) == 2 and tuple(frames[0]) == tuple(res) and frames[1]["alt_pose_joints"].shape == (J, J, 3)
    assert frames[1]["runner_up"] == runner[1] and frames[0]["max_marginals"].shape == (J, G, G, G)


# ------------------------------------------------------------------------------------------------------------------ 7. command line
def test_run_sequence_map_alternatives_output(tmp_path, capsys):
    import evaluate
    import run_sequence
    from sceneego_amd import synth
    demo_exr = os.path.join(GOLD, "demo", "img_001000.jpg.exr")
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 5, [demo_exr], estimated_depth_name="est_depth", seed=5)
    cfg_path = tmp_path / "batch2.yaml"
    with open(os.path.join(os.path.dirname(GOLD), "..", "experiments", "sceneego", "test", "sceneego.yaml")) as f:
        text = f.read()
    assert text.count("  batch_size: 8\n") == 1
    cfg_path.write_text(text.replace("  batch_size: 8\n", "  batch_size: 2\n"))
    np.save(tmp_path / "bones.npy", BONES)
    res = run_sequence.main(["--config", str(cfg_path), "--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name",
                             "est_depth", "--weights", "synthetic", "--output", str(tmp_path / "plain.pkl"), "--map_output",
                             str(tmp_path / "map.pkl"), "--map_alternatives_output", str(tmp_path / "alt.pkl"), "--map_separation", "3",
                             "--bone_lengths", str(tmp_path / "bones.npy")])
    last = capsys.readouterr().out.splitlines()[-1]
    assert "runner-up margin" in last and "below ln 2" in last
    with open(tmp_path / "alt.pkl", "rb") as f:
        alts = pickle.load(f)
    with open(tmp_path / "map.pkl", "rb") as f:
        posed = pickle.load(f)
    assert len(alts) == len(posed) == 5 and len(res["map_alternatives"]) == 5
    for fr, pose in zip(alts, posed):
        assert tuple(fr)[:7] == op.POSE_KEYS and "max_marginals" not in fr and np.array_equal(fr["joints"], pose)
        assert fr["complete"] and fr["runner_up"] >= 0 and fr["runner_up_joints"].shape == (15, 3) and np.isfinite(fr["runner_up_margin"])
        far = np.abs(np.stack(np.unravel_index(fr["alt_index"], (64, 64, 64))) - np.stack(np.unravel_index(fr["index"], (64, 64, 64))))
        assert (far.max(axis=0) > 3).all()
    assert np.isclose(res["map_runner_up_margin"], np.mean([fr["runner_up_margin"] for fr in alts]))
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((5, 15, 3)), f)
    ev = evaluate.main(["--pred_dir", str(tmp_path / "map.pkl"), "--alternatives", str(tmp_path / "alt.pkl"), "--gt", str(tmp_path / "gt.pkl")])
    capsys.readouterr()
    assert ev["alternatives"]["best_of_two_mpjpe"] <= ev["mpjpe"] + 1e-9 and -1.0 <= ev["alternatives"]["spearman_error_margin"] <= 1.0
