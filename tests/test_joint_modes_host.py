"""CPU: the joint-modes feature without a GPU: the C ABI declarations, the wrappers' refusal of CPU tensors, the exact model of
tests/joint_modes_model.py at volumes small enough to write the answers out by hand, sceneego_amd.track.select_modes against the
enumeration of every path, and evaluate.py --modes on hand-made pickles."""
import itertools
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from joint_modes_model import QNAN_BITS, joint_modes_model, mode_mask
from sceneego_amd import _lib, load_config, op, track


# ------------------------------------------------------------------------------------------------------------------ C ABI, wrappers
def test_abi_declarations():
    text = open(os.path.join(ROOT, "include", "sceneego_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("se_joint_modes_f32", "se_joint_modes_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["se_joint_modes_f32"][1]) == 15 and len(_lib.SIGNATURES["se_joint_modes_scratch_bytes"][1]) == 3
    assert _lib.ABI_VERSION >= 32
    assert _lib.MODES_SLOTS == 8 and _lib.MODES_MAX_K == 16 and _lib.MODES_MAX_RADIUS == 3
    assert op.MODES_KEYS == ("coord", "peak_coord", "peak_prob", "mass", "index", "count", "total", "valid")


def test_scratch_query_is_a_host_function_of_the_shape():
    lib = _lib.load()
    assert lib.se_joint_modes_scratch_bytes(0, 64, 4) == 0 and lib.se_joint_modes_scratch_bytes(-1, 64, 4) == 0
    assert lib.se_joint_modes_scratch_bytes(15, 1, 4) == 0 and lib.se_joint_modes_scratch_bytes(15, 64, 0) == 0
    assert lib.se_joint_modes_scratch_bytes(15, 64, 17) == 0
    # tiles of 4 i-planes x 256 / ceil(G / 4) j-rows; 2 + 2K words per (row, tile)
    assert lib.se_joint_modes_scratch_bytes(15, 64, 4) == 15 * (16 * 4) * 10 * 4
    assert lib.se_joint_modes_scratch_bytes(120, 16, 16) == 120 * (4 * 1) * 34 * 4
    assert lib.se_joint_modes_scratch_bytes(1, 24, 1) == 1 * (6 * 1) * 4 * 4
    assert lib.se_joint_modes_scratch_bytes(2, 128, 4) == 2 * (32 * 16) * 10 * 4


def test_wrappers_refuse_cpu_tensors():
    G, B, J, K = 4, 1, 2, 4
    N = G ** 3
    vol = torch.full((B, J, G, G, G), 1.0 / N)
    coord = torch.zeros((1, G, G, G, 3))
    with pytest.raises(_lib.HipExtensionError):
        _lib.joint_modes(vol.view(B * J, N), coord.view(N, 3), torch.zeros((B * J, K, 8)), torch.zeros((B * J, K), dtype=torch.int32),
                         torch.zeros(B * J, dtype=torch.int32), torch.zeros(B * J, dtype=torch.int32), B * J, N, G, K, 2, 0.0)
    with pytest.raises(_lib.HipExtensionError):
        op.joint_modes(vol, coord)
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    cfg = load_config()
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    Gn = net.volume_size
    with pytest.raises(_lib.HipExtensionError):
        net.joint_modes(torch.zeros((1, 15, Gn, Gn, Gn)))
    cfg.model.volume_softmax = False
    with pytest.raises(ValueError):
        VoxelNetwork_depth(cfg, device="cpu", verbose=False).joint_modes(torch.zeros((1, 15, Gn, Gn, Gn)))


# ------------------------------------------------------------------------------------------------------------------ the model by hand
def flat(G, i, j, k):
    return (i * G + j) * G + k


def grid_coord(G):
    """coord[n] = (i, j, k) as float32: window moments are then sums of small integers times p."""
    return np.stack(np.meshgrid(*(np.arange(G, dtype=np.float32),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)


def volume(G, values):
    p = np.zeros(G ** 3, dtype=np.float32)
    for at, v in values.items():
        p[flat(G, *at)] = v
    return p


def test_model_adjacent_tie_takes_the_lower_index():
    G = 4
    p = volume(G, {(1, 1, 1): 0.25, (1, 1, 2): 0.25})
    assert np.flatnonzero(mode_mask(p, G)).tolist() == [flat(G, 1, 1, 1)]
    # adjacent along a diagonal whose higher index has the lower j and k
    p = volume(G, {(1, 2, 2): 0.25, (2, 1, 1): 0.25})
    assert np.flatnonzero(mode_mask(p, G)).tolist() == [flat(G, 1, 2, 2)]


def test_model_non_adjacent_tie_gives_both_in_index_order():
    G = 5
    p = volume(G, {(1, 1, 1): 0.25, (1, 1, 3): 0.25, (4, 4, 4): 0.125})
    modes, index, count, total = joint_modes_model(p[None], grid_coord(G), G, 4, 0)
    assert total.tolist() == [3] and count.tolist() == [3]
    assert index[0].tolist() == [flat(G, 1, 1, 1), flat(G, 1, 1, 3), flat(G, 4, 4, 4), -1]
    assert modes[0, :3, 0].tolist() == [0.25, 0.25, 0.125]
    # radius 0: mass = p, mom = p * (i, j, k)
    assert modes[0, :3, 1].tolist() == [0.25, 0.25, 0.125]
    assert modes[0, :3, 2:5].tolist() == [[0.25, 0.25, 0.25], [0.25, 0.25, 0.75], [0.5, 0.5, 0.5]]
    assert modes[0, :3, 5:].tolist() == [[1, 1, 1], [1, 1, 3], [4, 4, 4]]
    # the unfilled record: +0 in slots 0..4, NaN in 5..7
    assert (modes[0, 3, :5].view(np.uint32) == 0).all() and (modes[0, 3, 5:].view(np.uint32) == QNAN_BITS).all()
    # K = 2 keeps the first two and still counts three
    _, index, count, total = joint_modes_model(p[None], grid_coord(G), G, 2, 0)
    assert index[0].tolist() == [flat(G, 1, 1, 1), flat(G, 1, 1, 3)] and count.tolist() == [2] and total.tolist() == [3]


def test_model_plateau_gives_one_mode():
    G = 4
    cube = {(1 + a, 1 + b, 1 + c): 0.0625 for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert np.flatnonzero(mode_mask(volume(G, cube), G)).tolist() == [flat(G, 1, 1, 1)]
    # a uniform volume: every voxel but n = 0 has an equal neighbour of lower index
    assert np.flatnonzero(mode_mask(np.full(G ** 3, 1.0 / G ** 3, dtype=np.float32), G)).tolist() == [0]
    # nothing wraps: (0, 0, 3) and (0, 1, 0) are flat indices 3 and 4, but |dk| = 3: not neighbours, two modes
    p = volume(G, {(0, 0, 3): 0.5, (0, 1, 0): 0.5})
    assert np.flatnonzero(mode_mask(p, G)).tolist() == [3, 4]
    p = volume(G, {(0, 3, 3): 0.5, (1, 0, 0): 0.5})          # likewise from one plane into the next: 15 and 16
    assert np.flatnonzero(mode_mask(p, G)).tolist() == [15, 16]


def test_model_corner_mode_with_a_clipped_window():
    G = 4
    p = volume(G, {(0, 0, 0): 0.5, (0, 0, 1): 0.25, (1, 1, 1): 0.125, (2, 2, 2): 0.0625, (3, 3, 3): 0.03125})
    modes, index, count, total = joint_modes_model(p[None], grid_coord(G), G, 4, 1)
    # (0,0,1) and (1,1,1) are neighbours of (0,0,0); (2,2,2) is a neighbour of (1,1,1); (3,3,3) of (2,2,2): one mode
    assert total.tolist() == [1] and index[0].tolist() == [0, -1, -1, -1]
    # window of radius 1 at the corner: i, j, k in 0..1, 8 voxels
    assert modes[0, 0, :5].tolist() == [0.5, 0.875, 0.125, 0.125, 0.25 + 0.125]
    # radius 3 reaches the whole grid from the corner
    modes, _, _, _ = joint_modes_model(p[None], grid_coord(G), G, 1, 3)
    assert modes[0, 0, 1] == 0.96875
    assert modes[0, 0, 2:5].tolist() == [0.125 + 0.125 + 0.09375, 0.125 + 0.125 + 0.09375, 0.25 + 0.125 + 0.125 + 0.09375]
    # the far corner, n = voxels - 1
    p = volume(G, {(3, 3, 3): 0.5, (3, 3, 2): 0.25})
    modes, index, _, _ = joint_modes_model(p[None], grid_coord(G), G, 1, 2)
    assert index[0].tolist() == [G ** 3 - 1] and modes[0, 0, :5].tolist() == [0.5, 0.75, 2.25, 2.25, 2.0]


def test_model_min_prob_is_inclusive():
    G = 4
    p = volume(G, {(0, 0, 0): 0.5, (3, 3, 3): 0.125})
    assert joint_modes_model(p[None], grid_coord(G), G, 4, 0, min_prob=0.125)[3].tolist() == [2]
    above = np.nextafter(np.float32(0.125), np.float32(1))
    _, index, count, total = joint_modes_model(p[None], grid_coord(G), G, 4, 0, min_prob=above)
    assert total.tolist() == [1] and count.tolist() == [1] and index[0].tolist() == [0, -1, -1, -1]
    assert joint_modes_model(p[None], grid_coord(G), G, 4, 0, min_prob=0.75)[3].tolist() == [0]


def test_model_all_zero_and_nan_rows():
    G = 4
    p = np.stack([np.zeros(G ** 3, dtype=np.float32), volume(G, {(1, 2, 3): 1.0}), volume(G, {(1, 2, 3): 1.0})])
    p[2, 5] = np.nan
    modes, index, count, total = joint_modes_model(p, grid_coord(G), G, 2, 1)
    assert count.tolist() == [0, 1, -1] and total.tolist() == [0, 1, -1]
    assert index.tolist() == [[-1, -1], [flat(G, 1, 2, 3), -1], [-1, -1]]
    assert (modes[0, :, :5].view(np.uint32) == 0).all() and (modes[0, :, 5:].view(np.uint32) == QNAN_BITS).all()
    assert modes[1, 0].tolist() == [1.0, 1.0, 1.0, 2.0, 3.0, 1.0, 2.0, 3.0]
    assert (modes[2].view(np.uint32) == QNAN_BITS).all()


# ------------------------------------------------------------------------------------------------------------------ select_modes
def random_frames(T, J, K, seed, valid_share=0.8):
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(T):
        valid = rng.random((J, K)) < valid_share
        valid[:, 0] = True
        frames.append({"coord": rng.uniform(-0.5, 0.5, size=(J, K, 3)).astype(np.float32),
                       "mass": rng.uniform(0.01, 0.9, size=(J, K)).astype(np.float32), "valid": valid})
    return frames


def enumerate_paths(frames, sigma, fallback=None):
    """Every path of every joint, costed in frame order as select_modes states it, ((c + step) + node); of the minimal ones the
    lowest slot in the last frame, then in the frame before, ..."""
    T, J = len(frames), frames[0]["mass"].shape[0]
    joints = np.empty((T, J, 3), dtype=np.float32)
    choice = np.empty((T, J), dtype=np.int64)
    inv = 1.0 / (2.0 * sigma * sigma)
    for j in range(J):
        cands = []
        for t, f in enumerate(frames):
            k = np.flatnonzero(f["valid"][j])
            if k.size:
                node = -np.log(np.asarray(f["mass"], dtype=np.float64)[j, k])
                cands.append([(int(s), f["coord"][j, s].astype(np.float64), node[n]) for n, s in enumerate(k)])
            else:
                cands.append([(-1, np.asarray(fallback[t, j], dtype=np.float64), 0.0)])
        best = None
        for path in itertools.product(*cands):
            c = path[0][2]
            for a, b in zip(path[:-1], path[1:]):
                d = b[1] - a[1]
                c = (c + ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * inv) + b[2]
            key = (c, tuple(s for s, _, _ in reversed(path)))
            if best is None or key < best[0]:
                best = (key, path)
        for t, (s, pos, _) in enumerate(best[1]):
            choice[t, j] = s
            joints[t, j] = pos
    return joints, choice


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_select_modes_equals_exhaustive_enumeration(seed):
    T, J, K = 5, 15, 3
    frames = random_frames(T, J, K, seed)
    # a planted cost tie: in frame 2 the only valid modes of joint 4 are slots 1 and 2, the same mode twice
    frames[2]["valid"][4] = [False, True, True]
    frames[2]["coord"][4, 2] = frames[2]["coord"][4, 1]
    frames[2]["mass"][4, 2] = frames[2]["mass"][4, 1]
    # and in the last frame of joint 7 slots 0 and 1
    frames[4]["valid"][7] = [True, True, False]
    frames[4]["coord"][7, 1] = frames[4]["coord"][7, 0]
    frames[4]["mass"][7, 1] = frames[4]["mass"][7, 0]
    joints, choice = track.select_modes(frames, sigma=0.1)
    want_joints, want_choice = enumerate_paths(frames, 0.1)
    assert joints.dtype == np.float32 and joints.shape == (T, J, 3) and choice.shape == (T, J)
    assert np.issubdtype(choice.dtype, np.integer)
    assert np.array_equal(choice, want_choice)
    assert np.array_equal(joints, want_joints)
    assert choice[2, 4] == 1 and choice[4, 7] == 0, "the planted ties were not broken by the lowest slot"


def test_select_modes_fallback():
    T, J, K = 5, 15, 3
    frames = random_frames(T, J, K, seed=11)
    frames[2]["valid"][3, :] = False
    frames[0]["valid"][9, :] = False
    frames[4]["valid"][9, :] = False
    fallback = np.random.default_rng(5).uniform(-0.5, 0.5, size=(T, J, 3)).astype(np.float32)
    with pytest.raises(ValueError):
        track.select_modes(frames, sigma=0.1, fallback=None)
    joints, choice = track.select_modes(frames, sigma=0.1, fallback=fallback)
    want_joints, want_choice = enumerate_paths(frames, 0.1, fallback)
    assert np.array_equal(choice, want_choice) and np.array_equal(joints, want_joints)
    assert choice[2, 3] == -1 and choice[0, 9] == -1 and choice[4, 9] == -1 and (choice >= 0).sum() == T * J - 3
    assert np.array_equal(joints[2, 3], fallback[2, 3]) and np.array_equal(joints[0, 9], fallback[0, 9])
    with pytest.raises(ValueError):
        track.select_modes(frames, sigma=0.1, fallback=fallback[:-1])
    with pytest.raises(ValueError):
        track.select_modes(frames, sigma=0.0, fallback=fallback)
    with pytest.raises(ValueError):
        track.select_modes([], sigma=0.1)


def test_select_modes_stays_on_one_lobe_where_the_per_frame_argmax_jumps():
    T, J, K = 7, 15, 2
    a, b = np.array([0.3, 0.0, 0.2], dtype=np.float32), np.array([-0.3, 0.1, 0.2], dtype=np.float32)      # 0.61 m apart
    frames = []
    for t in range(T):
        # the kernel lists the heavier lobe first: the lobes swap slots from frame to frame
        first, second = (a, b) if t % 2 == 0 else (b, a)
        frames.append({"coord": np.tile(np.stack([first, second])[None], (J, 1, 1)),
                       "mass": np.tile(np.array([[0.45, 0.40]], dtype=np.float32), (J, 1)), "valid": np.ones((J, K), dtype=bool)})
    joints, choice = track.select_modes(frames, sigma=0.1)
    per_frame = np.stack([f["coord"][:, 0] for f in frames])                       # the heaviest mode of every frame
    jump = np.linalg.norm(per_frame[1:] - per_frame[:-1], axis=-1)
    assert (jump > 0.6).all(), "the per-frame choice was meant to jump between the lobes"
    assert (np.linalg.norm(joints[1:] - joints[:-1], axis=-1) == 0).all(), "the selected path left its lobe"
    # -ln(0.40) - -ln(0.45) = 0.118 per frame is cheaper than one jump of 0.61^2 / 0.02 = 18.6: the path stays on one lobe, the one
    # that is the heavier in 4 of the 7 frames
    assert np.array_equal(choice[:, 0], np.array([0, 1, 0, 1, 0, 1, 0])) and (choice == choice[:, :1]).all()
    assert np.array_equal(joints[0, 0], a)


# ------------------------------------------------------------------------------------------------------------------ evaluate.py --modes
def test_evaluate_modes_on_hand_made_pickles(tmp_path, capsys):
    import evaluate
    T, J, K = 2, 15, 3
    gt = np.zeros((T, J, 3))
    gt[1, :, 0] = 1.0
    pred = gt.copy()
    pred[:, :, 2] += 0.5                                   # every prediction 0.5 off
    frames = []
    for t in range(T):
        coord = np.full((J, K, 3), np.nan, dtype=np.float32)
        valid = np.zeros((J, K), dtype=bool)
        coord[:, 0] = pred[t]                              # mode 0: the prediction, 0.5 off
        valid[:, 0] = True
        coord[:5, 1] = gt[t, :5] + np.array([0.0, 0.25, 0.0])      # joints 0..4: mode 1 is 0.25 off
        valid[:5, 1] = True
        coord[5:8, 2] = gt[t, 5:8]                         # joints 5..7: an exact mode that is NOT valid
        frames.append({"coord": coord, "valid": valid, "mass": np.ones((J, K), dtype=np.float32)})
    frames[1]["valid"][14, :] = False                      # one joint without a valid mode: its prediction counts
    pred_dir = tmp_path / "pred"
    pred_dir.mkdir()
    for t in range(T):
        with open(pred_dir / ("img_%06d.jpg.pkl" % t), "wb") as f:
            pickle.dump(pred[t].astype(np.float32), f)
        with open(pred_dir / ("img_%06d.jpg.modes.pkl" % t), "wb") as f:
            pickle.dump(frames[t], f)
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(gt, f)
    with open(tmp_path / "modes.pkl", "wb") as f:
        pickle.dump(frames, f)
    with open(tmp_path / "preds.pkl", "wb") as f:
        pickle.dump([p.astype(np.float32) for p in pred], f)
    want = (10 * 0.25 + 20 * 0.5) / 30
    for pred_arg, modes_arg in ((str(pred_dir), str(pred_dir)), (str(pred_dir), str(tmp_path / "modes.pkl")),
                                (str(tmp_path / "preds.pkl"), str(tmp_path / "modes.pkl"))):
        r = evaluate.main(["--pred_dir", pred_arg, "--gt", str(tmp_path / "gt.pkl"), "--modes", modes_arg])
        out = capsys.readouterr().out
        assert r["frames"] == T and abs(r["mpjpe"] - 0.5) < 1e-12
        assert abs(r["best_of_k_mpjpe"] - want) < 1e-9
        assert r["joints_with_modes"] == 29 and abs(r["best_not_first_share"] - 10 / 29) < 1e-12
        assert "best-of-K MPJPE" in out
    r = evaluate.main(["--pred_dir", str(pred_dir), "--gt", str(tmp_path / "gt.pkl")])
    capsys.readouterr()
    assert "best_of_k_mpjpe" not in r and r["frames"] == T
    with open(tmp_path / "short.pkl", "wb") as f:
        pickle.dump(frames[:1], f)
    with pytest.raises(SystemExit):
        evaluate.main(["--pred_dir", str(pred_dir), "--gt", str(tmp_path / "gt.pkl"), "--modes", str(tmp_path / "short.pkl")])
