"""Host side of the scene-constrained joints: op.build_sight_table against the float64 model of tests/scene_constraint_model.py, the
C ABI declarations (header, _lib.SIGNATURES, ABI version), the wrappers' refusal of CPU tensors, the demo.py / run_sequence.py flags
and evaluate.py's skip list.  No GPU."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import scene_constraint_model as M
from conftest import ROOT
from sceneego_amd import _lib, load_config, op
from sceneego_amd.config import resolve_calibration_path
from sceneego_amd.fisheye import FishEyeCameraCalibrated

H, W = 1024, 1280


def _shipped(G):
    cfg = load_config()
    cam = FishEyeCameraCalibrated(calibration_file_path=resolve_calibration_path(cfg.dataset.camera_calibration_path))
    coord = op.build_coord_volume(G, float(cfg.model.cuboid_side))
    proj = op.get_projected_2d_points_with_coord_volumes(fisheye_model=cam, coord_volume=coord)
    return proj, coord


# ------------------------------------------------------------------------------------------------------------------ sight table
@pytest.mark.parametrize("G", [8, 64])
def test_sight_table_matches_the_model_on_the_shipped_calibration(G):
    proj, coord = _shipped(G)
    pix, rng = op.build_sight_table(proj, coord, H, W)
    assert pix.dtype == torch.int32 and rng.dtype == torch.float32 and tuple(pix.shape) == (G ** 3,) == tuple(rng.shape)
    pix, rng = pix.numpy(), rng.numpy()
    assert ((pix == -1) | ((pix >= 0) & (pix < H * W))).all()
    assert (pix >= 0).any(), "no voxel of the shipped grid projects into the frame"
    want_pix, want_rng = M.sight_table(proj.float().numpy().reshape(-1, 2), coord.numpy().reshape(-1, 3), H, W)
    assert np.array_equal(pix, want_pix)
    assert np.array_equal(rng.view(np.int32), want_rng.view(np.int32))


def test_sight_table_hand_made_projection():
    h, w = 6, 10
    uv = torch.tensor([[2.5, 3.5],                      # u = x - 0.5 exactly: floor(2.5 + 0.5) = 3, floor(3.5 + 0.5) = 4
                       [0.0, 0.0], [9.49, 5.49],        # the corners
                       [-0.5, 0.0],                     # floor(0.0) = 0: still inside
                       [-0.51, 0.0], [0.0, -0.75],      # negative -> x = -1 / y = -1
                       [9.5, 0.0], [0.0, 5.5],          # >= W, >= H
                       [float("nan"), 1.0], [1.0, float("nan")], [float("inf"), 1.0], [1.0, float("-inf")],
                       [1e30, 1.0]], dtype=torch.float32)
    coord = torch.arange(uv.shape[0] * 3, dtype=torch.float32).reshape(-1, 3) * 0.1
    pix, rng = op.build_sight_table(uv, coord, h, w)
    assert pix.tolist() == [4 * w + 3, 0, 5 * w + 9, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1]
    want_pix, want_rng = M.sight_table(uv.numpy(), coord.numpy(), h, w)
    assert np.array_equal(pix.numpy(), want_pix) and np.array_equal(rng.numpy().view(np.int32), want_rng.view(np.int32))
    with pytest.raises(ValueError):
        op.build_sight_table(uv, coord[:-1], h, w)
    with pytest.raises(ValueError):
        op.build_sight_table(uv, coord, 0, w)


def test_model_free_mask_rule_by_hand():
    # frame 2 x 2 on a 1 x 2 depth map: pixel (x, y) reads depth[0][(x * 2) // 2]
    depth = np.array([[[1.0, 0.0]]], dtype=np.float32)
    pix = np.array([0, 0, 0, 1, -1, 3, 99], dtype=np.int32)
    rng = np.array([1.5, 1.25, 1.2, 9.0, 9.0, 9.0, 9.0], dtype=np.float32)
    free = M.free_mask(depth, pix, rng, 2, 2, 0.25, 100.0)
    #                          behind  equal  front  no surface  no pixel  no surface  out of frame
    assert free.tolist() == [[0, 1, 1, 1, 1, 1, 1]]


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_abi_declarations():
    text = open(os.path.join(ROOT, "include", "sceneego_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("se_scene_free_mask_u8", "se_softargmax3d_masked_f32", "se_softargmax3d_masked_scratch_elems"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["se_scene_free_mask_u8"][1]) == 13
    assert len(_lib.SIGNATURES["se_softargmax3d_masked_f32"][1]) == 10
    assert _lib.ABI_VERSION >= 30
    assert _lib.MASKED_SLOTS == 8


def test_scratch_query_follows_the_soft_argmax_chunk_rule():
    lib = _lib.load()
    assert lib.se_softargmax3d_masked_scratch_elems(0) == 0 and lib.se_softargmax3d_masked_scratch_elems(-3) == 0
    assert lib.se_softargmax3d_masked_scratch_elems(15) == 15 * 256 * 8 and lib.se_softargmax3d_masked_scratch_elems(30) == 30 * 128 * 8
    assert lib.se_softargmax3d_masked_scratch_elems(60) == 60 * 64 * 8 and lib.se_softargmax3d_masked_scratch_elems(120) == 120 * 32 * 8


def test_wrappers_refuse_cpu_tensors():
    G, B, J = 4, 1, 2
    N = G ** 3
    depth = torch.ones((B, 4, 4))
    pix, rng = torch.zeros(N, dtype=torch.int32), torch.ones(N)
    free = torch.ones((B, N), dtype=torch.uint8)
    vol = torch.full((B, J, G, G, G), 1.0 / N)
    coord = torch.zeros((1, G, G, G, 3))
    with pytest.raises(_lib.HipExtensionError):
        _lib.scene_free_mask(depth, pix, rng, free, 4, 4, 0.03, 100.0)
    with pytest.raises(_lib.HipExtensionError):
        _lib.softargmax3d_masked(vol.view(B * J, N), coord.view(N, 3), free, torch.zeros((B * J, 8)),
                                 torch.zeros(B * J, dtype=torch.int32), B * J, J, N)
    with pytest.raises(_lib.HipExtensionError):
        op.scene_free_mask(depth, pix, rng, 4, 4, 0.03, 100.0)
    with pytest.raises(_lib.HipExtensionError):
        op.constrained_joints(vol, coord, free.view(B, G, G, G), torch.zeros((B, J, 3)))


def test_module_method_refuses_cpu_tensors_and_relu_volumes():
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    cfg = load_config()
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    G = net.volume_size
    with pytest.raises(_lib.HipExtensionError):
        net.constrain_to_scene(torch.zeros((1, 15, G, G, G)), torch.zeros((1, 15, 3)), torch.zeros((1, 8, 8)))
    cfg.model.volume_softmax = False
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    with pytest.raises(ValueError):
        net.constrain_to_scene(torch.zeros((1, 15, G, G, G)), torch.zeros((1, 15, 3)), torch.zeros((1, 8, 8)))


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_demo_flag_parses():
    import demo
    assert demo.parse_args([]).constrained_dir is None
    assert demo.parse_args(["--constrained_dir", "out/c"]).constrained_dir == "out/c"


def test_run_sequence_flag_parses():
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    assert run_sequence.parse_args(base).constrain_output is None
    a = run_sequence.parse_args(base + ["--constrain_output", "c.pkl", "--scene_output", "s.pkl"])
    assert a.constrain_output == "c.pkl" and a.scene_output == "s.pkl"


def test_evaluate_skips_constraint_pickles(tmp_path):
    import evaluate
    pose = np.arange(45, dtype=np.float32).reshape(15, 3)
    for name, obj in (("img_1.jpg.pkl", pose), ("img_1.jpg.constraint.pkl", {"free_mass": np.ones(15)}),
                      ("img_1.jpg.stats.pkl", {"sigma": np.ones(15)}), ("img_1.jpg.scene.pkl", {"range": np.ones(15)})):
        with open(tmp_path / name, "wb") as f:
            pickle.dump(obj, f)
    names, poses = evaluate.load_predictions(str(tmp_path))
    assert names == ["img_1.jpg.pkl"] and poses.shape == (1, 15, 3)
