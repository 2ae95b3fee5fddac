"""Host side of the scene check: properties of the float64 model of se_scene_probe_f64 stated without the kernel,
SceneConsistency.probes on CPU tensors, metrics.scene_summary, the demo.py / run_sequence.py / evaluate.py flags and the C ABI
declarations.  No GPU."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import scene_cases as C
import scene_model as M
from conftest import CALIB, ROOT
from sceneego_amd import _lib
from sceneego_amd import metrics
from sceneego_amd.scene_check import SceneConsistency


# ------------------------------------------------------------------------------------------------------------------ the model
def test_a_probe_on_a_scene_point_is_at_distance_zero():
    k = C.inputs("small")
    _, _, s, is_scene, _ = M.scene(k["depth"], k["ray_tab"], C.MIN_Z, C.MAX_DEPTH)
    ns = np.flatnonzero(is_scene[0])[::41]
    assert len(ns) >= 8
    probes = np.zeros((2, len(ns), 3))
    probes[0] = s[0, ns]
    probes[1] = s[0, ns]                                  # frame 1 holds another depth map: the same points are off its surface
    out, index = M.probe(k["depth"], k["ray_tab"], probes, C.MIN_Z, C.MAX_DEPTH)
    assert (out[0, :, 0] == 0.0).all() and np.array_equal(index[0, :, 0], ns.astype(np.int32))
    assert np.array_equal(M.bits(out[0, :, 1:4]), M.bits(s[0, ns]))
    assert (out[1, :, 0] > 0.0).all()
    # the shared case places probe (1, 4) on a scene point of frame 1
    assert C.model("small")[0][1, 4, 0] == 0.0


def test_moving_a_probe_along_its_sight_ray_changes_the_sign_of_the_clearance():
    k = C.inputs("small")
    d, surface, s, is_scene, _ = M.scene(k["depth"], k["ray_tab"], C.MIN_Z, C.MAX_DEPTH)
    ns = np.flatnonzero(is_scene[0])[5::53]
    assert len(ns) >= 6
    rays = k["ray_tab"].reshape(-1, 3)[ns]
    rng = d[0, ns]                                        # unit rays: the range of the scene point is its depth
    probes = np.zeros((2, 2 * len(ns), 3))
    probes[0, :len(ns)] = rays * (0.9 * rng)[:, None]
    probes[0, len(ns):] = rays * (1.1 * rng)[:, None]
    out, index = M.probe(k["depth"], k["ray_tab"], probes, C.MIN_Z, C.MAX_DEPTH)
    assert np.array_equal(index[0, :, 1], np.concatenate([ns, ns]).astype(np.int32))       # each looks along its own pixel's ray
    clearance = out[0, :, 6] - np.sqrt(out[0, :, 4])
    assert (clearance[:len(ns)] > 0).all() and (clearance[len(ns):] < 0).all()
    assert np.abs(clearance[:len(ns)] - 0.1 * rng).max() <= 1e-12 and np.abs(clearance[len(ns):] + 0.1 * rng).max() <= 1e-12


def test_model_edge_rows():
    out, index = C.model("empty_frame")
    assert np.isposinf(out[1, :, 0]).all() and np.isnan(out[1, :, 1:4]).all() and (index[1, :, 0] == -1).all()
    assert np.isfinite(out[1, :, 4:6]).all() and (index[1, :, 1] >= 0).all() and np.isnan(out[1, :, 6]).all()
    assert np.isfinite(out[[0, 2], :, :6]).all() and (index[[0, 2]] >= 0).all()
    out, index = C.model("bad_probe")
    good, _ = C.model("small")
    assert np.isnan(out[0, 3]).all() and np.isnan(out[1, 14]).all() and (index[0, 3] == -1).all() and (index[1, 14] == -1).all()
    keep = np.ones((2, 15), dtype=bool)
    keep[0, 3] = keep[1, 14] = keep[1, 4] = False         # (1, 4) is the probe `small` moves onto a scene point
    assert np.array_equal(M.bits(out[keep]), M.bits(good[keep]))
    # ties: the probes sit on pixels that are not the first of their 4 x 4 block of equal rays; the lowest index is the block's first
    k = C.inputs("ties")
    out, index = C.model("ties")
    W = k["ray_tab"].shape[1]
    for p in (0, 1):
        y, x = divmod(int(index[0, p, 0]), W)
        assert out[0, p, 0] == 0.0 and y % 4 == 0 and x % 4 == 0
    y, x = divmod(int(index[0, 2, 1]), W)
    assert y % 4 == 0 and x % 4 == 0


# ------------------------------------------------------------------------------------------------------------------ probes()
def _numpy_probes(j, S):
    lines = [(0, 1), (0, 4), (1, 2), (2, 3), (4, 5), (5, 6), (1, 7), (4, 11), (7, 8), (8, 9), (9, 10), (11, 12), (12, 13), (13, 14), (7, 11)]
    rows = [j[:, a] + (j[:, b] - j[:, a]) * k / (S + 1) for a, b in lines for k in range(1, S + 1)]
    return np.concatenate([j, np.stack(rows, axis=1)], axis=1) if rows else j


def test_probes_on_cpu_tensors():
    j = np.random.default_rng(2).uniform(-1, 2, size=(3, 15, 3))
    got = SceneConsistency.probes(torch.from_numpy(j), 1)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, 30, 3) and got.device.type == "cpu"
    assert np.array_equal(got.numpy(), _numpy_probes(j, 1))                       # the midpoints: exact
    for S in (0, 2, 3):
        got = SceneConsistency.probes(torch.from_numpy(j.astype(np.float32)), S)
        assert got.dtype == torch.float64 and tuple(got.shape) == (3, 15 + 15 * S, 3)
        np.testing.assert_allclose(got.numpy(), _numpy_probes(j.astype(np.float32).astype(np.float64), S), rtol=0, atol=1e-15)
    assert tuple(SceneConsistency.probes(torch.from_numpy(j[0])).shape) == (1, 60, 3)     # one frame, the default S = 3
    with pytest.raises(ValueError):
        SceneConsistency.probes(torch.from_numpy(j), 4)                           # 75 probes: past the kernel's 64
    with pytest.raises(ValueError):
        SceneConsistency.probes(torch.from_numpy(j[:, :14]), 1)
    assert _lib.SKELETON_LINES[9:11] == ((8, 9), (9, 10)) and len(_lib.SKELETON_LINES) == 15


# ------------------------------------------------------------------------------------------------------------------ summary
def _frame(penetrating, depth, contact_joints):
    c = np.zeros(15, dtype=bool)
    c[list(contact_joints)] = True
    return {"penetrating": np.bool_(penetrating), "penetration_depth": np.float64(depth), "contact": c}


def test_scene_summary():
    frames = [_frame(False, 0.0, [10]), _frame(True, 0.08, [3]), _frame(False, 0.01, []), _frame(False, 0.0, [13, 0])]
    s = metrics.scene_summary(frames)
    assert s == {"non_penetration_rate": 0.75, "mean_penetration_depth": pytest.approx(0.0225), "foot_contact_rate": 0.5, "frames": 4}
    assert metrics.FOOT_JOINTS == (9, 10, 13, 14)
    for j in range(15):
        assert metrics.scene_summary([_frame(False, 0.0, [j])])["foot_contact_rate"] == (1.0 if j in (9, 10, 13, 14) else 0.0)
    empty = metrics.scene_summary([])
    assert empty["frames"] == 0 and np.isnan(empty["non_penetration_rate"])
    line = metrics.format_scene_summary(s)
    assert line.startswith("scene check: 4 frames") and "0.7500" in line and "0.5000" in line


# ------------------------------------------------------------------------------------------------------------------ no CPU fallback
def test_the_scene_check_has_no_cpu_fallback():
    with pytest.raises(_lib.HipExtensionError):
        SceneConsistency(CALIB, frame_size=(24, 40), device="cpu")
    with pytest.raises(_lib.HipExtensionError):
        SceneConsistency(CALIB, frame_size=(24, 40), device="cpu", ray_tab=torch.zeros((24, 40, 3), dtype=torch.float64))
    k = C.inputs("small")
    t = {n: torch.from_numpy(np.array(a)) for n, a in k.items()}
    with pytest.raises(_lib.HipExtensionError):
        _lib.scene_probe(t["depth"], t["ray_tab"], t["probes"], torch.empty((2, 15, 8), dtype=torch.float64),
                         torch.empty((2, 15, 2), dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ command lines
def test_demo_scene_check_argument():
    import demo
    assert demo.parse_args([]).scene_check is False
    assert demo.parse_args(["--scene_check", "true"]).scene_check is True
    assert demo.parse_args(["--scene_check", "False"]).scene_check is False
    with pytest.raises(SystemExit):
        demo.parse_args(["--scene_check", "maybe"])


def test_run_sequence_scene_output_argument(capsys):
    import run_sequence
    with pytest.raises(SystemExit):
        run_sequence.main(["--help"])
    assert "--scene_output" in capsys.readouterr().out
    with pytest.raises(SystemExit):                     # argparse knows the flag: the error is the missing required ones
        run_sequence.main(["--scene_output", "x.pkl"])
    assert "unrecognized" not in capsys.readouterr().err


def test_evaluate_scene_flag(tmp_path, capsys):
    import evaluate
    rng = np.random.default_rng(4)
    T = 4
    gt = rng.standard_normal((T, 15, 3))
    pred_dir = tmp_path / "pred"
    pred_dir.mkdir()
    frames = [_frame(False, 0.0, [9]), _frame(True, 0.2, []), _frame(False, 0.0, [14]), _frame(True, 0.04, [1])]
    for t in range(T):
        with open(pred_dir / f"img_{t:06d}.jpg.pkl", "wb") as f:
            pickle.dump((gt[t] + 0.01).astype(np.float32), f)
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(gt, f)
    base = ["--pred_dir", str(pred_dir), "--gt", str(tmp_path / "gt.pkl")]
    r0 = evaluate.main(base)
    plain = capsys.readouterr().out
    assert "scene_summary" not in r0 and len(plain.splitlines()) == 2
    with open(tmp_path / "all.scene.pkl", "wb") as f:                              # run_sequence.py --scene_output
        pickle.dump(frames, f)
    r1 = evaluate.main(base + ["--scene", str(tmp_path / "all.scene.pkl")])
    out1 = capsys.readouterr().out
    assert out1.startswith(plain) and len(out1.splitlines()) == 3
    assert out1.splitlines()[2] == metrics.format_scene_summary(metrics.scene_summary(frames))
    assert r1["scene_summary"] == {"non_penetration_rate": 0.5, "mean_penetration_depth": pytest.approx(0.06), "foot_contact_rate": 0.5,
                                   "frames": 4}
    # <image name>.scene.pkl beside the predictions (demo.py --scene_check true): not mistaken for predictions
    for t, fr in enumerate(frames):
        with open(pred_dir / f"img_{t:06d}.jpg.scene.pkl", "wb") as f:
            pickle.dump(fr, f)
    names, _ = evaluate.load_predictions(str(pred_dir))
    assert names == [f"img_{t:06d}.jpg.pkl" for t in range(T)]
    r2 = evaluate.main(base + ["--scene", str(pred_dir)])
    assert capsys.readouterr().out == out1 and r2["scene_summary"] == r1["scene_summary"] and r2["frames"] == r0["frames"]
    evaluate.main(base)
    assert capsys.readouterr().out == plain
    with open(tmp_path / "short.pkl", "wb") as f:
        pickle.dump(frames[:-1], f)
    with pytest.raises(SystemExit):
        evaluate.main(base + ["--scene", str(tmp_path / "short.pkl")])
    with pytest.raises(SystemExit):
        evaluate.main(["--help"])
    assert "--scene" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_abi_declares_the_scene_probe():
    header = open(os.path.join(ROOT, "include", "sceneego_hip.h")).read()
    assert re.search(r"\blong long\s+se_scene_probe_scratch_bytes\s*\(\s*int batch,\s*int height,\s*int width,\s*int probes\s*\)\s*;", header)
    assert re.search(r"\bint\s+se_scene_probe_f64\s*\(\s*const float\*\s*depth,\s*const double\*\s*ray_tab,\s*const double\*\s*probes,"
                     r"\s*double\*\s*out,\s*int\*\s*index,\s*void\*\s*scratch,\s*long long scratch_bytes,\s*int batch,\s*int depth_h,"
                     r"\s*int depth_w,\s*int height,\s*int width,\s*int n_probes,\s*double min_z,\s*double max_depth,\s*void\*\s*stream\)\s*;",
                     header)
    res, args = _lib.SIGNATURES["se_scene_probe_f64"]
    assert res is _lib._i and args == [_lib._vp] * 6 + [_lib._ll] + [_lib._i] * 6 + [_lib._d, _lib._d, _lib._vp]
    assert _lib.SIGNATURES["se_scene_probe_scratch_bytes"] == (_lib._ll, [_lib._i] * 4)
    assert _lib.ABI_VERSION >= 28
    build = open(os.path.join(ROOT, "sceneego_amd", "csrc", "build.sh")).read()
    assert re.search(r'"\$f" = scene_probe \] && extra="-ffp-contract=off"', build)
    lib = _lib.load()
    one = lib.se_scene_probe_scratch_bytes(1, 1024, 1280, 1)
    assert one > 0 and lib.se_scene_probe_scratch_bytes(8, 1024, 1280, 60) == 8 * 60 * one
    assert lib.se_scene_probe_scratch_bytes(0, 1024, 1280, 60) < 0 and lib.se_scene_probe_scratch_bytes(1, 24, 40, 65) < 0
