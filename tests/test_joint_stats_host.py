"""Host side of the joint statistics: metrics.error_by_confidence, the evaluate.py / demo.py / run_sequence.py flags, and the C ABI
declarations (header, _lib.SIGNATURES, ABI version).  No GPU."""
import os
import pickle
import re

import numpy as np
import pytest

from conftest import ROOT
from sceneego_amd import _lib
from sceneego_amd import metrics as M


def _poses(T=6, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, 15, 3))


def test_error_by_confidence_perfect_rank_correlation():
    gt = _poses()
    n = gt.shape[0] * 15
    err = np.linspace(0.01, 1.0, n).reshape(-1, 15)                 # error of pair k grows with k
    est = gt.copy()
    est[..., 0] += err
    sigma = np.exp(3.0 * err)                                       # monotone, far from linear: ranks only
    r = M.error_by_confidence(est, gt, sigma)
    assert r["spearman"] == pytest.approx(1.0, abs=1e-12) and r["pairs"] == n
    assert np.all(np.diff(r["bin_mean_error"]) > 0) and r["bin_count"].sum() == n
    r = M.error_by_confidence(est, gt, -sigma)
    assert r["spearman"] == pytest.approx(-1.0, abs=1e-12)
    assert np.all(np.diff(r["bin_mean_error"]) < 0)


def test_error_by_confidence_bins_by_hand():
    # one frame of 8 joints, small enough to sort and average by hand
    gt = np.zeros((1, 8, 3))
    est = np.zeros((1, 8, 3))
    errors = np.array([3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 6.0])
    est[0, :, 2] = errors
    sigma = np.array([[0.8, 0.1, 0.3, 0.2, 0.7, 0.4, 0.6, 0.5]])
    # sorted by sigma: joints 1 3 | 2 5 | 7 6 | 4 0  ->  errors (1 1) (4 9) (6 2) (5 3)
    r = M.error_by_confidence(est, gt, sigma, bins=4)
    assert np.array_equal(r["bin_count"], [2, 2, 2, 2])
    assert np.allclose(r["bin_mean_error"], [1.0, 6.5, 4.0, 4.0], rtol=0, atol=1e-15)
    assert np.allclose(r["bin_sigma_max"], [0.2, 0.4, 0.6, 0.8], rtol=0, atol=0)
    # Spearman by hand: ranks of the errors (ties averaged) 4 1.5 5 1.5 6 8 3 7, of sigma 8 1 3 2 7 4 6 5
    re = np.array([4, 1.5, 5, 1.5, 6, 8, 3, 7]) - 4.5
    rs = np.array([8, 1, 3, 2, 7, 4, 6, 5]) - 4.5
    assert r["spearman"] == pytest.approx(float((re * rs).sum() / np.sqrt((re * re).sum() * (rs * rs).sum())), abs=1e-15)
    # 3 bins over 8 pairs: 3 + 3 + 2
    r3 = M.error_by_confidence(est, gt, sigma, bins=3)
    assert np.array_equal(r3["bin_count"], [3, 3, 2])
    assert np.allclose(r3["bin_mean_error"], [(1 + 1 + 4) / 3, (9 + 6 + 2) / 3, 4.0], rtol=0, atol=1e-15)


def test_error_by_confidence_edge_cases():
    gt = _poses(2)
    est = gt + 0.1
    sigma = np.ones((2, 15))
    assert np.isnan(M.error_by_confidence(est, gt, sigma)["spearman"])         # constant sigma: undefined
    sigma = np.arange(30, dtype=np.float64).reshape(2, 15)
    sigma[0, 3] = np.nan                                                        # a NaN volume's joint is left out
    r = M.error_by_confidence(est, gt, sigma)
    assert r["pairs"] == 29 and r["bin_count"].sum() == 29
    with pytest.raises(ValueError):
        M.error_by_confidence(est, gt, sigma[:, :14])
    with pytest.raises(ValueError):
        M.error_by_confidence(est, gt, sigma, bins=0)


def _write_eval_inputs(tmp_path, T=5):
    import evaluate  # noqa: F401  (importable from the repository root)
    rng = np.random.default_rng(3)
    gt = rng.standard_normal((T, 15, 3))
    scale = np.linspace(0.01, 0.3, T * 15).reshape(T, 15)
    pred = gt + scale[..., None] * rng.standard_normal((T, 15, 3))
    pred_dir = tmp_path / "pred"
    pred_dir.mkdir()
    frames = []
    for t in range(T):
        with open(pred_dir / f"img_{t:06d}.jpg.pkl", "wb") as f:
            pickle.dump(pred[t].astype(np.float32), f)
        frames.append({"sigma": scale[t].astype(np.float32), "entropy": np.zeros(15, dtype=np.float32)})
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(gt, f)
    return pred_dir, frames


def test_evaluate_stats_flag(tmp_path, capsys):
    import evaluate
    pred_dir, frames = _write_eval_inputs(tmp_path)
    base = ["--pred_dir", str(pred_dir), "--gt", str(tmp_path / "gt.pkl")]
    r0 = evaluate.main(base)
    plain = capsys.readouterr().out
    assert "by_confidence" not in r0 and len(plain.splitlines()) == 2
    # one pickle with the list of per-frame dicts (run_sequence.py --stats_output)
    with open(tmp_path / "all.stats.pkl", "wb") as f:
        pickle.dump(frames, f)
    r1 = evaluate.main(base + ["--stats", str(tmp_path / "all.stats.pkl")])
    out1 = capsys.readouterr().out
    assert out1.startswith(plain) and len(out1.splitlines()) == 4                 # the existing lines byte for byte, two more
    assert out1.splitlines()[2].startswith("error by sigma quantile") and out1.splitlines()[3].startswith("spearman(error, sigma): ")
    assert len(r1["by_confidence"]["bin_mean_error"]) == 4 and r1["by_confidence"]["spearman"] > 0.5
    assert {k: r1[k] for k in r0} == r0
    # <image name>.stats.pkl beside the predictions (demo.py --stats true): not mistaken for predictions
    for t, fr in enumerate(frames):
        with open(pred_dir / f"img_{t:06d}.jpg.stats.pkl", "wb") as f:
            pickle.dump(fr, f)
    r2 = evaluate.main(base + ["--stats", str(pred_dir), "--stats_bins", "3"])
    out2 = capsys.readouterr().out
    assert out2.startswith(plain) and r2["frames"] == r0["frames"] and len(r2["by_confidence"]["bin_mean_error"]) == 3
    assert r2["by_confidence"]["spearman"] == r1["by_confidence"]["spearman"]
    evaluate.main(base)
    assert capsys.readouterr().out == plain
    with open(tmp_path / "short.pkl", "wb") as f:
        pickle.dump(frames[:-1], f)
    with pytest.raises(SystemExit):
        evaluate.main(base + ["--stats", str(tmp_path / "short.pkl")])


def test_demo_stats_argument():
    import demo
    assert demo.parse_args([]).stats is False
    assert demo.parse_args(["--stats", "true"]).stats is True
    assert demo.parse_args(["--stats", "False"]).stats is False
    with pytest.raises(SystemExit):
        demo.parse_args(["--stats", "maybe"])
    with pytest.raises(SystemExit):
        demo.parse_args(["--vis", "true"])


def test_run_sequence_stats_argument():
    src = open(os.path.join(ROOT, "run_sequence.py")).read()
    assert '"--stats_output"' in src
    import run_sequence
    with pytest.raises(SystemExit):                     # argparse knows the flag: the error is the missing required ones
        run_sequence.main(["--stats_output"])


def test_abi_declares_joint_stats():
    """Fails on the parent commit: the operator did not exist."""
    header = open(os.path.join(ROOT, "include", "sceneego_hip.h")).read()
    assert re.search(r"\bint\s+se_joint_stats_f32\s*\(\s*const float\*\s*prob,\s*const float\*\s*coord,\s*const float\*\s*joints,"
                     r"\s*float\*\s*stats,\s*int\*\s*peak_index,\s*float\*\s*scratch,\s*int rows,\s*int voxels,\s*void\*\s*stream\)\s*;",
                     header)
    assert re.search(r"\blong long\s+se_joint_stats_scratch_elems\s*\(\s*int rows\s*\)\s*;", header)
    res, args = _lib.SIGNATURES["se_joint_stats_f32"]
    assert res is _lib._i and args == [_lib._vp] * 6 + [_lib._i, _lib._i, _lib._vp]
    assert _lib.SIGNATURES["se_joint_stats_scratch_elems"] == (_lib._ll, [_lib._i])
    assert _lib.ABI_VERSION >= 26
    assert "joint_stats" in open(os.path.join(ROOT, "sceneego_amd", "csrc", "build.sh")).read()
    assert os.path.isfile(os.path.join(ROOT, "sceneego_amd", "csrc", "joint_stats.hip"))
