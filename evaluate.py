#!/usr/bin/env python3
"""Accuracy evaluation of saved predictions: MPJPE / PA-MPJPE of a directory of ``demo.py`` outputs.

The reference evaluates a sequence by collecting ``vol_keypoints_3d`` of every batch (``test.py:42-57``) and passing the list with
the ground truth through ``utils/calculate_errors.py``: ``align_skeleton`` (``:60-91``, per-pose similarity alignment) followed by
``calculate_error`` (``:22-28``).  Here the predictions are the ``<image name>.pkl`` files ``demo.py`` writes (one float32 [15,3]
array each, ``demo.py:88-97`` of the reference) and the ground truth is ONE pickle: either a dict ``{image name or stem: [15,3]}``
or a sequence / array [T,15,3] in the sorted order of the prediction files.  Host-side numpy (``sceneego_amd/metrics.py``); the
dataset classes of the reference (``dataset/test_dataset.py``) are not rebuilt - neither data nor weights ship with it.
"""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_predictions(pred_dir):
    if os.path.isfile(pred_dir):                             # the one pickle of run_sequence.py --output / --track_output / --path_output
        with open(pred_dir, "rb") as f:
            poses = np.asarray(pickle.load(f), dtype=np.float64)
        if poses.ndim != 3 or poses.shape[1:] != (15, 3):
            raise SystemExit(f"{pred_dir}: expected a list of [15,3] poses, got {poses.shape}")
        return ["%06d.pkl" % t for t in range(poses.shape[0])], poses
    names = sorted(n for n in os.listdir(pred_dir)
                   if n.endswith(".pkl") and not n.endswith((".stats.pkl", ".scene.pkl", ".constraint.pkl", ".modes.pkl", ".skeleton.pkl")))
    if not names:
        raise SystemExit(f"no .pkl predictions in {pred_dir}")
    poses = []
    for n in names:
        with open(os.path.join(pred_dir, n), "rb") as f:
            p = np.asarray(pickle.load(f), dtype=np.float64)
        if p.shape != (15, 3):
            raise SystemExit(f"{n}: expected a [15,3] pose, got {p.shape}")
        poses.append(p)
    return names, np.stack(poses)


def load_sigma(path, names):
    """[T,15] sigma of the frames behind the prediction files ``names``: from a directory of ``<image name>.stats.pkl`` files or from
    one pickle holding the list of per-frame dicts in the same (sorted file) order."""
    if os.path.isdir(path):
        frames = []
        for n in names:
            with open(os.path.join(path, n[:-4] + ".stats.pkl"), "rb") as f:
                frames.append(pickle.load(f))
    else:
        with open(path, "rb") as f:
            frames = pickle.load(f)
    if len(frames) != len(names):
        raise SystemExit(f"{path}: statistics of {len(frames)} frames for {len(names)} predictions")
    sigma = np.stack([np.asarray(fr["sigma"], dtype=np.float64) for fr in frames])
    if sigma.shape != (len(names), 15):
        raise SystemExit(f"{path}: expected sigma of shape ({len(names)}, 15), got {sigma.shape}")
    return sigma


def load_scene(path, names):
    """The per-frame scene-check dicts of the frames behind the prediction files ``names``: from a directory of
    ``<image name>.scene.pkl`` files (demo.py --scene_check true) or from the one pickle of run_sequence.py --scene_output."""
    if os.path.isdir(path):
        frames = []
        for n in names:
            with open(os.path.join(path, n[:-4] + ".scene.pkl"), "rb") as f:
                frames.append(pickle.load(f))
    else:
        with open(path, "rb") as f:
            frames = pickle.load(f)
    if len(frames) != len(names):
        raise SystemExit(f"{path}: scene checks of {len(frames)} frames for {len(names)} predictions")
    return frames


def load_modes(path, names):
    """The per-frame joint-mode dicts of the frames behind the prediction files ``names``: from a directory of
    ``<image name>.modes.pkl`` files (demo.py --modes true) or from the one pickle of run_sequence.py --modes_output."""
    if os.path.isdir(path):
        frames = []
        for n in names:
            with open(os.path.join(path, n[:-4] + ".modes.pkl"), "rb") as f:
                frames.append(pickle.load(f))
    else:
        with open(path, "rb") as f:
            frames = pickle.load(f)
    if len(frames) != len(names):
        raise SystemExit(f"{path}: modes of {len(frames)} frames for {len(names)} predictions")
    return frames


def best_of_k(frames, pred, gt):
    """The usual multi-hypothesis figure: per joint the smallest distance to the ground truth over its VALID modes (their ``coord``;
    the prediction itself where a joint has no valid mode), averaged over joints and frames; and the share of the joints that have
    a valid mode whose best mode is not mode 0.  No alignment: the distances are in the frame of the predictions, as MPJPE."""
    best, not_first, have = [], 0, 0
    for fr, p, g in zip(frames, pred, gt):
        valid = np.asarray(fr["valid"]).astype(bool)                                            # [15,K]
        with np.errstate(invalid="ignore"):
            d = np.sqrt(((np.asarray(fr["coord"], dtype=np.float64) - g[:, None, :]) ** 2).sum(axis=2))
        d = np.where(valid, d, np.inf)
        k = d.argmin(axis=1)                                                                    # the lowest slot of the minimum
        any_valid = valid.any(axis=1)
        fallback = np.sqrt(((p - g) ** 2).sum(axis=1))
        best.append(np.where(any_valid, d[np.arange(d.shape[0]), k], fallback))
        not_first += int((any_valid & (k != 0)).sum())
        have += int(any_valid.sum())
    return {"best_of_k_mpjpe": float(np.mean(best)), "best_not_first_share": not_first / have if have else 0.0,
            "joints_with_modes": have}


def load_alternatives(path, count):
    """The per-frame dicts of run_sequence.py --map_alternatives_output, for the ``count`` frames of --map_output."""
    with open(path, "rb") as f:
        frames = pickle.load(f)
    if len(frames) != count:
        raise SystemExit(f"{path}: alternatives of {len(frames)} frames for {count} predictions")
    return frames


def pose_sample_summary(frames, unit):
    """What the pose samples say without a ground truth: the mean of the finite spreads and the mean bone error of the samples."""
    spread = np.concatenate([np.asarray(fr["spread"], dtype=np.float64).reshape(-1) for fr in frames])
    bone = np.concatenate([np.asarray(fr["bone_error"], dtype=np.float64).reshape(-1) for fr in frames])
    out = {"mean_sample_spread": float(spread[np.isfinite(spread)].mean()) if np.isfinite(spread).any() else float("nan"),
           "mean_bone_error": float(bone[np.isfinite(bone)].mean()) if np.isfinite(bone).any() else float("nan"),
           "samples_per_frame": int(np.asarray(frames[0]["valid"]).shape[0]),
           "frames_not_sampled": int(sum(not bool(fr["sampled"]) for fr in frames))}
    print(f"pose samples (the skeleton model's posterior, not calibrated; the spread is no error bar): {out['samples_per_frame']} per "
          f"frame, mean spread {out['mean_sample_spread']:.4f} {unit}, mean bone error {out['mean_bone_error']:.4f} {unit}, "
          f"{out['frames_not_sampled']} frames not sampled")
    return out


def best_of_two(frames, pred, gt):
    """Does the runner-up margin say where the most probable pose is wrong?  Per frame the smaller of the mean joint error of the pose
    and of its runner-up pose (``runner_up_joints``; the pose alone where there is none), averaged over the frames; the share of the
    frames in which the runner-up is the closer one; and the rank correlation of the pose's error and ``runner_up_margin`` over the
    frames with a finite margin (average ranks for ties; NaN when there are fewer than two or either is constant).  No alignment."""
    from sceneego_amd.metrics import _average_ranks
    err = np.sqrt(((pred - gt) ** 2).sum(axis=2)).mean(axis=1)
    best, margins = err.copy(), np.full(len(frames), np.nan)
    for t, fr in enumerate(frames):
        margins[t] = float(fr["runner_up_margin"])
        if int(fr["runner_up"]) >= 0 and np.isfinite(fr["runner_up_joints"]).all():
            other = np.sqrt(((np.asarray(fr["runner_up_joints"], dtype=np.float64) - gt[t]) ** 2).sum(axis=1)).mean()
            best[t] = min(best[t], other)
    ok = np.isfinite(margins)
    rho = float("nan")
    if ok.sum() >= 2:
        re, rm = _average_ranks(err[ok]), _average_ranks(margins[ok])
        re, rm = re - re.mean(), rm - rm.mean()
        den = np.sqrt((re * re).sum() * (rm * rm).sum())
        rho = float((re * rm).sum() / den) if den > 0.0 else rho
    return {"best_of_two_mpjpe": float(best.mean()), "runner_up_closer_share": float((best < err).mean()),
            "spearman_error_margin": rho, "frames_with_margin": int(ok.sum()),
            "mean_runner_up_margin": float(margins[ok].mean()) if ok.any() else float("nan")}


def best_of_two_path(frames, pred, gt):
    """``best_of_two`` per joint, for the per-frame dicts of run_sequence.py --path_alternatives_output: every joint has a trajectory
    and a runner-up of its own.  Per joint and frame the smaller of the error of the path's joint and of ``runner_up_joints`` (the
    path's alone where the runner-up has none), averaged; the share of the joint-frames in which the runner-up is the closer one;
    and the rank correlation of the path's error and the per-frame ``margin`` over the joint-frames with a finite margin."""
    from sceneego_amd.metrics import _average_ranks
    err = np.sqrt(((pred - gt) ** 2).sum(axis=2))                                               # [T,15]
    other = np.sqrt(((np.stack([np.asarray(fr["runner_up_joints"], dtype=np.float64) for fr in frames]) - gt) ** 2).sum(axis=2))
    best = np.where(np.isfinite(other), np.minimum(err, other), err)
    margins = np.stack([np.asarray(fr["margin"], dtype=np.float64) for fr in frames])
    ok = np.isfinite(margins)
    rho = float("nan")
    if ok.sum() >= 2:
        re, rm = _average_ranks(err[ok]), _average_ranks(margins[ok])
        re, rm = re - re.mean(), rm - rm.mean()
        den = np.sqrt((re * re).sum() * (rm * rm).sum())
        rho = float((re * rm).sum() / den) if den > 0.0 else rho
    return {"best_of_two_mpjpe": float(best.mean()), "runner_up_closer_share": float((best < err).mean()),
            "spearman_error_margin": rho, "joint_frames_with_margin": int(ok.sum()),
            "mean_margin": float(margins[ok].mean()) if ok.any() else float("nan"),
            "below_ln2_share": float((margins < np.log(2.0)).mean())}


def match_ground_truth(gt, names):
    if isinstance(gt, dict):
        def find(n):
            stem = n[:-4]                                    # "<image file name>.pkl" -> "<image file name>"
            for k in (stem, os.path.splitext(stem)[0], n):
                if k in gt:
                    return gt[k]
            raise SystemExit(f"ground truth has no entry for {stem}")
        return np.stack([np.asarray(find(n), dtype=np.float64) for n in names])
    arr = np.asarray(gt, dtype=np.float64)
    if arr.shape != (len(names), 15, 3):
        raise SystemExit(f"ground truth shape {arr.shape} does not match {len(names)} predictions of [15,3]")
    return arr


def evaluate(pred, gt, scale=True):
    from sceneego_amd import metrics as M
    return {"frames": int(pred.shape[0]), "mpjpe": M.mpjpe(pred, gt), "pa_mpjpe": M.pa_mpjpe(pred, gt, scale=scale),
            "per_joint": M.per_joint_error(pred, gt).tolist(), "root_trajectory": M.root_trajectory_error(pred, gt)}


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pred_dir", required=True, help="directory of <image name>.pkl files written by demo.py, or the one pickle of "
                    "run_sequence.py --output / --track_output / --path_output")
    ap.add_argument("--gt", default=None, help="pickle: dict name -> [15,3], or [T,15,3] in sorted file order (required unless --bones "
                    "is all that is asked for)")
    ap.add_argument("--no-scale", action="store_true", help="rigid instead of similarity alignment (align_skeleton(scale=False))")
    ap.add_argument("--unit", default="m", help="label only; the numbers are in the unit of the inputs")
    ap.add_argument("--stats", default=None, help="joint statistics of the same frames: a directory of <image name>.stats.pkl files "
                    "(demo.py --stats true) or the one pickle of run_sequence.py --stats_output; adds the error per sigma quantile")
    ap.add_argument("--stats_bins", type=int, default=4, help="number of sigma quantile bins of --stats")
    ap.add_argument("--scene", default=None, help="scene checks of the same frames: a directory of <image name>.scene.pkl files "
                    "(demo.py --scene_check true) or the one pickle of run_sequence.py --scene_output; adds the plausibility summary")
    ap.add_argument("--modes", default=None, help="joint modes of the same frames: a directory of <image name>.modes.pkl files "
                    "(demo.py --modes true) or the one pickle of run_sequence.py --modes_output; adds the best-of-K MPJPE")
    ap.add_argument("--alternatives", default=None, help="with --pred_dir map.pkl: the pickle of run_sequence.py "
                    "--map_alternatives_output for the same frames; adds the best-of-two MPJPE (pose or runner-up) and "
                    "spearman(error, runner-up margin); without --gt only the margins are summarised")
    ap.add_argument("--path_alternatives", default=None, help="with --pred_dir path.pkl: the pickle of run_sequence.py "
                    "--path_alternatives_output for the same frames; adds the best-of-two MPJPE per joint (the path or its runner-up "
                    "trajectory) and spearman(error, margin); without --gt only the margins are summarised")
    ap.add_argument("--samples", default=None, help="with --pred_dir smoothed.pkl: the pickle of run_sequence.py --sample_output for the "
                    "same frames; adds the best-of-N MPJPE per joint (the closest valid sample of every joint) and the rank correlation "
                    "of the smoothed joint's error and the samples' spread")
    ap.add_argument("--pose_samples", default=None, help="the pickle of run_sequence.py --pose_samples_output for the same frames; adds "
                    "the best-of-N MPJPE per joint and per whole pose (the closest sample whose joints are all valid), the samples' "
                    "mean spread and mean bone error; without --gt only the spread and the bone error are summarised")
    ap.add_argument("--bones", nargs="?", const="", default=None, metavar="FILE.npy",
                    help="bone-length summary of the predictions (needs no ground truth): the per-bone standard deviation over the "
                    "sequence and, with FILE.npy (14 or 15 lengths, as run_sequence.py --bone_lengths takes them), the mean absolute "
                    "deviation from them")
    return ap


def bones(pred, path, unit="m"):
    """--bones: metrics.bone_length_summary of the predictions, printed."""
    from sceneego_amd import metrics as M
    s = M.bone_length_summary(pred, np.load(path) if path else None)
    print(M.format_bone_length_summary(s, unit))
    return s


def main(argv=None):
    args = build_parser().parse_args(argv)
    names, pred = load_predictions(args.pred_dir)
    if args.gt is None:
        if args.bones is None and args.alternatives is None and args.path_alternatives is None and args.pose_samples is None:
            raise SystemExit("--gt is required (only --bones, --alternatives, --path_alternatives and --pose_samples work without it)")
        r = {"frames": int(pred.shape[0])}
        if args.path_alternatives is not None:
            margins = np.stack([np.asarray(fr["margin"], dtype=np.float64)
                                for fr in load_alternatives(args.path_alternatives, len(names))])
            ok = np.isfinite(margins)
            r["path_alternatives"] = {"mean_margin": float(margins[ok].mean()) if ok.any() else float("nan"),
                                      "below_ln2_share": float((margins < np.log(2.0)).mean()), "joint_frames_with_margin": int(ok.sum())}
            print("path margin: mean {mean_margin:.4f} over {joint_frames_with_margin} joint-frames, {below_ln2_share:.1%} below "
                  "ln 2".format(**r["path_alternatives"]))
        if args.alternatives is not None:
            margins = np.array([float(fr["runner_up_margin"]) for fr in load_alternatives(args.alternatives, len(names))])
            ok = np.isfinite(margins)
            r["alternatives"] = {"mean_runner_up_margin": float(margins[ok].mean()) if ok.any() else float("nan"),
                                 "below_ln2_share": float((margins < np.log(2.0)).mean()), "frames_with_margin": int(ok.sum())}
            print("runner-up margin: mean {mean_runner_up_margin:.4f} over {frames_with_margin} frames, {below_ln2_share:.1%} below "
                  "ln 2".format(**r["alternatives"]))
        if args.pose_samples is not None:
            r["pose_samples"] = pose_sample_summary(load_alternatives(args.pose_samples, len(names)), args.unit)
        if args.bones is not None:
            r["bones"] = bones(pred, args.bones, args.unit)
        return r
    with open(args.gt, "rb") as f:
        gt = match_ground_truth(pickle.load(f), names)
    r = evaluate(pred, gt, scale=not args.no_scale)
    print(f"{r['frames']} frames  MPJPE {r['mpjpe']:.6f} {args.unit}  PA-MPJPE {r['pa_mpjpe']:.6f} {args.unit}  "
          f"root trajectory {r['root_trajectory']:.6f} {args.unit}")
    print("per joint: " + " ".join(f"{v:.4f}" for v in r["per_joint"]))
    if args.stats is not None:
        from sceneego_amd import metrics as M
        c = M.error_by_confidence(pred, gt, load_sigma(args.stats, names), bins=args.stats_bins)
        r["by_confidence"] = c
        print("error by sigma quantile (low to high): " + " ".join(f"{v:.4f}" for v in c["bin_mean_error"]) + f" {args.unit}")
        print(f"spearman(error, sigma): {c['spearman']:.4f} over {c['pairs']} joints")
    if args.scene is not None:
        from sceneego_amd import metrics as M
        r["scene_summary"] = M.scene_summary(load_scene(args.scene, names))
        print(M.format_scene_summary(r["scene_summary"], args.unit))
    if args.modes is not None:
        r.update(best_of_k(load_modes(args.modes, names), pred, gt))
        print(f"best-of-K MPJPE {r['best_of_k_mpjpe']:.6f} {args.unit} (the closest valid mode of every joint); the best mode is not "
              f"mode 0 in {r['best_not_first_share']:.1%} of {r['joints_with_modes']} joints")
    if args.alternatives is not None:
        a = r["alternatives"] = best_of_two(load_alternatives(args.alternatives, len(names)), pred, gt)
        print(f"best-of-two MPJPE {a['best_of_two_mpjpe']:.6f} {args.unit} (the pose or its runner-up, whichever is closer; the runner-up "
              f"in {a['runner_up_closer_share']:.1%} of the frames); spearman(error, runner-up margin): {a['spearman_error_margin']:.4f} "
              f"over {a['frames_with_margin']} frames")
    if args.path_alternatives is not None:
        a = r["path_alternatives"] = best_of_two_path(load_alternatives(args.path_alternatives, len(names)), pred, gt)
        print(f"best-of-two MPJPE {a['best_of_two_mpjpe']:.6f} {args.unit} (every joint on its path or on its runner-up trajectory, "
              f"whichever is closer; the runner-up in {a['runner_up_closer_share']:.1%} of the joint-frames); spearman(error, margin): "
              f"{a['spearman_error_margin']:.4f} over {a['joint_frames_with_margin']} joint-frames")
    if args.samples is not None:
        from sceneego_amd import metrics as M
        a = r["samples"] = M.best_of_samples(load_alternatives(args.samples, len(names)), pred, gt)
        print(f"best-of-{a['samples_per_joint']} MPJPE {a['best_of_n_mpjpe']:.6f} {args.unit} (the closest valid sample of every joint; "
              f"{a['valid_draws']} of {a['draws']} draws valid); mean spread {a['mean_sample_spread']:.4f} {args.unit}; "
              f"spearman(error, spread): {a['spearman_error_spread']:.4f}")
    if args.pose_samples is not None:
        from sceneego_amd import metrics as M
        frames = load_alternatives(args.pose_samples, len(names))
        a = r["pose_samples"] = {**pose_sample_summary(frames, args.unit), **M.best_of_samples(frames, pred, gt),
                                 **M.best_pose_of_samples(frames, pred, gt)}
        print(f"best-of-{a['samples_per_frame']} MPJPE per joint {a['best_of_n_mpjpe']:.6f} {args.unit} (the closest valid sample of "
              f"every joint), per whole pose {a['best_pose_of_n_mpjpe']:.6f} {args.unit} (the closest sample whose joints are all "
              f"valid; {a['whole_poses']} of {a['poses']} poses whole, {a['frames_without_pose']} frames without one); "
              f"spearman(error, spread): {a['spearman_error_spread']:.4f}")
    if args.bones is not None:
        r["bones"] = bones(pred, args.bones, args.unit)
    return r


if __name__ == "__main__":
    main()
