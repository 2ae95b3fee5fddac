"""Pose error metrics of the reference's evaluation path, vectorised over the sequence.

Restates what ``utils/calculate_errors.py`` computes (``calculate_error`` ``:22-28`` = MPJPE, ``align_skeleton`` ``:60-91`` +
``calculate_error`` = PA-MPJPE, ``calculate_joint_error`` ``:94-100``, ``calculate_slam_error`` ``:31-46``) on top of the
similarity alignment of ``utils/rigid_transform_with_scale.py:18-43`` (Umeyama: ``Q ~ c P R + t`` for row-vector points).
Host-side numpy in float64; only meaningful with real weights and ground truth, neither of which ships with the reference.
"""
from __future__ import annotations

import numpy as np

LEFT_HIP, RIGHT_HIP = 11, 7      # indices in the 15-joint order of utils/skeleton.py:17-19
FOOT_JOINTS = (9, 10, 13, 14)    # Right_ankle, Right_foot, Left_ankle, Left_foot: the ends of the chains 7-8-9-10 and 11-12-13-14


def umeyama(P, Q):
    """Least-squares similarity transform between corresponding point sets.

    P, Q: [..., n, d].  Returns (c [...], R [..., d, d], t [..., d]) with ``Q ~= c * (P @ R) + t``; reflections are excluded
    (the last singular direction is flipped when det < 0), exactly as the reference does."""
    P = np.asarray(P, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    if P.shape != Q.shape:
        raise ValueError(f"shape mismatch {P.shape} vs {Q.shape}")
    n = P.shape[-2]
    mp, mq = P.mean(axis=-2, keepdims=True), Q.mean(axis=-2, keepdims=True)
    cov = np.swapaxes(P - mp, -1, -2) @ (Q - mq) / n
    U, S, Vt = np.linalg.svd(cov)
    flip = (np.linalg.det(U) * np.linalg.det(Vt)) < 0.0
    S = S.copy()
    U = U.copy()
    S[..., -1] = np.where(flip, -S[..., -1], S[..., -1])
    U[..., :, -1] = np.where(flip[..., None], -U[..., :, -1], U[..., :, -1])
    R = U @ Vt
    c = S.sum(axis=-1) / P.var(axis=-2).sum(axis=-1)
    t = mq[..., 0, :] - (mp @ (c[..., None, None] * R))[..., 0, :]
    return c, R, t


def mpjpe(estimated, gt) -> float:
    """Mean per-joint position error over a sequence [T, J, 3] (same unit as the input)."""
    e = np.asarray(estimated, dtype=np.float64) - np.asarray(gt, dtype=np.float64)
    return float(np.linalg.norm(e, axis=-1).mean())


def procrustes_align(estimated, gt, scale: bool = True):
    """Per-pose similarity (or rigid, ``scale=False``: both poses are centred first) alignment of estimated [T,J,3] onto gt.
    Returns (aligned estimate, gt as used)."""
    est = np.array(estimated, dtype=np.float64)
    ref = np.array(gt, dtype=np.float64)
    if not scale:
        est -= est.mean(axis=1, keepdims=True)
        ref -= ref.mean(axis=1, keepdims=True)
    c, R, t = umeyama(est, ref)
    if scale:
        out = c[:, None, None] * (est @ R) + t[:, None, :]
    else:
        out = est @ R + t[:, None, :]
    return out, ref


def pa_mpjpe(estimated, gt, scale: bool = True) -> float:
    aligned, ref = procrustes_align(estimated, gt, scale)
    return mpjpe(aligned, ref)


def per_joint_error(estimated, gt):
    """[J] mean Euclidean error of every joint over the sequence."""
    e = np.asarray(estimated, dtype=np.float64) - np.asarray(gt, dtype=np.float64)
    return np.linalg.norm(e, axis=-1).mean(axis=0)


def root_trajectory_error(estimated, gt, align: bool = False) -> float:
    """Mean error of the hip-centre trajectory; ``align`` fits one similarity transform to the whole trajectory first."""
    est = np.asarray(estimated, dtype=np.float64)
    ref = np.asarray(gt, dtype=np.float64)
    re = 0.5 * (est[:, RIGHT_HIP] + est[:, LEFT_HIP])
    rg = 0.5 * (ref[:, RIGHT_HIP] + ref[:, LEFT_HIP])
    if align:
        c, R, t = umeyama(re, rg)
        re = c * (re @ R) + t
    return float(np.linalg.norm(re - rg, axis=1).mean())


def global_align_sequence(estimated, gt):
    """One similarity transform for the whole sequence (all joints of all frames pooled), reshaped back to [T,J,3]."""
    est = np.asarray(estimated, dtype=np.float64)
    c, R, t = umeyama(est.reshape(-1, 3), np.asarray(gt, dtype=np.float64).reshape(-1, 3))
    return (c * (est.reshape(-1, 3) @ R) + t).reshape(est.shape)


def _average_ranks(x):
    """Ranks 1..n of a 1-D float64 array, ties sharing the mean of their ranks (what Spearman's coefficient is defined on)."""
    order = np.argsort(x, kind="stable")
    xs = x[order]
    start = np.concatenate(([True], xs[1:] != xs[:-1]))          # first element of every run of equal values
    first = np.flatnonzero(start)
    last = np.concatenate((first[1:], [len(xs)])) - 1
    run = np.cumsum(start) - 1
    ranks = np.empty(len(x), dtype=np.float64)
    ranks[order] = 0.5 * (first[run] + last[run]) + 1.0
    return ranks


def error_by_confidence(estimated, gt, sigma, bins: int = 4):
    """Does the soft-argmax's own spread say where it is wrong?  ``estimated`` / ``gt`` [T,J,3], ``sigma`` [T,J] (the ``sigma`` of
    ``op.joint_statistics``; any per-joint spread in any unit works: only its order is used).

    All (frame, joint) pairs with a finite sigma are sorted by sigma (stable) and cut into ``bins`` groups of equal count (the first
    ``n % bins`` groups hold one more): the sigma quantile bins, lowest first.  Returns a dict:
      ``bin_mean_error`` [bins]  mean Euclidean joint error inside each bin (NaN for an empty bin)
      ``bin_sigma_max``  [bins]  the largest sigma of each bin (its upper quantile edge)
      ``bin_count``      [bins]
      ``spearman``               rank correlation of error and sigma (average ranks for ties; NaN when either is constant)
      ``pairs``                  number of pairs used
    numpy, float64."""
    est = np.asarray(estimated, dtype=np.float64)
    ref = np.asarray(gt, dtype=np.float64)
    sig = np.asarray(sigma, dtype=np.float64)
    if est.shape != ref.shape or est.shape[-1] != 3 or sig.shape != est.shape[:-1]:
        raise ValueError(f"shape mismatch: estimated {est.shape}, gt {ref.shape}, sigma {sig.shape}")
    if bins < 1:
        raise ValueError("bins must be >= 1")
    err = np.linalg.norm(est - ref, axis=-1).reshape(-1)
    sig = sig.reshape(-1)
    keep = np.isfinite(sig) & np.isfinite(err)
    err, sig = err[keep], sig[keep]
    order = np.argsort(sig, kind="stable")
    groups = np.array_split(order, bins)
    nan = float("nan")
    out = {"bin_mean_error": np.array([err[g].mean() if len(g) else nan for g in groups], dtype=np.float64),
           "bin_sigma_max": np.array([sig[g].max() if len(g) else nan for g in groups], dtype=np.float64),
           "bin_count": np.array([len(g) for g in groups], dtype=np.int64), "pairs": int(len(err))}
    rho = nan
    if len(err) >= 2:
        re, rs = _average_ranks(err), _average_ranks(sig)
        re -= re.mean()
        rs -= rs.mean()
        den = np.sqrt((re * re).sum() * (rs * rs).sum())
        if den > 0.0:
            rho = float((re * rs).sum() / den)
    out["spearman"] = rho
    return out


def best_of_samples(frames, estimated, gt):
    """The multi-hypothesis figure of trajectory samples.  ``frames``: the per-frame dicts of ``op.volume_samples_to_numpy`` (``coord``
    [S,J,3], ``valid`` [S,J], ``spread`` [J]); ``estimated`` / ``gt`` [T,J,3].  Per joint and frame the smallest distance to the
    ground truth over the joint's VALID samples (every joint has trajectories of its own; the estimate itself where none is valid),
    averaged: ``best_of_n_mpjpe``.  ``mean_sample_spread``: the mean of the finite spreads.  ``spearman_error_spread``: the rank
    correlation of the estimate's error and the spread (``error_by_confidence``).  No alignment.  numpy, float64."""
    est = np.asarray(estimated, dtype=np.float64)
    ref = np.asarray(gt, dtype=np.float64)
    coord = np.stack([np.asarray(fr["coord"], dtype=np.float64) for fr in frames])               # [T,S,J,3]
    valid = np.stack([np.asarray(fr["valid"]).astype(bool) for fr in frames])                    # [T,S,J]
    spread = np.stack([np.asarray(fr["spread"], dtype=np.float64) for fr in frames])             # [T,J]
    if est.shape != ref.shape or coord.shape[0] != est.shape[0] or coord.shape[2:] != est.shape[1:] or spread.shape != est.shape[:2]:
        raise ValueError(f"shape mismatch: estimated {est.shape}, gt {ref.shape}, samples {coord.shape}, spread {spread.shape}")
    with np.errstate(invalid="ignore"):
        d = np.linalg.norm(coord - ref[:, None], axis=-1)
    d = np.where(valid, d, np.inf).min(axis=1)                                                   # [T,J]
    best = np.where(valid.any(axis=1), d, np.linalg.norm(est - ref, axis=-1))
    finite = np.isfinite(spread)
    return {"best_of_n_mpjpe": float(best.mean()), "mean_sample_spread": float(spread[finite].mean()) if finite.any() else float("nan"),
            "spearman_error_spread": error_by_confidence(est, ref, spread, bins=1)["spearman"],
            "samples_per_joint": int(coord.shape[1]), "valid_draws": int(valid.sum()), "draws": int(valid.size)}


def best_pose_of_samples(frames, estimated, gt):
    """The whole-pose figure of pose samples, beside the per-joint ``best_of_samples``.  ``frames``: the per-frame dicts of
    ``op.skeleton_samples_to_numpy`` (``coord`` [S,J,3], ``valid`` [S,J]); ``estimated`` / ``gt`` [T,J,3].  Per frame the smallest
    MEAN joint error over the samples whose joints are ALL valid (the estimate's own mean joint error where there is none), averaged
    over the frames: ``best_pose_of_n_mpjpe``.  A sampled pose is one joint draw, so its joints may not be picked apart: this is the
    honest figure for whole poses, and it is never below ``best_of_n_mpjpe``.  No alignment.  numpy, float64."""
    est = np.asarray(estimated, dtype=np.float64)
    ref = np.asarray(gt, dtype=np.float64)
    coord = np.stack([np.asarray(fr["coord"], dtype=np.float64) for fr in frames])               # [T,S,J,3]
    valid = np.stack([np.asarray(fr["valid"]).astype(bool) for fr in frames])                    # [T,S,J]
    if est.shape != ref.shape or coord.shape[0] != est.shape[0] or coord.shape[2:] != est.shape[1:] or valid.shape != coord.shape[:3]:
        raise ValueError(f"shape mismatch: estimated {est.shape}, gt {ref.shape}, samples {coord.shape}, valid {valid.shape}")
    whole = valid.all(axis=2)                                                                    # [T,S]
    with np.errstate(invalid="ignore"):
        err = np.linalg.norm(coord - ref[:, None], axis=-1).mean(axis=2)                         # [T,S]
    err = np.where(whole, err, np.inf).min(axis=1)
    own = np.linalg.norm(est - ref, axis=-1).mean(axis=1)
    best = np.where(whole.any(axis=1), err, own)
    return {"best_pose_of_n_mpjpe": float(best.mean()), "estimate_mpjpe": float(own.mean()), "samples_per_frame": int(coord.shape[1]),
            "whole_poses": int(whole.sum()), "poses": int(whole.size), "frames_without_pose": int((~whole.any(axis=1)).sum())}


def scene_summary(frames):
    """Physical plausibility of a sequence: ``frames`` is the list of per-frame dicts of ``op.scene_check_to_numpy`` (the keys
    ``penetrating``, ``penetration_depth`` and ``contact`` [15] are used).  Returns a dict:
      ``non_penetration_rate``    share of frames with ``penetrating == False``
      ``mean_penetration_depth``  mean of ``penetration_depth`` over the frames (metres)
      ``foot_contact_rate``       share of frames in which at least one ankle or foot joint (9, 10, 13, 14) is in contact
      ``frames``                  number of frames
    The rates are NaN for an empty list."""
    n = len(frames)
    if n == 0:
        nan = float("nan")
        return {"non_penetration_rate": nan, "mean_penetration_depth": nan, "foot_contact_rate": nan, "frames": 0}
    pen = np.array([bool(np.asarray(f["penetrating"]).reshape(())) for f in frames])
    depth = np.array([float(np.asarray(f["penetration_depth"]).reshape(())) for f in frames], dtype=np.float64)
    contact = np.stack([np.asarray(f["contact"], dtype=bool).reshape(15) for f in frames])
    return {"non_penetration_rate": float((~pen).mean()), "mean_penetration_depth": float(depth.mean()),
            "foot_contact_rate": float(contact[:, list(FOOT_JOINTS)].any(axis=1).mean()), "frames": n}


def format_scene_summary(s, unit="m") -> str:
    """The one line demo / sequence / evaluation tools print for ``scene_summary``."""
    return (f"scene check: {s['frames']} frames  non-penetration rate {s['non_penetration_rate']:.4f}  mean penetration depth "
            f"{s['mean_penetration_depth']:.6f} {unit}  foot contact rate {s['foot_contact_rate']:.4f}")


def scene_field_summary(frames, sample_frames=None, radius_index=None):
    """The beliefs of a sequence against the scene field: ``frames`` is the list of per-frame dicts of ``op.scene_field_to_numpy``
    over ``VoxelNetwork_depth.scene_expectations`` (the keys ``contact_prob`` [15,K] and ``blocked_prob`` [15] are used);
    ``radius_index``: which of the K contact radii counts (default: the second, two voxel spacings with the default radii, or the
    only one).  ``sample_frames``: optionally the per-frame dicts of ``op.scene_field_to_numpy`` over ``op.scene_field_lookup`` of
    sampled poses (``blocked`` [S,15]).  Returns a dict:
      ``mean_foot_contact_prob``  mean contact probability of the ankle and foot joints (9, 10, 13, 14) over the frames
      ``mean_blocked_prob``       mean blocked probability over all joints and frames
      ``frames``                  number of frames
      ``blocked_pose_rate``       with ``sample_frames``: the share of whole sampled poses with any joint in a blocked voxel
      ``poses``                   with ``sample_frames``: the number of sampled poses
    NaN entries (a NaN volume) are left out of the means; the means are NaN for an empty list."""
    n = len(frames)
    nan = float("nan")
    out = {"mean_foot_contact_prob": nan, "mean_blocked_prob": nan, "frames": n}
    if n:
        contact = np.stack([np.asarray(f["contact_prob"], dtype=np.float64).reshape(15, -1) for f in frames])     # [T,15,K]
        k = min(1, contact.shape[2] - 1) if radius_index is None else int(radius_index)
        blocked = np.stack([np.asarray(f["blocked_prob"], dtype=np.float64).reshape(15) for f in frames])
        feet = contact[:, list(FOOT_JOINTS), k]
        if np.isfinite(feet).any():
            out["mean_foot_contact_prob"] = float(np.nanmean(feet))
        if np.isfinite(blocked).any():
            out["mean_blocked_prob"] = float(np.nanmean(blocked))
    if sample_frames is not None:
        poses = [np.asarray(f["blocked"], dtype=bool).reshape(-1, 15).any(axis=1) for f in sample_frames]
        whole = np.concatenate(poses) if poses else np.zeros(0, dtype=bool)
        out["blocked_pose_rate"] = float(whole.mean()) if whole.size else nan
        out["poses"] = int(whole.size)
    return out


def format_scene_field_summary(s) -> str:
    """The one line the sequence tool prints for ``scene_field_summary``."""
    line = (f"scene field: {s['frames']} frames  mean foot contact probability {s['mean_foot_contact_prob']:.4f}  mean blocked "
            f"probability {s['mean_blocked_prob']:.4f}")
    if "blocked_pose_rate" in s:
        line += f"  sampled poses with a blocked joint {s['blocked_pose_rate']:.4f} of {s['poses']}"
    return line


# Skeleton.kinematic_parents of the reference (utils/skeleton.py); sceneego_amd/_lib.py holds the same table beside SKELETON_LINES
KINEMATIC_PARENTS = (0, 0, 1, 2, 0, 4, 5, 1, 7, 8, 9, 4, 11, 12, 13)


def bone_length_summary(poses, bone_lengths=None, parents=KINEMATIC_PARENTS):
    """How constant the bones of a sequence of predictions ``poses`` [T,J,3] are, and, with ``bone_lengths`` (J - 1 values for the
    edges 1..J-1, or J with entry 0 ignored), how far they are from those lengths.  A frame in which either end of a bone is not
    finite is skipped for that bone.  Returns a dict: ``frames``, ``mean`` and ``std`` [J-1] (per bone over the sequence),
    ``mean_std`` (their mean) and, with ``bone_lengths``, ``deviation`` [J-1] (per bone the mean of | length - target |) and
    ``mean_deviation``.  It needs no ground truth, so it shows what ``SkeletonPrior`` does to any prediction directory."""
    x = np.asarray(poses, dtype=np.float64)
    par = [int(v) for v in parents]
    J = len(par)
    if x.ndim != 3 or x.shape[1:] != (J, 3):
        raise ValueError(f"poses {x.shape}, expected [T, {J}, 3]")
    d = np.linalg.norm(x[:, 1:] - x[:, par[1:]], axis=2)                   # [T, J-1]
    out = {"frames": int(x.shape[0]), "mean": np.nanmean(d, axis=0) if d.size else np.zeros(J - 1),
           "std": np.nanstd(d, axis=0) if d.size else np.zeros(J - 1)}
    out["mean_std"] = float(np.mean(out["std"])) if J > 1 else 0.0
    if bone_lengths is not None:
        L = np.asarray(bone_lengths, dtype=np.float64).reshape(-1)
        if L.size == J:
            L = L[1:]
        elif L.size != J - 1:
            raise ValueError(f"bone_lengths holds {L.size} values, {J - 1} or {J} expected")
        dev = np.abs(d - L[None])
        out["deviation"] = np.nanmean(dev, axis=0)
        out["mean_deviation"] = float(np.nanmean(dev))
    return out


def format_bone_length_summary(s, unit="m") -> str:
    text = f"bone lengths over {s['frames']} frames: mean per-bone std {s['mean_std']:.6f} {unit}; per bone: " \
        + " ".join(f"{v:.4f}" for v in s["std"])
    if "deviation" in s:
        text += f"\nmean |length - given| {s['mean_deviation']:.6f} {unit}; per bone: " + " ".join(f"{v:.4f}" for v in s["deviation"])
    return text

