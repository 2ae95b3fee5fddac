"""The most probable pose of a frame: the max-product pass over the kinematic tree of the joint volumes, on the device
(``csrc/skeleton_pose.hip``, ``se_skeleton_pose_f32``): what ``VolumeViterbi`` is to ``VolumeFilter``, for ``SkeletonPrior``.

``SkeletonPrior.couple`` answers one question: per joint, the marginal under the bone-length model.  Its joints are expectations of
those marginals, and fifteen expectations taken from fifteen marginals are not a pose: with a left/right ghost on an arm every marginal
hedges between the two sides and nothing makes the elbow and the wrist choose the same side.  ``SkeletonPose`` answers the other
question: which single configuration of all joints is the most probable?  Joints by depth level, deepest first, with ``m_c`` the
messages of the children of joint j,

    A_j  = p_j prod_c m_c,  M_j = max A_j at peak_j,  s_j = A_j 2^-e with e = ilogb(M_j)      an exact rescaling, no division
    e3_j = the maximum over the bone vector d of s_j(x + d) w_j(d), with the lowest tap that attains it
    m_j  = max((1 - floor) e3_j, (floor / N) max s_j)        the bone, or a jump to the best voxel of joint j

and the walk down from the root's best voxel along the 14 arguments.  Shells, floor and tree are ``SkeletonPrior``'s, unchanged.  A
frame in which some ``M_j`` is not a finite number > 0 is not solved: every joint takes the peak of its own volume.  A single NaN cell
does not cause that: it never wins a maximum and is passed over (``couple`` differs: there a NaN reaches the sums and the frame falls
back).

MODEL NOTE.  The score of an edge is ``max((1 - floor) w(d), floor / N)``, within a factor of 2 of the coupling's sum.  No other
convention is added and none is calibrated.  The limit follows from what it is: the pose is all-or-nothing where the marginals hedge.
A ghost that is slightly stronger than the truth on every joint of a limb is followed on every one of them.  It is an offline tool for
recorded sequences, like ``couple``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .skeleton_prior import KINEMATIC_PARENTS, SkeletonPrior
from .volume_viterbi import MAX_REFINE

POSE_KEYS = ("joints", "index", "coord", "jumped", "solved", "log_score", "bone_error")


class SkeletonPose:
    """``s = SkeletonPose(coord, grid, cuboid_side, bone_lengths, tau=0.03, floor=1e-3, refine=1, parents=KINEMATIC_PARENTS)``;
    ``s.solve(volumes)`` per batch.  Every parameter but ``refine`` is ``SkeletonPrior``'s and a bad one raises its ValueError here,
    before anything touches the device.  ``refine``: the half-width in voxels (0..3) of the window each pose voxel is refined over to
    the centroid of the joint's volume; 0 keeps the voxel centre."""

    def __init__(self, coord, grid, cuboid_side, bone_lengths, tau=0.03, floor=1e-3, refine=1, parents=KINEMATIC_PARENTS):
        self.prior = SkeletonPrior(coord, grid, cuboid_side, bone_lengths, tau=tau, floor=floor, parents=parents)   # the parameters, checked
        if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= int(refine) <= MAX_REFINE:
            raise ValueError(f"refine = {refine!r} (an integer in 0..{MAX_REFINE}) expected")
        self.refine = int(refine)
        p = self.prior
        self.parents, self.bone_lengths, self.taps = p.parents, p.bone_lengths, p.taps
        self.grid, self.cuboid_side, self.tau, self.floor, self.radius, self.joints, self.voxels = \
            p.grid, p.cuboid_side, p.tau, p.floor, p.radius, p.joints, p.voxels
        self._scratch_of = {}

    def _scratch(self, dev, frames, stream):
        """The workspace of one call: one per stream, so that calls on different streams do not share it."""
        need = _lib.skeleton_pose_scratch_bytes(frames, self.joints, self.grid, self.radius)
        key = (str(dev), stream.cuda_stream)
        have = self._scratch_of.get(key)
        if have is None or have.numel() < need:
            have = self._scratch_of[key] = torch.empty(need, device=dev, dtype=torch.uint8)
        return have

    @torch.no_grad()
    def solve(self, volumes, joints=None, stream=None):
        """The most probable pose of each of the B frames ``volumes`` [B,J,G,G,G] (softmaxed, as ``forward()`` returns them).  Returns a
        dict of device tensors: ``joints`` [B,J,3] (each pose voxel refined to the centroid of its joint's volume over the window of
        ``refine`` voxels around it; NaN where a joint has no voxel), ``index`` [B,J] int32 (the pose's flat voxel indices; -1: none),
        ``coord`` [B,J,3] (the voxel centres), ``jumped`` [B,J] bool (the joint was reached by a jump, not along its bone), ``solved``
        [B] bool (False where the frame fell back to the peaks of its own volumes), ``log_score`` [B] float64 (the natural logarithm of
        the pose's score, ln best_0 + ln 2 x the sum of the exponents; NaN where not solved), ``bone_error`` [B,J-1] (| |x_j - x_parent|
        - L_j | of ``joints``, metres); with ``joints`` [B,J,3] given also ``shift`` [B,J] (metres between the pose and the given
        joints) and ``bone_error_before`` [B,J-1].

        ``stream``: the stream to run on (default: the current one).  Shapes are checked before anything touches the device
        (ValueError)."""
        G, J, p = self.grid, self.joints, self.prior
        if not isinstance(volumes, torch.Tensor) or volumes.dim() != 5 or tuple(volumes.shape[1:]) != (J, G, G, G) \
                or volumes.dtype != torch.float32 or volumes.shape[0] < 1:
            raise ValueError("solve: volumes must be a [B,%d,%d,%d,%d] float32 tensor with B >= 1, got %s"
                             % (J, G, G, G, (tuple(volumes.shape), volumes.dtype) if isinstance(volumes, torch.Tensor) else type(volumes)))
        B = int(volumes.shape[0])
        if joints is not None and (not isinstance(joints, torch.Tensor) or tuple(joints.shape) != (B, J, 3)):
            raise ValueError("solve: joints %s, expected %s" % (tuple(getattr(joints, "shape", ())), (B, J, 3)))
        _lib.require_hip(volumes, joints)
        dev = volumes.device
        d = p._device_state(dev)
        stream = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            vol = volumes.contiguous()
            index = torch.empty((B, J), device=dev, dtype=torch.int32)
            jumped = torch.empty((B, J), device=dev, dtype=torch.int32)
            exponent = torch.empty((B, J), device=dev, dtype=torch.int32)
            best_root = torch.empty((B,), device=dev, dtype=torch.float32)
            solved = torch.empty((B,), device=dev, dtype=torch.int32)
            _lib.skeleton_pose(vol, d["taps"], self.parents, index, jumped, exponent, best_root, solved, B, self.voxels, G, self.radius,
                               self.floor, scratch=self._scratch(dev, B, stream))
            out_j = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
            _lib.volume_viterbi_refine(vol if self.refine > 0 else None, d["coord"], index, out_j, B, J, self.voxels, G, self.refine)
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float32)
            coord = torch.where((index >= 0).unsqueeze(-1), d["coord"][index.clamp(min=0).long()], nan)
            log_score = torch.log(best_root.double()) + math.log(2.0) * exponent.double().sum(dim=1)       # NaN where not solved
            result = {"joints": out_j, "index": index, "coord": coord, "jumped": jumped != 0, "solved": solved != 0,
                      "log_score": log_score, "bone_error": p._bone_error(d, out_j)}
            if joints is not None:
                given = joints.to(device=dev, dtype=torch.float32)
                result["shift"] = (out_j - given).norm(dim=-1)
                result["bone_error_before"] = p._bone_error(d, given)
        return result
