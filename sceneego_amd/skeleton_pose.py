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

``SkeletonPose.alternatives`` says how close the other side was: the downward max-product pass (``se_skeleton_alternatives_f32``) gives
the max-marginal of every joint, the score of the best whole pose that puts the joint at a voxel, and from it per joint the best pose
that moves the joint out of a window around its voxel, with its log margin, and the runner-up pose of the frame.  The conventions are
``solve``'s; the window on one joint is one more.
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

    def _scratch(self, dev, frames, stream, sizer=_lib.skeleton_pose_scratch_bytes):
        """The workspace of one call: one per stream, so that calls on different streams do not share it."""
        need = sizer(frames, self.joints, self.grid, self.radius)
        key = (str(dev), stream.cuda_stream)
        have = self._scratch_of.get(key)
        if have is None or have.numel() < need:
            have = self._scratch_of[key] = torch.empty(need, device=dev, dtype=torch.uint8)
        return have

    def _checked(self, what, volumes, joints):
        """B, or ValueError: the shapes of a call, checked before anything touches the device."""
        G, J = self.grid, self.joints
        if not isinstance(volumes, torch.Tensor) or volumes.dim() != 5 or tuple(volumes.shape[1:]) != (J, G, G, G) \
                or volumes.dtype != torch.float32 or volumes.shape[0] < 1:
            raise ValueError("%s: volumes must be a [B,%d,%d,%d,%d] float32 tensor with B >= 1, got %s"
                             % (what, J, G, G, G, (tuple(volumes.shape), volumes.dtype) if isinstance(volumes, torch.Tensor) else type(volumes)))
        B = int(volumes.shape[0])
        if joints is not None and (not isinstance(joints, torch.Tensor) or tuple(joints.shape) != (B, J, 3)):
            raise ValueError("%s: joints %s, expected %s" % (what, tuple(getattr(joints, "shape", ())), (B, J, 3)))
        return B

    def _pose_result(self, d, vol, index, jumped, exponent, best_root, solved, joints):
        """What ``solve`` returns, from the outputs of the upward pass."""
        B, J, p, dev = int(vol.shape[0]), self.joints, self.prior, vol.device
        out_j = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
        _lib.volume_viterbi_refine(vol if self.refine > 0 else None, d["coord"], index, out_j, B, J, self.voxels, self.grid, self.refine)
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
        B = self._checked("solve", volumes, joints)
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
            result = self._pose_result(d, vol, index, jumped, exponent, best_root, solved, joints)
        return result

    @torch.no_grad()
    def alternatives(self, volumes, separation=2, joints=None, return_max_marginals=False, stream=None):
        """How close the second-best pose was: the downward max-product pass behind ``solve`` (``se_skeleton_alternatives_f32``).  It
        gives per joint and voxel the max-marginal, the score of the best whole pose that puts the joint there, and per joint (the
        anchor) the best pose that places it more than ``separation`` voxels (Chebyshev, an int >= 0) from its voxel in the most
        probable pose.  Returns everything ``solve`` returns, with the same bits, and

        ``complete`` [B] bool (False where the frame is not solved or a downward message has no finite maximum > 0: the entries below
        are then NaN, -1 or False), ``margin`` [B,J] float64 (ln of the pose's score over the anchor's alternative; +inf: there is no
        alternative), ``alt_log_score`` [B,J] float64 (-inf: none), ``alt_index`` [B,J] int32 and ``alt_coord`` [B,J,3] (the anchor's
        voxel in its alternative), ``alt_pose_index`` [B,J,J] int32 and ``alt_pose_jumped`` [B,J,J] bool (anchor, joint),
        ``alt_pose_joints`` [B,J,J,3] (refined as ``joints``), ``max_marginal_peak_index`` [B,J] int32, ``pose_is_peak`` [B,J] bool
        (the max-marginal of the joint peaks at the pose's voxel), ``runner_up`` [B] int64 (the anchor whose alternative scores best,
        the lowest among equals; -1: none), ``runner_up_joints`` [B,J,3], ``runner_up_margin`` [B] float64 and
        ``runner_up_bone_error`` [B,J-1] (NaN joints and errors where there is none); with ``return_max_marginals`` also
        ``max_marginals`` [B,J,G,G,G], each joint's volume divided by its largest value.

        The conventions and the lack of calibration are ``solve``'s; the window on one joint is a convention of this call."""
        G, J, p, N = self.grid, self.joints, self.prior, self.voxels
        B = self._checked("alternatives", volumes, joints)
        if isinstance(separation, bool) or not isinstance(separation, (int, np.integer)) or separation < 0:
            raise ValueError(f"alternatives: separation = {separation!r} (an integer >= 0) expected")
        separation = int(separation)
        _lib.require_hip(volumes, joints)
        dev = volumes.device
        d = p._device_state(dev)
        stream = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            vol = volumes.contiguous()
            i32 = {k: torch.empty(s, device=dev, dtype=torch.int32) for k, s in
                   (("index", (B, J)), ("jumped", (B, J)), ("exponent", (B, J)), ("solved", (B,)), ("down_exponent", (B, J)),
                    ("mm_peak", (B, J)), ("alt_index", (B, J)), ("alt_pose", (B, J, J)), ("alt_jumped", (B, J, J)), ("complete", (B,)))}
            f32 = {k: torch.empty(s, device=dev, dtype=torch.float32) for k, s in
                   (("best_root", (B,)), ("mm_best", (B, J)), ("pose_value", (B, J)), ("alt_value", (B, J)))}
            mm = torch.empty((B, J, N), device=dev, dtype=torch.float32) if return_max_marginals else None
            _lib.skeleton_alternatives(vol, d["taps"], self.parents, separation, frames=B, voxels=N, grid=G, radius=self.radius,
                                       floor=self.floor, max_marginals=mm,
                                       scratch=self._scratch(dev, B, stream, _lib.skeleton_alternatives_scratch_bytes), **i32, **f32)
            result = self._pose_result(d, vol, i32["index"], i32["jumped"], i32["exponent"], f32["best_root"], i32["solved"], joints)
            complete, has = i32["complete"] != 0, i32["alt_index"] >= 0
            # the exponents, summed in integers: Esub_j over the subtree of j, F_j over everything outside it
            e, q = i32["exponent"].long(), i32["down_exponent"].long()
            kids = [[c for c in range(1, J) if self.parents[c] == j] for j in range(J)]
            esub = [e[:, j] for j in range(J)]
            for j in range(J - 1, 0, -1):
                esub[self.parents[j]] = esub[self.parents[j]] + esub[j]
            outer = [torch.zeros_like(e[:, 0]) for _ in range(J)]
            for c in range(1, J):
                outer[c] = outer[self.parents[c]] + q[:, c]
                for o in kids[self.parents[c]]:
                    if o != c:
                        outer[c] = outer[c] + esub[o]
            shift = math.log(2.0) * (torch.stack(esub, dim=1) + torch.stack(outer, dim=1)).double()
            inf = torch.full((), float("inf"), device=dev, dtype=torch.float64)
            none = torch.where(complete.unsqueeze(-1), inf, inf * 0)                              # +inf, or NaN where not complete
            ln_alt = torch.log(f32["alt_value"].double())
            margin = torch.where(has, torch.log(f32["mm_best"].double()) - ln_alt, none)
            alt_log_score = torch.where(has, ln_alt + shift, -none)
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float32)
            alt_coord = torch.where(has.unsqueeze(-1), d["coord"][i32["alt_index"].clamp(min=0).long()], nan)
            alt_joints = torch.empty((B, J, J, 3), device=dev, dtype=torch.float32)
            for a in range(J):                                                                   # one anchor's poses: [B, J] voxels
                out_a = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
                _lib.volume_viterbi_refine(vol if self.refine > 0 else None, d["coord"], i32["alt_pose"][:, a].contiguous(), out_a, B, J,
                                           N, G, self.refine)
                alt_joints[:, a] = out_a
            scores = torch.where(has, alt_log_score, -inf)
            best = scores.max(dim=1, keepdim=True).values
            anchors = torch.arange(J, device=dev).unsqueeze(0)
            first = torch.where(has & (scores == best), anchors, J).min(dim=1).values             # the lowest among equals
            runner = torch.where(first < J, first, -1)
            pick = runner.clamp(min=0)
            rows = torch.arange(B, device=dev)
            runner_joints = torch.where((runner >= 0).view(B, 1, 1), alt_joints[rows, pick], nan)
            result.update({"complete": complete, "margin": margin, "alt_log_score": alt_log_score, "alt_index": i32["alt_index"],
                           "alt_coord": alt_coord, "alt_pose_index": i32["alt_pose"], "alt_pose_jumped": i32["alt_jumped"] != 0,
                           "alt_pose_joints": alt_joints, "max_marginal_peak_index": i32["mm_peak"],
                           "pose_is_peak": complete.unsqueeze(-1) & (i32["mm_peak"] == i32["index"]), "runner_up": runner,
                           "runner_up_joints": runner_joints,
                           "runner_up_margin": torch.where(runner >= 0, margin[rows, pick], none[:, 0]),
                           "runner_up_bone_error": p._bone_error(d, runner_joints)})
            if return_max_marginals:
                top = f32["mm_best"].unsqueeze(-1)                                              # NaN where not complete: left as it is
                result["max_marginals"] = (mm / torch.where(top > 0, top, torch.ones_like(top))).view(B, J, G, G, G)
        return result
