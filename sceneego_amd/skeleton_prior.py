"""Skeleton-coupled joints: belief propagation over the kinematic tree of the joint volumes, on the device
(``csrc/skeleton_prior.hip``, ``se_skeleton_couple_f32``).

``joint_statistics``, ``joint_modes``, ``constrain_to_scene`` and ``VolumeFilter`` treat the fifteen joints of a frame as fifteen
unrelated distributions.  The strongest prior a pose has is the skeleton itself: a wrist lies one forearm away from its elbow.  The
reference forces bone lengths onto a finished pose (``utils/skeleton.py``: ``_skeleton_resize``), after the fact and on point
estimates.  ``SkeletonPrior`` runs sum-product belief propagation over the tree ``KINEMATIC_PARENTS`` on the whole ``[J, G, G, G]``
distributions, with a spherical-shell factor on every edge,

    w_j(d) = exp(-(|d| h - L_j)^2 / (2 tau^2)),  0 beyond 3 tau,  normalised          corr(a, w)(x) = sum_d w(d) a(x + d)
    upward    A_j = p_j prod_c U_c,        U_j = (1 - floor) corr(A_j, w_j) / sum A_j + floor / N
    downward  T_j = p_j D_j prod_c U_c,    b_j = T_j / Z_j,   D_c = (1 - floor) corr(E, w_c) / sum E + floor / N  with E = T_j without U_c

so every joint's marginal ``b_j`` uses what the other joints say about it in the same frame.  The marginals have the shape and the
meaning of the volumes: every per-frame tool and ``VolumeFilter.step`` take them unchanged.  The hip-to-hip line (7, 11) of
``SKELETON_LINES`` closes a loop and is not part of the tree.  A frame one of whose normalisers is not a finite number > 0 falls back to
its own volumes, bit for bit (``coupled`` False).  Frames are independent: no state is carried.

Read it for what it is: a convention, like the ``sigma`` of the filter.  The softmaxed volume is read as a likelihood, a Gaussian shell
of ``tau`` metres as the bone model and ``floor`` as the chance that the bone prior is simply wrong for an edge; none of the three is
calibrated against annotated data, because none ships with the method.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

KINEMATIC_PARENTS = _lib.KINEMATIC_PARENTS
MAX_RADIUS = _lib.SKELETON_MAX_RADIUS
MAX_GRID = _lib.SKELETON_MAX_GRID
MAX_JOINTS = _lib.SKELETON_MAX_JOINTS
SAMPLE_GROUP = 8            # frames per pair of library calls inside SkeletonPrior.sample: bounds the buffer of the upward products


def check_parents(parents):
    """The tree as a tuple of ints: 1..32 joints, parents[0] = 0 and parents[j] < j (ValueError otherwise)."""
    try:
        par = tuple(int(v) for v in parents)
    except (TypeError, ValueError):
        raise ValueError("parents must be a sequence of integers") from None
    if not 1 <= len(par) <= MAX_JOINTS or par[0] != 0 or any(not 0 <= par[j] < j for j in range(1, len(par))):
        raise ValueError(f"parents = {par}: 1..{MAX_JOINTS} joints with parents[0] = 0 and 0 <= parents[j] < j expected")
    return par


def _edge_lengths(bone_lengths, joints):
    """[J] float64 with entry 0 set to 0, from J - 1 values (edges 1..J-1) or J (entry 0 ignored): positive, finite metres."""
    L = np.asarray(bone_lengths, dtype=np.float64).reshape(-1)
    if L.size == joints - 1:
        L = np.concatenate([[0.0], L])
    elif L.size == joints:
        L = L.copy()
        L[0] = 0.0
    else:
        raise ValueError(f"bone_lengths holds {L.size} values, {joints - 1} (edges 1..{joints - 1}) or {joints} expected")
    if not (np.isfinite(L[1:]).all() and (L[1:] > 0).all()):
        raise ValueError(f"bone_lengths must be positive and finite, got {L[1:].tolist()}")
    return L


def default_radius(bone_lengths, tau, voxel_edge):
    """R = ceil((max L + 3 tau) / h): the voxels one block of taps must reach to hold every edge's shell."""
    L = np.asarray(bone_lengths, dtype=np.float64).reshape(-1)
    return int(math.ceil((float(L.max()) + 3.0 * float(tau)) / float(voxel_edge))) if L.size else 0


def shell_taps(lengths, tau, voxel_edge, radius):
    """The dense blocks ``[J, (2R+1)^3]`` float32 of the edges' shells, block j for the bone of ``lengths[j]`` metres (block 0 is unused
    and zero; ``lengths[0]`` is ignored): w(d) = exp(-(|d| h - L)^2 / (2 tau^2)) in float64, exactly 0 where ||d| h - L| > 3 tau,
    normalised to sum 1, then rounded to float32.  Index ((di+R)(2R+1) + dj+R)(2R+1) + dk+R; w(d) = w(-d)."""
    L = np.asarray(lengths, dtype=np.float64).reshape(-1)
    tau, h, R = float(tau), float(voxel_edge), int(radius)
    if L.size < 1 or not (np.isfinite(L[1:]).all() and (L[1:] > 0).all()):
        raise ValueError(f"lengths must be positive and finite (entry 0 is ignored), got {L.tolist()}")
    if not (tau > 0.0 and math.isfinite(tau)) or not (h > 0.0 and math.isfinite(h)):
        raise ValueError(f"tau = {tau} and the voxel edge {h} must be positive and finite")
    if not 0 <= R <= MAX_RADIUS:
        raise ValueError(f"radius = {R} (0..{MAX_RADIUS}) expected")
    if L.size > 1 and R < default_radius(L[1:], tau, h):
        raise ValueError(f"radius = {R} does not hold the longest shell: {default_radius(L[1:], tau, h)} needed")
    ax = np.arange(-R, R + 1, dtype=np.float64)
    dist = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) * h
    out = np.zeros((L.size, (2 * R + 1) ** 3), dtype=np.float32)
    for j in range(1, L.size):
        off = dist - L[j]
        w = np.where(np.abs(off) <= 3.0 * tau, np.exp(-(off * off) / (2.0 * tau * tau)), 0.0)
        total = w.sum()
        if not total > 0.0:
            raise ValueError(f"no voxel lies within 3 tau = {3 * tau} m of the bone length {L[j]} m at a voxel edge of {h} m")
        out[j] = (w / total).reshape(-1).astype(np.float32)
    return out


def estimate_bone_lengths(joints, parents=KINEMATIC_PARENTS):
    """Per-bone median over the frames of ``joints`` [T, J, 3] of the distance between a joint and its parent, in float64; a frame in
    which either end is not finite is skipped for that bone.  Returns [J] float64 with entry 0 set to 0 (NaN where no frame counts)."""
    par = check_parents(parents)
    x = np.asarray(joints, dtype=np.float64)
    if x.ndim != 3 or x.shape[1:] != (len(par), 3):
        raise ValueError(f"joints {x.shape}, expected [T, {len(par)}, 3]")
    out = np.zeros(len(par), dtype=np.float64)
    for j in range(1, len(par)):
        d = np.linalg.norm(x[:, j] - x[:, par[j]], axis=1)
        d = d[np.isfinite(d)]
        out[j] = np.median(d) if d.size else np.nan
    return out


class SkeletonPrior:
    """``s = SkeletonPrior(coord, grid, cuboid_side, bone_lengths, tau=0.03, floor=1e-3, parents=KINEMATIC_PARENTS)``;
    ``s.couple(volumes)`` per batch.

    ``coord``: the voxel-centre coordinates, ``[G,G,G,3]`` or ``[G^3,3]`` (tensor or array; ``VoxelNetwork_depth.skeleton_prior``
    passes the network's own).  ``bone_lengths``: J - 1 values (edges 1..J-1) or J (entry 0 ignored), metres, positive and finite.
    ``tau``: the width of the shell in metres (> 0); ``floor`` in [0, 1].  The taps reach ``radius`` = ceil((max L + 3 tau) / h)
    voxels, h = cuboid_side / grid, which must not exceed min(24, G - 1): the 128^3 grid with full-length bones is out of scope.
    A bad parameter raises ValueError here, before anything touches the device."""

    def __init__(self, coord, grid, cuboid_side, bone_lengths, tau=0.03, floor=1e-3, parents=KINEMATIC_PARENTS):
        grid, cuboid_side, tau, floor = int(grid), float(cuboid_side), float(tau), float(floor)
        self.parents = check_parents(parents)
        J = len(self.parents)
        if not 2 <= grid <= MAX_GRID:
            raise ValueError(f"grid = {grid} (2..{MAX_GRID}) expected")
        if not (cuboid_side > 0.0 and math.isfinite(cuboid_side)):
            raise ValueError(f"cuboid_side = {cuboid_side} must be positive and finite")
        if not (tau > 0.0 and math.isfinite(tau)):
            raise ValueError(f"tau = {tau} must be a finite number > 0")
        if not 0.0 <= floor <= 1.0:
            raise ValueError(f"floor = {floor} must lie in [0, 1]")
        self.bone_lengths = _edge_lengths(bone_lengths, J)
        h = cuboid_side / grid
        radius = default_radius(self.bone_lengths[1:], tau, h)
        if radius > min(MAX_RADIUS, grid - 1):
            raise ValueError(f"the shells reach {radius} voxels of {h:.5f} m; at most min({MAX_RADIUS}, grid - 1) = "
                             f"{min(MAX_RADIUS, grid - 1)} are supported")
        coord = torch.as_tensor(coord) if not isinstance(coord, torch.Tensor) else coord
        if coord.numel() != grid ** 3 * 3 or coord.shape[-1] != 3:
            raise ValueError(f"coord {tuple(coord.shape)} is not [{grid},{grid},{grid},3] or [{grid ** 3},3]")
        self.grid, self.cuboid_side, self.tau, self.floor, self.radius, self.joints = grid, cuboid_side, tau, floor, radius, J
        self.voxels = grid ** 3
        self.taps = shell_taps(self.bone_lengths, tau, h, radius)
        self._coord_src = coord.detach().reshape(self.voxels, 3)
        self._dev = {}

    def _device_state(self, dev):
        key = str(dev)
        if self._dev.get("key") != key:
            self._dev = {"key": key, "coord": self._coord_src.to(device=dev, dtype=torch.float32).contiguous(),
                         "taps": torch.from_numpy(self.taps).to(dev), "scratch": {},
                         "lengths": torch.from_numpy(self.bone_lengths[1:].astype(np.float32)).to(dev),
                         "child": torch.arange(1, self.joints, device=dev), "parent": torch.tensor(self.parents[1:], device=dev,
                                                                                                   dtype=torch.long)}
        return self._dev

    def _scratch(self, d, dev, frames, stream):
        """The workspace of one call: one per stream, so that calls on different streams do not share it."""
        need = _lib.skeleton_couple_scratch_bytes(frames, self.joints, self.grid, self.radius)
        have = d["scratch"].get(stream.cuda_stream)
        if have is None or have.numel() < need:
            have = d["scratch"][stream.cuda_stream] = torch.empty(need, device=dev, dtype=torch.uint8)
        return have

    def _bone_error(self, d, joints):
        return ((joints[:, d["child"]] - joints[:, d["parent"]]).norm(dim=-1) - d["lengths"]).abs()

    @torch.no_grad()
    def couple(self, volumes, joints=None, return_beliefs=False, stream=None):
        """Couple the joints of the B frames ``volumes`` [B,J,G,G,G] (softmaxed, as ``forward()`` returns them).  Returns a dict of
        device tensors: ``joints`` [B,J,3] (the expectation of each coupled marginal), ``evidence`` [B,J] (Z_j: how well joint j's own
        volume agrees with what the rest of the skeleton predicts for it), ``coupled`` [B] bool (False where the frame fell back to
        its own volumes), ``bone_error`` [B,J-1] (| |x_j - x_parent| - L_j | of the coupled joints, metres); with ``joints`` [B,J,3]
        given also ``shift`` [B,J] (metres between the coupled and the given joints) and ``bone_error_before`` [B,J-1] (the same error
        of the given joints); with ``return_beliefs`` also ``beliefs`` [B,J,G,G,G].

        ``stream``: the stream to run on (default: the current one).  Shapes are checked before anything touches the device
        (ValueError)."""
        G, J = self.grid, self.joints
        if not isinstance(volumes, torch.Tensor) or volumes.dim() != 5 or tuple(volumes.shape[1:]) != (J, G, G, G) \
                or volumes.dtype != torch.float32 or volumes.shape[0] < 1:
            raise ValueError("couple: volumes must be a [B,%d,%d,%d,%d] float32 tensor with B >= 1, got %s"
                             % (J, G, G, G, (tuple(volumes.shape), volumes.dtype) if isinstance(volumes, torch.Tensor) else type(volumes)))
        B = int(volumes.shape[0])
        if joints is not None and (not isinstance(joints, torch.Tensor) or tuple(joints.shape) != (B, J, 3)):
            raise ValueError("couple: joints %s, expected %s" % (tuple(getattr(joints, "shape", ())), (B, J, 3)))
        _lib.require_hip(volumes, joints)
        dev = volumes.device
        d = self._device_state(dev)
        stream = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            vol = volumes.contiguous()
            out_j = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
            evidence = torch.empty((B, J), device=dev, dtype=torch.float32)
            coupled = torch.empty((B,), device=dev, dtype=torch.int32)
            beliefs = torch.empty_like(vol) if return_beliefs else None
            _lib.skeleton_couple(vol, d["coord"], d["taps"], self.parents, beliefs, out_j, evidence, coupled, B, self.voxels, G,
                                 self.radius, self.floor, scratch=self._scratch(d, dev, B, stream))
            result = {"joints": out_j, "evidence": evidence, "coupled": coupled != 0, "bone_error": self._bone_error(d, out_j)}
            if return_beliefs:
                result["beliefs"] = beliefs
            if joints is not None:
                given = joints.to(device=dev, dtype=torch.float32)
                result["shift"] = (out_j - given).norm(dim=-1)
                result["bone_error_before"] = self._bone_error(d, given)
        return result

    def _workspace(self, d, dev, stream, name, need, dtype=torch.uint8):
        """A buffer of ``sample``: one per stream and name, grown when a call needs more."""
        key = (stream.cuda_stream, name)
        have = d["scratch"].get(key)
        if have is None or have.numel() < need:
            have = d["scratch"][key] = torch.empty(need, device=dev, dtype=dtype)
        return have

    @torch.no_grad()
    def sample(self, volumes, samples=16, seed=0, first_frame=0, first_sample=0, joints=None, return_upward=False, stream=None):
        """Draw ``samples`` whole poses per frame from the posterior of the coupling's own model, for the B frames ``volumes``
        [B,J,G,G,G] (softmaxed, as ``forward()`` returns them): x_0 ~ A_0, then every child given its parent's voxel, down the tree
        (``se_skeleton_upward_f32`` and ``se_skeleton_sample_f32``; the header states the definition).  Every sample is a member of the
        posterior - its elbow and wrist lie on the same side - and the marginals of the samples are ``couple``'s beliefs.

        Stateless, like ``couple``.  The random numbers are a function of (``seed``, global sample, global frame, joint) alone:
        ``first_frame`` is the global number of ``volumes[0]`` and ``first_sample`` that of the first sample, so a sequence cut into
        batches, or samples drawn in several calls, give the bits of one call.  ``seed``: 0..2^64-1.  The batch is walked in groups
        of at most ``SAMPLE_GROUP`` = 8 frames, which bounds the buffer of the A_j (126 MB at 15 x 64^3); the results do not depend
        on the grouping.

        Returns a dict of device tensors, S = ``samples``: ``index`` [S,B,J] int32 (the flat voxel, -1 where invalid), ``coord``
        [S,B,J,3] (the voxel centres: nothing is refined; NaN where invalid), ``kind`` [S,B,J] int32 (0 a step along the bone, 1 a
        jump of the floor, 2 a fresh draw: the root, or a joint whose parent has no draw), ``valid`` [S,B,J] bool, ``sampled`` [B]
        bool (False where one of the frame's upward sums is not a finite number > 0: nothing is drawn there), ``mean`` [B,J,3] (over
        the valid samples), ``spread`` [B,J] (the root of the trace of the sample covariance over the valid samples, metres; NaN with
        fewer than two), ``bone_error`` [S,B,J-1] (| |x_c - x_parent| - L_c | of every sample, NaN where an end is invalid); with
        ``joints`` [B,J,3] given also ``shift`` [B,J] (metres between ``mean`` and them); with ``return_upward`` also ``upward``
        [B,J,G,G,G] (the A_j) and ``sums`` [B,J].

        ``stream``: the stream to run on (default: the current one).  Shapes and ranges are checked before anything touches the
        device (ValueError)."""
        G, J, N = self.grid, self.joints, self.voxels
        if not isinstance(volumes, torch.Tensor) or volumes.dim() != 5 or tuple(volumes.shape[1:]) != (J, G, G, G) \
                or volumes.dtype != torch.float32 or volumes.shape[0] < 1:
            raise ValueError("sample: volumes must be a [B,%d,%d,%d,%d] float32 tensor with B >= 1, got %s"
                             % (J, G, G, G, (tuple(volumes.shape), volumes.dtype) if isinstance(volumes, torch.Tensor) else type(volumes)))
        B = int(volumes.shape[0])
        if joints is not None and (not isinstance(joints, torch.Tensor) or tuple(joints.shape) != (B, J, 3)):
            raise ValueError("sample: joints %s, expected %s" % (tuple(getattr(joints, "shape", ())), (B, J, 3)))
        try:
            S, seed, first_frame, first_sample = int(samples), int(seed), int(first_frame), int(first_sample)
        except (TypeError, ValueError):
            raise ValueError("sample: samples, seed, first_frame and first_sample must be integers") from None
        if S < 1:
            raise ValueError(f"sample: samples = {S} (>= 1) expected")
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"sample: seed = {seed} (0..2^64-1) expected")
        if first_frame < 0 or first_sample < 0 or first_frame + B > 2 ** 32 or first_sample + S > 2 ** 32:
            raise ValueError(f"sample: first_frame = {first_frame} and first_sample = {first_sample} must not be negative and the "
                             "last frame and sample index must lie below 2^32")
        _lib.require_hip(volumes, joints)
        dev = volumes.device
        d = self._device_state(dev)
        stream = stream if stream is not None else torch.cuda.current_stream(dev)
        group = min(B, SAMPLE_GROUP)
        with torch.cuda.stream(stream):
            vol = volumes.contiguous().reshape(B, J, N)
            index = torch.empty((S, B, J), device=dev, dtype=torch.int32)
            kind = torch.empty((S, B, J), device=dev, dtype=torch.int32)
            sums = torch.empty((B, J), device=dev, dtype=torch.float32)
            sampled = torch.empty((B,), device=dev, dtype=torch.int32)
            if return_upward:
                upward = torch.empty((B, J, N), device=dev, dtype=torch.float32)
            else:
                upward = self._workspace(d, dev, stream, "upward", group * J * N, torch.float32)[:group * J * N].view(group, J, N)
            up_scratch = self._workspace(d, dev, stream, "upward_scratch",
                                         _lib.skeleton_upward_scratch_bytes(group, J, G, self.radius))
            # 8 bytes more: the float64 sums start on an 8-byte boundary whatever the allocator returns
            sm_scratch = self._workspace(d, dev, stream, "sample_scratch", _lib.skeleton_sample_scratch_bytes(group, J, G) + 8)
            sm_scratch = sm_scratch[(-sm_scratch.data_ptr()) % 8:]
            for b0 in range(0, B, group):
                n = min(group, B - b0)
                A = upward[b0:b0 + n] if return_upward else upward[:n]
                _lib.skeleton_upward(vol[b0:b0 + n], d["taps"], self.parents, A, sums[b0:b0 + n], sampled[b0:b0 + n], n, N, G,
                                     self.radius, self.floor, scratch=up_scratch)
                if n == B:
                    idx, knd = index, kind
                else:
                    idx = torch.empty((S, n, J), device=dev, dtype=torch.int32)
                    knd = torch.empty((S, n, J), device=dev, dtype=torch.int32)
                _lib.skeleton_sample(A, sampled[b0:b0 + n], d["taps"], self.parents, idx, knd, n, N, G, self.radius, self.floor, S,
                                     first_sample=first_sample, first_frame=first_frame + b0, seed=seed, scratch=sm_scratch)
                if n != B:
                    index[:, b0:b0 + n] = idx
                    kind[:, b0:b0 + n] = knd
            valid = index >= 0
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float32)
            coord = torch.where(valid[..., None], d["coord"][index.clamp(min=0).long()], nan)
            count = valid.sum(dim=0).to(torch.float32)                                       # [B,J]
            kept = torch.where(valid[..., None], coord, torch.zeros_like(nan))
            mean = torch.where(count[..., None] > 0, kept.sum(dim=0) / count[..., None].clamp(min=1), nan)
            dev2 = torch.where(valid, ((coord - mean[None]) ** 2).sum(dim=-1), torch.zeros_like(nan)).sum(dim=0)
            spread = torch.where(count > 1, (dev2 / (count - 1).clamp(min=1)).sqrt(), nan)
            bone = ((coord[:, :, d["child"]] - coord[:, :, d["parent"]]).norm(dim=-1) - d["lengths"]).abs()
            result = {"index": index, "coord": coord, "kind": kind, "valid": valid, "sampled": sampled != 0, "mean": mean,
                      "spread": spread, "bone_error": bone}
            if joints is not None:
                result["shift"] = (mean - joints.to(device=dev, dtype=torch.float32)).norm(dim=-1)
            if return_upward:
                result["upward"] = upward.view(B, J, G, G, G)
                result["sums"] = sums
        return result
