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
