"""A recursive Bayes filter over the joint volumes of a sequence, on the device (``csrc/volume_filter.hip``, ``se_volume_filter_f32``).

``VoxelNetwork_depth.joint_modes`` says where the peaks of a joint's distribution are in one frame and ``track.select_modes`` picks
among at most K of them on the host after the fact.  ``VolumeFilter`` keeps the whole ``[J, G, G, G]`` grid instead: per joint a
belief ``b`` over the voxels that is blurred by a motion model, multiplied by the next frame's volume and normalised,

    q = blur3(b)                      separable truncated Gaussian, taps w[-R..R], zero-padded: what leaves the grid is lost
    u = (1 - floor) q + floor / N     the uniform floor: the chance of a jump to anywhere
    a = p u,  Z = sum a,  b' = a / Z  (a row without a prior, or whose Z is not a finite number > 0, restarts with b' = p)

so "the joint was here a frame ago" weighs the two lobes of an ambiguous volume.  The beliefs have the shape and the meaning of the
volumes: ``joint_statistics``, ``joint_modes``, ``constrain_to_scene``, ``render_volumes`` and ``overlay_volumes`` take them unchanged.

Read it for what it is: a convention, like the ``sigma`` of ``select_modes`` and the thresholds of the scene check.  The softmaxed
volume is read as a likelihood, a Gaussian step of ``sigma`` metres per frame as the motion model and ``floor`` as the chance of a
jump; none of the three is calibrated against annotated data, because none ships with the method.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

MAX_RADIUS = _lib.FILTER_MAX_RADIUS
MAX_GRID = _lib.FILTER_MAX_GRID
FILTER_KEYS = ("joints", "evidence", "restarted")


def default_radius(sigma, grid, cuboid_side):
    """min(16, G - 1, ceil(3 sigma / h)) with h = cuboid_side / G the voxel edge."""
    h = float(cuboid_side) / int(grid)
    return int(min(MAX_RADIUS, int(grid) - 1, math.ceil(3.0 * float(sigma) / h)))


def gaussian_taps(sigma, radius, voxel_edge):
    """The 2 radius + 1 taps w[d] = exp(-(d h)^2 / (2 sigma^2)), d = -radius..radius: float64, normalised to sum 1, then rounded to
    float32.  ``sigma == 0`` or ``radius == 0`` gives [1]: the belief does not move."""
    sigma, radius, h = float(sigma), int(radius), float(voxel_edge)
    if not sigma >= 0.0:
        raise ValueError(f"sigma = {sigma} must be >= 0")
    if radius < 0 or not h > 0.0:
        raise ValueError(f"radius = {radius} must be >= 0 and the voxel edge {h} positive")
    if sigma == 0.0 or radius == 0:
        w = np.zeros(2 * radius + 1, dtype=np.float64)
        w[radius] = 1.0
        return w.astype(np.float32)
    d = np.arange(-radius, radius + 1, dtype=np.float64) * h
    w = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32)


class VolumeFilter:
    """``f = VolumeFilter(coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3)``; ``f.step(volumes)`` per batch.

    ``coord``: the voxel-centre coordinates, ``[G,G,G,3]`` or ``[G^3,3]`` (tensor or array; ``VoxelNetwork_depth.volume_filter`` passes
    the network's own).  ``sigma``: metres a joint is assumed to move per frame (>= 0); ``radius``: voxels the step is truncated at,
    0..min(16, G - 1), default ``min(16, G - 1, ceil(3 sigma / h))``; ``floor`` in [0, 1].  A bad parameter raises ValueError here,
    before anything touches the device.  The filter is one track: the state (one belief per joint) is carried from call to call."""

    def __init__(self, coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3):
        grid, cuboid_side, sigma, floor = int(grid), float(cuboid_side), float(sigma), float(floor)
        if not 2 <= grid <= MAX_GRID:
            raise ValueError(f"grid = {grid} (2..{MAX_GRID}) expected")
        if not cuboid_side > 0.0:
            raise ValueError(f"cuboid_side = {cuboid_side} must be positive")
        if not sigma >= 0.0 or math.isinf(sigma):
            raise ValueError(f"sigma = {sigma} must be a finite number >= 0")
        if not 0.0 <= floor <= 1.0:
            raise ValueError(f"floor = {floor} must lie in [0, 1]")
        if radius is None:
            radius = default_radius(sigma, grid, cuboid_side)
        if int(radius) != radius or not 0 <= int(radius) <= min(MAX_RADIUS, grid - 1):
            raise ValueError(f"radius = {radius} (an integer in 0..{min(MAX_RADIUS, grid - 1)}) expected")
        coord = torch.as_tensor(coord) if not isinstance(coord, torch.Tensor) else coord
        if coord.numel() != grid ** 3 * 3 or coord.shape[-1] != 3:
            raise ValueError(f"coord {tuple(coord.shape)} is not [{grid},{grid},{grid},3] or [{grid ** 3},3]")
        self.grid, self.cuboid_side, self.sigma, self.radius, self.floor = grid, cuboid_side, sigma, int(radius), floor
        self.voxels = grid ** 3
        self.taps = gaussian_taps(sigma, self.radius, cuboid_side / grid)
        self.frames_seen = 0
        self.rows = None                 # the joints per frame, fixed by the first step
        self._coord_src = coord.detach().reshape(self.voxels, 3)
        self._prior = None               # host: which rows have a prior
        self._dev = {}                   # device state, built by the first step
        self._event = None               # recorded behind the last step: the next one waits for it, whatever stream it runs on

    # ------------------------------------------------------------------------------------------------------------------------
    def reset(self, rows=None):
        """Forget the prior of ``rows`` (an iterable of joint indices; default: all, which also zeroes ``frames_seen``): those rows
        restart at the next frame with ``b = p``.  Nothing is queued on the device."""
        if rows is None:
            self.frames_seen = 0
            if self._prior is not None:
                self._prior[:] = False
            return
        idx = [int(r) for r in rows]
        n = self.rows
        if n is None:
            if idx:
                raise ValueError("reset(rows=...) before the first step: the filter has no rows yet")
            return
        if any(r < 0 or r >= n for r in idx):
            raise ValueError(f"reset: rows {idx} outside 0..{n - 1}")
        self._prior[idx] = False

    def _check_step(self, volumes, joints):
        G = self.grid
        if not isinstance(volumes, torch.Tensor) or volumes.dim() != 5 or tuple(volumes.shape[2:]) != (G, G, G) \
                or volumes.dtype != torch.float32:
            raise ValueError("step: volumes must be a [B,J,%d,%d,%d] float32 tensor, got %s"
                             % (G, G, G, (tuple(volumes.shape), volumes.dtype) if isinstance(volumes, torch.Tensor) else type(volumes)))
        B, J = int(volumes.shape[0]), int(volumes.shape[1])
        if B < 1 or J < 1 or J > 65535:
            raise ValueError(f"step: {B} frames of {J} joints; at least one frame and 1..65535 joints expected")
        if self.rows is not None and J != self.rows:
            raise ValueError(f"step: {J} joints per frame, the filter's state holds {self.rows}")
        if joints is not None and (not isinstance(joints, torch.Tensor) or tuple(joints.shape) != (B, J, 3)):
            raise ValueError("step: joints %s, expected %s" % (tuple(getattr(joints, "shape", ())), (B, J, 3)))
        return B, J

    def _device_constants(self, dev, J):
        """``coord``, ``taps`` and a row of ones on ``dev``: what every operator on the filter's model reads.  ``VolumeSmoother`` and
        ``VolumeViterbi`` take them from here; the belief and its workspace are added by the filter's own first step."""
        key = str(dev)
        if self._dev.get("key") != key:
            if self._dev and self._prior is not None and self._prior.any():
                raise ValueError(f"step: the filter's state is on {self._dev['key']}, the volumes on {key}")
            self._dev = {
                "key": key,
                "coord": self._coord_src.to(device=dev, dtype=torch.float32).contiguous(),
                "taps": torch.from_numpy(self.taps).to(dev),
                "ones": torch.ones(J, device=dev, dtype=torch.int32),
            }
        return self._dev

    def _device_state(self, dev, J):
        d = self._device_constants(dev, J)
        if "state" not in d:
            d["state"] = torch.empty((J, self.voxels), device=dev, dtype=torch.float32)
            d["scratch"] = torch.empty(_lib.volume_filter_scratch_bytes(J, self.grid, self.radius), device=dev, dtype=torch.uint8)
        return d

    @property
    def state(self):
        """The belief after the last step, [J,G,G,G] on the device (None before the first): the filter's own buffer, not a copy."""
        s = self._dev.get("state")
        return None if s is None else s.view(-1, self.grid, self.grid, self.grid)

    @torch.no_grad()
    def step(self, volumes, joints=None, return_beliefs=False, stream=None):
        """Filter the B consecutive frames ``volumes`` [B,J,G,G,G] (softmaxed, as ``forward()`` returns them) of the track.  Returns
        a dict of device tensors: ``joints`` [B,J,3] (the expectation of each belief), ``evidence`` [B,J] (Z: the predictive
        likelihood of the frame, 1 / G^3 is chance; NaN where the row had no prior), ``restarted`` [B,J] bool, with
        ``return_beliefs`` also ``beliefs`` [B,J,G,G,G] and with ``joints`` [B,J,3] given also ``shift`` [B,J]: metres between the
        filtered and the given joints.

        ``stream``: the stream to run on (default: the current one).  Every call records an event behind itself and the next call
        makes its stream wait for it, so the state stays correct when consecutive batches run on different streams
        (``pipeline.PipelinedForward``); the caller only has to issue the calls in frame order.  Shapes are checked before anything
        touches the device (ValueError)."""
        B, J = self._check_step(volumes, joints)
        _lib.require_hip(volumes, joints)
        dev = volumes.device
        if self.rows is None:
            self.rows = J
            self._prior = np.zeros(J, dtype=bool)
        d = self._device_state(dev, J)
        stream = stream if stream is not None else torch.cuda.current_stream(dev)
        if self._event is not None:
            stream.wait_event(self._event)
        with torch.cuda.stream(stream):
            vol = volumes.contiguous()
            out_j = torch.empty((B, J, 3), device=dev, dtype=torch.float32)
            evidence = torch.empty((B, J), device=dev, dtype=torch.float32)
            restarted = torch.empty((B, J), device=dev, dtype=torch.int32)
            beliefs = torch.empty_like(vol) if return_beliefs else None
            if self._prior.all():
                have = d["ones"]
            elif not self._prior.any():
                have = None
            else:
                have = torch.from_numpy(self._prior.astype(np.int32)).to(dev)
            _lib.volume_filter(vol, d["coord"], d["taps"], d["state"], beliefs, out_j, evidence, restarted, B, J, self.voxels,
                               self.grid, self.radius, self.floor, have_prior=have, scratch=d["scratch"])
            result = {"joints": out_j, "evidence": evidence, "restarted": restarted != 0}
            if return_beliefs:
                result["beliefs"] = beliefs
            if joints is not None:
                result["shift"] = (out_j - joints.to(device=dev, dtype=torch.float32)).norm(dim=-1)
            self._event = torch.cuda.Event()
            self._event.record(stream)
        self._prior[:] = True
        self.frames_seen += B
        return result


class StoredTrack:
    """What ``VolumeSmoother`` and ``VolumeViterbi`` share: both run a forward pass as the frames are pushed, keep what the backward
    pass needs on the device under a byte budget and release it in ``finish()``.  (``MotionModelFit`` stores under the same budget
    and waits for its pushes the same way; it keeps the frames until ``reset()``.)  A stored push is a NamedTuple of the subclass with
    at least ``restarted`` [B,J], ``given`` (the joints pushed with it, or None) and ``event`` (recorded behind everything the push
    queued).  The subclass says what a push weighs (``bytes_stored``)."""

    _budget_advice = "finish() the track in pieces or raise max_bytes"      # what a subclass without finish() says instead

    def _init_store(self, max_bytes):
        if max_bytes is not None and (isinstance(max_bytes, bool) or not float(max_bytes) >= 0):
            raise ValueError(f"max_bytes = {max_bytes} must be None or a number >= 0")
        self.max_bytes = None if max_bytes is None else int(max_bytes)
        # The forward pass's own event chain orders the steps only: what a push stores is queued behind the event its step recorded,
        # so the next push on another stream is not ordered behind it and finish() waits for the event of every push.
        self._pushes = []
        self._done = None                # recorded behind the last finish(): the next one reuses its workspace

    @property
    def frames_stored(self):
        return sum(int(p.restarted.shape[0]) for p in self._pushes)

    def _admit(self, B, need, dev):
        """The budget gate of a push of ``B`` frames that would store ``need`` bytes: ValueError, with nothing allocated, over it."""
        if self.max_bytes is None:
            self.max_bytes = int(torch.cuda.mem_get_info(dev)[0]) // 2
        if self.bytes_stored + need > self.max_bytes:
            raise ValueError(f"push: {self.frames_stored} frames are stored ({self.bytes_stored} bytes) and {B} more need {need} bytes: "
                             f"over max_bytes = {self.max_bytes}; {self._budget_advice}")

    def _begin_finish(self, stream):
        """The stored pushes, their device, J and the stream finish() runs on (default: the current one), which is made to wait for
        every push, whatever stream each ran on, and for the finish() before this one.  ValueError when nothing is stored."""
        if not self._pushes:
            raise ValueError("finish: nothing is stored; push() the frames of the track first")
        first = self._pushes[0].restarted
        stream = stream if stream is not None else torch.cuda.current_stream(first.device)
        for p in self._pushes:
            stream.wait_event(p.event)
        if self._done is not None:
            stream.wait_event(self._done)
        return self._pushes, first.device, int(first.shape[1]), stream

    @staticmethod
    def _add_shift(result, pushes):
        """``result["shift"]`` [T,J]: metres between ``result["joints"]`` and the joints given with the pushes, NaN for a push without;
        no key when no push had any."""
        if any(p.given is not None for p in pushes):
            joints = result["joints"]
            given = torch.cat([p.given if p.given is not None
                               else torch.full(tuple(p.restarted.shape) + (3,), float("nan"), device=joints.device, dtype=torch.float32)
                               for p in pushes])
            result["shift"] = (joints - given).norm(dim=-1)
