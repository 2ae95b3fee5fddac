"""The most probable trajectory of every joint through the joint volumes of a recorded sequence, on the device
(``csrc/volume_viterbi.hip``, ``se_volume_viterbi_f32``): the max-product pass that goes with ``VolumeFilter`` and ``VolumeSmoother``.

The filter and the smoother answer one question: per frame, the marginal of each joint.  Their joints are expectations of those
marginals, and between two lobes of equal weight an expectation is a point that carries no probability.  ``VolumeViterbi`` answers
the other question a hidden Markov model is asked: which single trajectory is the most probable?  Per joint and frame, with ``s``
the scaled scores of the frame before,

    e3   = the maximum over the step d of s(x + d) w(d), taken along k, then j, then i with the filter's taps, with its argmax y(x)
    m    = max((1 - floor) e3, (floor / N) max s)       the step, or a jump from the best voxel of the frame before
    a    = p m,  M = max a,  s' = a 2^-e with e = ilogb(M)      an exact rescaling: no division, no drift over long sequences

and a back-pointer per voxel (y(x), or the best voxel of the frame before with the jump bit).  A row without a prior, or whose M is not
a finite number > 0, restarts with ``a = p`` and back-pointers of -1: a segment start.  ``finish()`` walks the back-pointers from the
last frame's best voxel to the first frame and refines each path voxel to the centroid of ``p`` over a small window around it.

MODEL NOTE.  This is the Viterbi recursion of the model whose transition score is ``max((1 - floor) W(d), floor / N)``, ``W`` the
separable product of the taps.  It is within a factor of 2 of the filter's ``(1 - floor) W + floor / N``, and unlike that sum it is
separable under the maximum.  No other convention is added to the filter's: motion model, floor and restart rule are its own, and
none is calibrated.  Its limit follows from what it is: the path is all-or-nothing where the marginals hedge.  A false lobe that is
slightly stronger than the true one throughout is followed in every frame (README: the measured example).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .volume_filter import StoredTrack, VolumeFilter

PATH_KEYS = ("joints", "index", "coord", "jumped", "segment_start", "log_score", "moved")
PUSH_KEYS = ("peak_index", "best", "exponent", "restarted")
MAX_REFINE = _lib.VITERBI_MAX_REFINE


class _Push(NamedTuple):
    """One stored push: its back-pointers [B,J,G^3] int32, the copy of its volumes (None with ``refine`` = 0), the forward pass's
    ``peak``, ``best``, ``exponent`` and ``restarted`` [B,J], the joints given with it and the event behind it all."""
    back: torch.Tensor
    volumes: Optional[torch.Tensor]
    peak: torch.Tensor
    best: torch.Tensor
    exponent: torch.Tensor
    restarted: torch.Tensor
    given: Optional[torch.Tensor]
    event: torch.cuda.Event


class VolumeViterbi(StoredTrack):
    """``v = VolumeViterbi(coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3, refine=1, max_bytes=None)``; ``v.push(volumes)``
    per batch in frame order, ``v.finish()`` at the end of the track.  ``sigma``, ``radius`` and ``floor`` are ``VolumeFilter``'s and a
    bad one raises its ValueError here, before anything touches the device.  ``refine``: the half-width in voxels (0..3) of the window
    the path voxel is refined over; 0 keeps the voxel centre and stores no volumes.  ``max_bytes``: the most the stored back-pointers
    and volumes may take (B x J x G^3 x 4 bytes per push each: 31.4 MB per frame at 15 x 64^3 with ``refine`` > 0, 15.7 MB without);
    default: half of the device memory that is free at the first push."""

    def __init__(self, coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3, refine=1, max_bytes=None):
        self.filter = VolumeFilter(coord, grid, cuboid_side, sigma=sigma, radius=radius, floor=floor)     # the parameters, checked
        if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= int(refine) <= MAX_REFINE:
            raise ValueError(f"refine = {refine!r} (an integer in 0..{MAX_REFINE}) expected")
        self._init_store(max_bytes)
        self.refine = int(refine)
        self.frames_seen = 0
        self.rows = None                 # the joints per frame, fixed by the first push
        self._has_prior = False
        self._event = None               # recorded behind the last forward pass: the next one waits for it, whatever its stream
        self._dev = {}

    # ------------------------------------------------------------------------------------------------------------------------
    @property
    def bytes_stored(self):
        return sum(p.back.numel() * 4 + (0 if p.volumes is None else p.volumes.numel() * 4) for p in self._pushes)

    @property
    def state(self):
        """The scaled scores after the last push, [J,G,G,G] on the device (None before the first): the object's own buffer."""
        s = self._dev.get("state")
        g = self.filter.grid
        return None if s is None else s.view(-1, g, g, g)

    def reset(self):
        """Forget everything: the stored frames and the prior.  Nothing is queued on the device."""
        self._pushes = []
        self._has_prior = False
        self.frames_seen = 0

    def _device_state(self, dev, J):
        """The recursion's own state on ``dev``; ``coord``, ``taps`` and the row of ones are the filter's (``_device_constants``)."""
        f = self.filter
        key = str(dev)
        if self._dev.get("key") != key:
            if self._dev and self._has_prior:
                raise ValueError(f"push: the state is on {self._dev['key']}, the volumes on {key}")
            self._dev = {
                "key": key,
                "state": torch.empty((J, f.voxels), device=dev, dtype=torch.float32),
                "peak": torch.full((J,), -1, device=dev, dtype=torch.int32),
                "best": torch.full((J,), float("nan"), device=dev, dtype=torch.float32),
                "cursor": torch.full((J,), -1, device=dev, dtype=torch.int32),
                "scratch": torch.empty(_lib.volume_viterbi_scratch_bytes(J, f.grid, f.radius), device=dev, dtype=torch.uint8),
            }
        return self._dev

    @torch.no_grad()
    def push(self, volumes, joints=None, stream=None):
        """The next B consecutive frames ``volumes`` [B,J,G,G,G] (softmaxed, as ``forward()`` returns them) of the track: runs the
        forward pass over them and stores their back-pointers and, with ``refine`` > 0, a copy of the volumes (``forward()``'s are
        static buffers under graphs and the pipeline).  Returns a dict of device tensors over the B frames: ``peak_index`` [B,J] (the
        best voxel of each frame's scores, -1 where the frame has none), ``best`` [B,J] (the scaled maximum, in [1, 2)), ``exponent``
        [B,J] (its power of two) and ``restarted`` [B,J] bool.  ``joints`` [B,J,3]: kept for ``finish()``'s ``shift``.  ``stream``: as
        for ``VolumeFilter.step``.  Raises ValueError, with nothing allocated, once the stored bytes plus this push would exceed
        ``max_bytes``."""
        f = self.filter
        B, J = f._check_step(volumes, joints)
        if self.rows is not None and J != self.rows:
            raise ValueError(f"push: {J} joints per frame, the state holds {self.rows}")
        _lib.require_hip(volumes, joints)
        dev = volumes.device
        self._admit(B, (2 if self.refine > 0 else 1) * B * J * f.voxels * 4, dev)
        self.rows = J
        stream = stream if stream is not None else torch.cuda.current_stream(dev)
        if self._event is not None:
            stream.wait_event(self._event)
        with torch.cuda.stream(stream):
            d = self._device_state(dev, J)
            c = f._device_constants(dev, J)
            vol = volumes.contiguous()
            back = torch.empty((B, J, f.voxels), device=dev, dtype=torch.int32)
            peak = torch.empty((B, J), device=dev, dtype=torch.int32)
            best = torch.empty((B, J), device=dev, dtype=torch.float32)
            exponent = torch.empty((B, J), device=dev, dtype=torch.int32)
            restarted = torch.empty((B, J), device=dev, dtype=torch.int32)
            _lib.volume_viterbi(vol, c["taps"], d["state"], d["peak"], d["best"], back, peak, best, exponent, restarted, B, J, f.voxels,
                                f.grid, f.radius, f.floor, have_prior=c["ones"] if self._has_prior else None, scratch=d["scratch"])
            self._event = torch.cuda.Event()
            self._event.record(stream)
            given = None if joints is None else joints.to(device=dev, dtype=torch.float32).clone()
            copy = volumes.clone(memory_format=torch.contiguous_format) if self.refine > 0 else None
            event = torch.cuda.Event()
            event.record(stream)
            self._pushes.append(_Push(back, copy, peak, best, exponent, restarted, given, event))
        self._has_prior = True
        self.frames_seen += B
        return {"peak_index": peak, "best": best, "exponent": exponent, "restarted": restarted != 0}

    @torch.no_grad()
    def finish(self, stream=None):
        """Walk the T stored frames back from the last frame's best voxel, on ``stream`` (default: the current one; it waits for every
        push, whatever stream each ran on, and for the finish() before it).  Returns a dict of device tensors over all T frames:
        ``joints`` [T,J,3] (the path voxel refined to the centroid of the frame's volume over the window of ``refine`` voxels around
        it; the voxel centre with ``refine`` = 0 or where the window holds no finite positive mass; NaN where the frame has no path
        voxel), ``index`` [T,J] int32 (the path's flat voxel index, -1 for none), ``coord`` [T,J,3] (the voxel centres), ``jumped``
        [T,J] bool (the path reached this frame's voxel by a jump, not a step), ``segment_start`` [T,J] bool (the frame restarted: the
        path before it is a trajectory of its own), ``log_score`` [T,J] float64 (at the last frame of each segment the natural
        logarithm of the segment's path score, ln best + ln 2 x the sum of the segment's exponents, computed in float64 on the host;
        NaN elsewhere), ``moved`` [T,J] (metres from the previous frame's path voxel; NaN for the first frame) and ``shift`` [T,J]
        when joints were pushed (metres from those; NaN for a push without).  The host waits for ``stream`` (the log scores are
        summed there).  The storage is released; the scores keep their state, so frames pushed afterwards continue the recursion but
        are walked as a piece of their own."""
        pushes, dev, J, stream = self._begin_finish(stream)
        f = self.filter
        d, coord_dev = self._dev, f._dev["coord"]
        with torch.cuda.stream(stream):
            T = self.frames_stored
            joints = torch.empty((T, J, 3), device=dev, dtype=torch.float32)
            index = torch.empty((T, J), device=dev, dtype=torch.int32)
            jumped = torch.empty((T, J), device=dev, dtype=torch.int32)
            t1 = T
            for i in range(len(pushes) - 1, -1, -1):
                back, vol, peak, restarted = pushes[i].back, pushes[i].volumes, pushes[i].peak, pushes[i].restarted
                for t in (back, vol, peak, restarted):
                    if t is not None:
                        t.record_stream(stream)
                B = int(back.shape[0])
                t0 = t1 - B
                _lib.volume_viterbi_path(back, peak, restarted, d["cursor"], index[t0:t1], jumped[t0:t1], B, J, f.voxels,
                                         have_next=int(i != len(pushes) - 1))
                _lib.volume_viterbi_refine(vol, coord_dev, index[t0:t1], joints[t0:t1], B, J, f.voxels, f.grid, self.refine)
                t1 = t0
            self._done = torch.cuda.Event()
            self._done.record(stream)
            self._pushes = []
            restarted = torch.cat([p.restarted for p in pushes]) != 0
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float32)
            on_path = (index >= 0).unsqueeze(-1)
            coord = torch.where(on_path, coord_dev[index.clamp(min=0).long()], nan)
            moved = torch.full((T, J), float("nan"), device=dev, dtype=torch.float32)
            moved[1:] = (coord[1:] - coord[:-1]).norm(dim=-1)
            best = torch.cat([p.best for p in pushes]).cpu().numpy().astype(np.float64)
            exponent = torch.cat([p.exponent for p in pushes]).cpu().numpy().astype(np.float64)
            log_score = torch.from_numpy(segment_log_scores(best, exponent, restarted.cpu().numpy())).to(dev)
            result = {"joints": joints, "index": index, "coord": coord, "jumped": jumped != 0, "segment_start": restarted,
                      "log_score": log_score, "moved": moved}
            self._add_shift(result, pushes)
        return result


def segment_log_scores(best, exponent, restarted):
    """Host, float64: ``best``, ``exponent`` [T,J] and ``restarted`` [T,J] bool of a track -> [T,J]: at the last frame of each
    segment (the frame before a restart, or the last one) ln best + ln 2 x the sum of the exponents since the segment's start; NaN
    elsewhere and where the frame has no best score."""
    best, exponent, restarted = np.asarray(best, dtype=np.float64), np.asarray(exponent, dtype=np.float64), np.asarray(restarted) != 0
    T = best.shape[0]
    out = np.full(best.shape, np.nan)
    acc = np.zeros(best.shape[1:])
    for t in range(T):
        acc = np.where(restarted[t], 0.0, acc) + exponent[t]
        last = np.ones(best.shape[1:], dtype=bool) if t == T - 1 else restarted[t + 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[t] = np.where(last, np.log(best[t]) + math.log(2.0) * acc, np.nan)
    return out
