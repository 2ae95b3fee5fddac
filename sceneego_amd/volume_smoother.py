"""Forward-backward smoothing of the joint volumes of a recorded sequence, on the device (``csrc/volume_filter.hip``,
``se_volume_smooth_f32``): the backward pass that goes with ``VolumeFilter``.

The filter's belief at frame t knows frames 0..t, so it can do nothing about an ambiguity in the first frames of a track or right
after a restart.  On a recorded sequence the future is there: ``VolumeSmoother`` runs the filter as the frames are pushed, keeps the
volumes ``p_t`` and the filtered beliefs ``b_t`` on the device, and ``finish()`` walks them from last to first with a backward belief
``r`` (the same filter run backwards in time),

    u = (1 - floor) blur3T(r_{t+1}) + floor / N       blur3T: blur3 with the taps reversed (the same for the symmetric taps used here)
    g = b_t u,  S = sum g,  gamma_t = g / S           the smoothed belief: gamma_t ~ (prediction from the past) p_t (prediction from the future)
    a = p_t u,  s = sum a,  r_t = a / s

Frame t is linked to t + 1 unless it is the last of the track or the filter restarted at t + 1: a forward restart cuts the chain in
both directions.  An unlinked frame, or one whose S is not a finite number > 0, keeps ``gamma_t = b_t`` bit for bit (``smoothed``
false); the last frame's gamma is always its filtered belief.  These are the forward-backward marginals of the hidden Markov model
whose transition is ``(1 - floor) blur3 + floor / N``.

It adds no convention to the filter's: the motion model, the floor and the restart rule are the filter's own, and none is calibrated.
Its limit follows from the model: a false lobe that is stronger than the true one for several frames in a row stays the likelier
explanation under any ``floor > 0``, because one jump is then cheaper than the weaker lobe (README: the measured example).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from .volume_filter import StoredTrack, VolumeFilter


class _Push(NamedTuple):
    """One stored push: the copies of its volumes and filtered beliefs [B,J,G^3 as G,G,G], the filter's restart flags (int32) and
    joints, the joints given with it and the event behind the copies."""
    volumes: torch.Tensor
    beliefs: torch.Tensor
    restarted: torch.Tensor
    given: Optional[torch.Tensor]
    filtered: torch.Tensor
    event: torch.cuda.Event


class VolumeSmoother(StoredTrack):
    """``s = VolumeSmoother(coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3, max_bytes=None)``; ``s.push(volumes)`` per
    batch in frame order, ``s.finish()`` at the end of the track.  The parameters are ``VolumeFilter``'s and a bad one raises its
    ValueError here, before anything touches the device.  ``max_bytes``: the most the stored volumes and beliefs may take (2 x B x J x
    G^3 x 4 bytes per push: 31.4 MB per frame at 15 x 64^3); default: half of the device memory that is free at the first push."""

    def __init__(self, coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3, max_bytes=None):
        self.filter = VolumeFilter(coord, grid, cuboid_side, sigma=sigma, radius=radius, floor=floor)
        self._init_store(max_bytes)
        self._dev = {}

    # ------------------------------------------------------------------------------------------------------------------------
    @property
    def bytes_stored(self):
        return sum(2 * p.volumes.numel() * 4 for p in self._pushes)

    def reset(self):
        """Forget everything: the stored frames and the filter's prior.  Nothing is queued on the device."""
        self._pushes = []
        self.filter.reset()

    @torch.no_grad()
    def push(self, volumes, joints=None, stream=None):
        """The next B consecutive frames ``volumes`` [B,J,G,G,G] of the track: runs ``VolumeFilter.step(volumes, joints,
        return_beliefs=True, stream=stream)`` and returns exactly its dict, so the live filtered result loses nothing.  The volumes
        and the beliefs are copied into storage of the smoother's own (``forward()``'s volumes are static buffers under graphs and the
        pipeline).  Raises ValueError, with nothing allocated, once the stored bytes plus this push would exceed ``max_bytes``."""
        f = self.filter
        B, J = f._check_step(volumes, joints)
        _lib.require_hip(volumes, joints)
        self._admit(B, 2 * B * J * f.voxels * 4, volumes.device)
        stream = stream if stream is not None else torch.cuda.current_stream(volumes.device)
        result = f.step(volumes, joints=joints, return_beliefs=True, stream=stream)
        with torch.cuda.stream(stream):
            given = None if joints is None else joints.to(device=volumes.device, dtype=torch.float32).clone()
            copies = (volumes.clone(memory_format=torch.contiguous_format), result["beliefs"].clone(),
                      result["restarted"].to(torch.int32), given, result["joints"].clone())
            event = torch.cuda.Event()
            event.record(stream)
            self._pushes.append(_Push(*copies, event))
        return result

    def _workspace(self, dev, J):
        f = self.filter
        key = (str(dev), J)
        if self._dev.get("key") != key:
            self._dev = {"key": key,
                         "state": torch.empty((J, f.voxels), device=dev, dtype=torch.float32),
                         "scratch": torch.empty(_lib.volume_smooth_scratch_bytes(J, f.grid, f.radius), device=dev, dtype=torch.uint8)}
        return self._dev

    @torch.no_grad()
    def finish(self, return_beliefs=False, stream=None):
        """Smooth the T stored frames, last to first, on ``stream`` (default: the current one; it waits for every push, whatever stream
        each ran on, and for the finish() before it, whose workspace it reuses).  Returns
        a dict of device tensors over all T frames: ``joints`` [T,J,3] (the expectation of each smoothed belief; where ``smoothed`` is
        false the filter's own joint, bit for bit), ``smoothed`` [T,J] bool, ``agreement`` [T,J] (S: how well the future's prediction
        agrees with the filtered belief, 1 / G^3 is chance; NaN where the frame is not linked to the next), ``filtered_joints``
        [T,J,3], ``shift_filtered`` [T,J] (metres between the smoothed and the filtered joints), ``shift`` [T,J] when joints were
        pushed (metres from those; NaN for a push without) and, with ``return_beliefs``, ``beliefs``: a list with one [B_i,J,G,G,G]
        tensor per push, written in place over the stored filtered beliefs.  Without ``return_beliefs`` nothing of that size is
        written.  The storage is released once every launch is queued (an argument error leaves the stored track as it was); the
        filter keeps its state, so frames pushed afterwards continue the track for the filter but are smoothed as a piece of their
        own."""
        pushes, dev, J, stream = self._begin_finish(stream)
        f = self.filter
        fd = f._dev
        with torch.cuda.stream(stream):
            ws = self._workspace(dev, J)
            T = self.frames_stored
            joints = torch.empty((T, J, 3), device=dev, dtype=torch.float32)
            agreement = torch.empty((T, J), device=dev, dtype=torch.float32)
            smoothed = torch.empty((T, J), device=dev, dtype=torch.int32)
            t1 = T
            for i in range(len(pushes) - 1, -1, -1):
                vol, bel, restarted = pushes[i].volumes, pushes[i].beliefs, pushes[i].restarted
                for t in (vol, bel, restarted):
                    t.record_stream(stream)
                B = int(vol.shape[0])
                t0 = t1 - B
                link = None if i == len(pushes) - 1 else (pushes[i + 1].restarted[0] == 0).to(torch.int32)
                _lib.volume_smooth(vol, bel, restarted, fd["coord"], fd["taps"], ws["state"], bel if return_beliefs else None,
                                   joints[t0:t1], agreement[t0:t1], smoothed[t0:t1], B, J, f.voxels, f.grid, f.radius, f.floor,
                                   have_link=link, scratch=ws["scratch"])
                t1 = t0
            self._done = torch.cuda.Event()
            self._done.record(stream)
            self._pushes = []
            filtered = torch.cat([p.filtered for p in pushes])
            # where gamma_t is the copy of b_t the joint is the filter's own, bit for bit: the kernel's sum b c there is the same
            # expectation summed in another order ((sum a c) / Z in the filter)
            joints = torch.where((smoothed != 0).unsqueeze(-1), joints, filtered)
            result = {"joints": joints, "smoothed": smoothed != 0, "agreement": agreement, "filtered_joints": filtered,
                      "shift_filtered": (joints - filtered).norm(dim=-1)}
            self._add_shift(result, pushes)
            if return_beliefs:
                result["beliefs"] = [p.beliefs for p in pushes]
        return result
