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

import numbers
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
    def sample(self, samples=16, seed=0, stream=None):
        """``samples`` whole trajectories per joint through the T stored frames, drawn jointly from the posterior of the hidden Markov
        model that ``finish()`` gives the marginals of: forward-filter backward-sampling on the stored filtered beliefs
        (``csrc/volume_sample.hip``, ``se_volume_sample_f32``; the header states the definition).  Call it BEFORE ``finish()``: it
        consumes and modifies nothing, and a later ``finish()`` returns the bits it would have returned.  With nothing stored (after
        ``finish()`` or ``reset()``) it raises ValueError.  ``seed`` in 0..2^64-1: the same seed gives the same trajectories, however the
        frames were cut into pushes; sample s of ``samples=n`` is sample s of any larger n.  It runs on ``stream`` (default: the current
        one), which waits for every push.  Returns a dict of device tensors over all T frames: ``index`` [S,T,J] int32 (the flat voxel,
        -1 where the frame's belief has no finite positive mass), ``coord`` [S,T,J,3] (the voxel centres, NaN where invalid), ``kind``
        [S,T,J] int32 (0 a step from the next frame's voxel, 1 a jump, 2 a fresh draw: the last frame, a frame before a restart or
        before an invalid one), ``valid`` [S,T,J] bool, ``mean`` [T,J,3] and ``spread`` [T,J]: the mean of the valid samples and the
        root of the trace of their sample covariance in metres (NaN with fewer than two), and ``shift`` [T,J] when joints were pushed
        (metres from ``mean`` to those).  A sample is a voxel centre: nothing is refined below the voxel edge."""
        if isinstance(samples, bool) or not isinstance(samples, numbers.Integral) or samples < 1:
            raise ValueError(f"sample: samples = {samples!r} (an integer >= 1) expected")
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"sample: seed = {seed!r} (an integer in 0..2^64-1) expected")
        if not self._pushes:
            raise ValueError("sample: nothing is stored; push() the frames of the track first and draw before finish()")
        pushes, dev, J, stream = self._begin_finish(stream)
        f = self.filter
        fd = f._dev
        S = int(samples)
        with torch.cuda.stream(stream):
            T = self.frames_stored
            index = torch.empty((S, T, J), device=dev, dtype=torch.int32)
            kind = torch.empty((S, T, J), device=dev, dtype=torch.int32)
            carried = torch.full((S, J), -1, device=dev, dtype=torch.int32)
            t1 = T
            for i in range(len(pushes) - 1, -1, -1):
                bel, restarted = pushes[i].beliefs, pushes[i].restarted
                for t in (bel, restarted):
                    t.record_stream(stream)
                B = int(bel.shape[0])
                t0 = t1 - B
                link = None if i == len(pushes) - 1 else (pushes[i + 1].restarted[0] == 0).to(torch.int32)
                idx = torch.empty((S, B, J), device=dev, dtype=torch.int32)
                knd = torch.empty((S, B, J), device=dev, dtype=torch.int32)
                _lib.volume_sample(bel, restarted, fd["taps"], carried, idx, knd, B, J, f.voxels, f.grid, f.radius, f.floor, S,
                                   first_sample=0, first_frame=t0, seed=int(seed), have_link=link)
                index[:, t0:t1], kind[:, t0:t1] = idx, knd
                t1 = t0
            # a finish() on another stream writes over the beliefs read here: it waits for this event as for a finish() before it
            self._done = torch.cuda.Event()
            self._done.record(stream)
            valid = index >= 0
            coord = fd["coord"][index.clamp(min=0).long()]
            coord = torch.where(valid.unsqueeze(-1), coord, torch.full_like(coord, float("nan")))
            n = valid.sum(dim=0).to(torch.float32)                                          # [T,J]
            kept = torch.where(valid.unsqueeze(-1), coord, torch.zeros_like(coord))
            mean = kept.sum(dim=0) / n.unsqueeze(-1)                                        # 0 / 0 = NaN without a valid sample
            dev2 = torch.where(valid.unsqueeze(-1), (kept - mean) ** 2, torch.zeros_like(kept)).sum(dim=(0, 3))
            spread = torch.where(n >= 2, (dev2 / (n - 1).clamp(min=1)).sqrt(), torch.full_like(n, float("nan")))
            result = {"index": index, "coord": coord, "kind": kind, "valid": valid, "mean": mean, "spread": spread}
            with_joints = {"joints": mean}
            self._add_shift(with_joints, pushes)
            if "shift" in with_joints:
                result["shift"] = with_joints["shift"]
        return result

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
