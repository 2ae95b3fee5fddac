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

HOW CLOSE WAS THE NEXT ONE.  ``VolumeViterbi(..., alternatives=True)`` also keeps every frame's scores, and ``alternatives()`` runs
the backward max-product pass behind the walk (``se_volume_viterbi_back_f32``: the same stages on ``r = p m`` of the frame behind with
the taps reversed).  It gives the max-marginal of every frame and voxel, the score of the best whole trajectory that is there then,
and from it the margin of every frame of the path, the best trajectory that is somewhere else in that frame, and the runner-up
trajectory of each segment (``se_volume_viterbi_branch_i32`` walks it).  With the default nothing changes.
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
ALTERNATIVE_KEYS = ("complete", "margin", "alt_index", "alt_coord", "alt_log_score", "max_marginal_peak_index", "path_is_peak",
                    "runner_up_index", "runner_up_coord", "runner_up_joints", "runner_up_jumped", "runner_up_anchor", "runner_up_margin")
MAX_REFINE = _lib.VITERBI_MAX_REFINE


class _Push(NamedTuple):
    """One stored push: its back-pointers [B,J,G^3] int32, the copy of its volumes (None with ``refine`` = 0), the forward pass's
    ``peak``, ``best``, ``exponent`` and ``restarted`` [B,J], the joints given with it, the event behind it all and, with
    ``alternatives``, the frames' scores [B,J,G^3] float32 (``alternatives()`` turns them into the successor pointers in place)."""
    back: torch.Tensor
    volumes: Optional[torch.Tensor]
    peak: torch.Tensor
    best: torch.Tensor
    exponent: torch.Tensor
    restarted: torch.Tensor
    given: Optional[torch.Tensor]
    event: torch.cuda.Event
    scores: Optional[torch.Tensor] = None


class VolumeViterbi(StoredTrack):
    """``v = VolumeViterbi(coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3, refine=1, max_bytes=None,
    alternatives=False)``; ``v.push(volumes)`` per batch in frame order, ``v.finish()`` (or ``v.alternatives()``) at the end of the track.  ``sigma``, ``radius`` and ``floor`` are ``VolumeFilter``'s and a
    bad one raises its ValueError here, before anything touches the device.  ``refine``: the half-width in voxels (0..3) of the window
    the path voxel is refined over; 0 keeps the voxel centre and stores no volumes.  ``max_bytes``: the most the stored back-pointers
    and volumes may take (B x J x G^3 x 4 bytes per push each: 31.4 MB per frame at 15 x 64^3 with ``refine`` > 0, 15.7 MB without);
    default: half of the device memory that is free at the first push.  ``alternatives`` = True keeps what ``alternatives()`` needs:
    the volumes (also with ``refine`` = 0) and every frame's scores, 12 bytes per voxel in all (47.2 MB per frame at 15 x 64^3)."""

    def __init__(self, coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3, refine=1, max_bytes=None, alternatives=False):
        self.filter = VolumeFilter(coord, grid, cuboid_side, sigma=sigma, radius=radius, floor=floor)     # the parameters, checked
        if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= int(refine) <= MAX_REFINE:
            raise ValueError(f"refine = {refine!r} (an integer in 0..{MAX_REFINE}) expected")
        self._init_store(max_bytes)
        self.refine = int(refine)
        self.keep_scores = bool(alternatives)
        self.frames_seen = 0
        self.rows = None                 # the joints per frame, fixed by the first push
        self._has_prior = False
        self._event = None               # recorded behind the last forward pass: the next one waits for it, whatever its stream
        self._dev = {}

    # ------------------------------------------------------------------------------------------------------------------------
    @property
    def bytes_stored(self):
        return sum(p.back.numel() * 4 + sum(t.numel() * 4 for t in (p.volumes, p.scores) if t is not None) for p in self._pushes)

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
        self._admit(B, (3 if self.keep_scores else 2 if self.refine > 0 else 1) * B * J * f.voxels * 4, dev)
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
            have_prior = c["ones"] if self._has_prior else None
            scores = None
            if self.keep_scores:
                scores = torch.empty((B, J, f.voxels), device=dev, dtype=torch.float32)
                _lib.volume_viterbi_keep(vol, c["taps"], d["state"], d["peak"], d["best"], back, peak, best, exponent, restarted, scores,
                                         B, J, f.voxels, f.grid, f.radius, f.floor, have_prior=have_prior, scratch=d["scratch"])
            else:
                _lib.volume_viterbi(vol, c["taps"], d["state"], d["peak"], d["best"], back, peak, best, exponent, restarted, B, J,
                                    f.voxels, f.grid, f.radius, f.floor, have_prior=have_prior, scratch=d["scratch"])
            self._event = torch.cuda.Event()
            self._event.record(stream)
            given = None if joints is None else joints.to(device=dev, dtype=torch.float32).clone()
            copy = volumes.clone(memory_format=torch.contiguous_format) if self.refine > 0 or self.keep_scores else None
            event = torch.cuda.Event()
            event.record(stream)
            self._pushes.append(_Push(back, copy, peak, best, exponent, restarted, given, event, scores))
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
        return self._finish(stream, None)

    @torch.no_grad()
    def alternatives(self, separation=2, return_max_marginals=False, stream=None):
        """``finish()`` with the backward max-product pass (``se_volume_viterbi_back_f32``) behind the walk of every chunk: how close
        was the second-best trajectory?  The max-marginal mm_t(x) is the score of the best whole trajectory that is at voxel x in
        frame t.  Needs ``VolumeViterbi(..., alternatives=True)`` (ValueError otherwise).  Consumes the stored frames as ``finish()``
        does and returns everything it returns, with the same bits, and over all T frames:
        ``margin`` [T,J] float64: ln mm_t(x*_t) - ln of the largest mm_t further than ``separation`` voxels (Chebyshev, in voxel
        indices) from the path voxel x*_t, from the float32 values: by how much the best trajectory that is somewhere else in this
        frame loses.  +inf where the window leaves nothing, NaN without a path voxel.
        ``alt_index`` [T,J] int32, ``alt_coord`` [T,J,3]: where that trajectory is in this frame (-1 / NaN for none);
        ``alt_log_score`` [T,J] float64: its score, the segment's ``log_score`` minus the margin.
        ``max_marginal_peak_index`` [T,J] int32 and ``path_is_peak`` [T,J] bool: the best voxel of mm_t; it is the path voxel unless
        two trajectories tie.  ``complete`` [T,J] bool: the backward recursion reached this frame from the segment's end (False
        where it underflowed on the way: the margins of such frames cover the frames up to there only).
        Per segment the RUNNER-UP: the anchor frame is the one with the smallest margin (the lowest frame among equals), its
        trajectory the best one through ``alt_index`` there: ``runner_up_index`` [T,J] int32, ``runner_up_coord``,
        ``runner_up_joints`` [T,J,3] (refined as ``joints``), ``runner_up_jumped`` [T,J] bool, ``runner_up_anchor`` [T,J] bool (True
        at the anchor frame) and ``runner_up_margin`` [T,J] float64 (the anchor's margin, over the whole segment; NaN and -1 for a
        segment without an alternative).  With ``return_max_marginals``, ``max_marginals``: one [B,J,G,G,G] tensor per push, every
        frame and joint divided by its largest value, so ``joint_modes`` and the volume renderer take them.
        Nothing here is calibrated: a margin is a log score ratio under the motion model's conventions, not a probability."""
        if not self.keep_scores:
            raise ValueError("alternatives: the scores of the frames were not kept; construct VolumeViterbi(..., alternatives=True)")
        if isinstance(separation, bool) or not isinstance(separation, (int, np.integer)) or separation < 0:
            raise ValueError(f"alternatives: separation = {separation!r} (an integer >= 0) expected")
        return self._finish(stream, {"separation": int(separation), "max_marginals": bool(return_max_marginals)})

    def _finish(self, stream, alt):
        pushes, dev, J, stream = self._begin_finish(stream)
        f = self.filter
        d, coord_dev = self._dev, f._dev["coord"]
        with torch.cuda.stream(stream):
            T = self.frames_stored
            joints = torch.empty((T, J, 3), device=dev, dtype=torch.float32)
            index = torch.empty((T, J), device=dev, dtype=torch.int32)
            jumped = torch.empty((T, J), device=dev, dtype=torch.int32)
            if alt is not None:
                if "back_scratch" not in d:
                    d["back_scratch"] = torch.empty(_lib.volume_viterbi_back_scratch_bytes(J, f.grid, f.radius), device=dev,
                                                    dtype=torch.uint8)
                    d["carry"] = {"r": torch.empty((J, f.voxels), device=dev, dtype=torch.float32),
                                  "link": torch.full((J,), -1, device=dev, dtype=torch.int32),
                                  "best": torch.full((J,), float("nan"), device=dev, dtype=torch.float32),
                                  "complete": torch.ones((J,), device=dev, dtype=torch.int32)}
                taps = f._device_constants(dev, J)["taps"]
                out = {name: torch.empty((T, J), device=dev, dtype=dtype) for name, dtype in _lib.BACK_OUTPUTS}
                mms = [torch.empty_like(p.volumes) if alt["max_marginals"] else None for p in pushes]
            t1 = T
            for i in range(len(pushes) - 1, -1, -1):
                back, vol, peak, restarted = pushes[i].back, pushes[i].volumes, pushes[i].peak, pushes[i].restarted
                for t in (back, vol, peak, restarted, pushes[i].scores):
                    if t is not None:
                        t.record_stream(stream)
                B = int(back.shape[0])
                t0 = t1 - B
                _lib.volume_viterbi_path(back, peak, restarted, d["cursor"], index[t0:t1], jumped[t0:t1], B, J, f.voxels,
                                         have_next=int(i != len(pushes) - 1))
                _lib.volume_viterbi_refine(vol, coord_dev, index[t0:t1], joints[t0:t1], B, J, f.voxels, f.grid, self.refine)
                if alt is not None:         # the successor pointers take the place of the scores
                    _lib.volume_viterbi_back(vol, pushes[i].scores, pushes[i].exponent, restarted, index[t0:t1], taps, d["carry"],
                                             {name: out[name][t0:t1] for name in out}, B, J, f.voxels, f.grid, f.radius, f.floor,
                                             alt["separation"], int(i != len(pushes) - 1), succ=pushes[i].scores.view(torch.int32),
                                             max_marginals=mms[i], scratch=d["back_scratch"])
                t1 = t0
            restarted = torch.cat([p.restarted for p in pushes]) != 0
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float32)
            on_path = (index >= 0).unsqueeze(-1)
            coord = torch.where(on_path, coord_dev[index.clamp(min=0).long()], nan)
            moved = torch.full((T, J), float("nan"), device=dev, dtype=torch.float32)
            moved[1:] = (coord[1:] - coord[:-1]).norm(dim=-1)
            best = torch.cat([p.best for p in pushes]).cpu().numpy().astype(np.float64)
            exponent = torch.cat([p.exponent for p in pushes]).cpu().numpy().astype(np.float64)
            restarted_host = restarted.cpu().numpy()
            log_score_host = segment_log_scores(best, exponent, restarted_host)
            log_score = torch.from_numpy(log_score_host).to(dev)
            result = {"joints": joints, "index": index, "coord": coord, "jumped": jumped != 0, "segment_start": restarted,
                      "log_score": log_score, "moved": moved}
            self._add_shift(result, pushes)
            if alt is not None:
                self._add_alternatives(result, pushes, out, mms, restarted_host, log_score_host, alt, dev, J)
            self._done = torch.cuda.Event()
            self._done.record(stream)
            self._pushes = []
        return result

    def _add_alternatives(self, result, pushes, out, mms, restarted, log_score, alt, dev, J):
        """The host half of ``alternatives()``: margins and anchors in float64 where ``finish()`` already waits, then the branch walk
        from the anchors (back through the back-pointers, chunks last first; on through the successor pointers, chunks first to
        last) and its refinement."""
        f = self.filter
        d, coord_dev = self._dev, f._dev["coord"]
        index, T = result["index"], int(result["index"].shape[0])
        alt_index = out["alt_index"].cpu().numpy()
        margin = path_margins(out["path_value"].cpu().numpy(), out["alt_value"].cpu().numpy(), alt_index, index.cpu().numpy())
        anchor_host, runner_margin = runner_up_anchors(margin, alt_index, restarted)
        anchor = torch.from_numpy(anchor_host).to(dev)
        ru_index = torch.empty((T, J), device=dev, dtype=torch.int32)
        ru_jumped = torch.empty((T, J), device=dev, dtype=torch.int32)
        ru_joints = torch.empty((T, J, 3), device=dev, dtype=torch.float32)
        starts = np.concatenate([[0], np.cumsum([int(p.back.shape[0]) for p in pushes])]).tolist()
        order = list(range(len(pushes)))
        for direction, chunks in ((-1, order[::-1]), (1, order)):
            for n, i in enumerate(chunks):
                t0, t1 = starts[i], starts[i + 1]
                _lib.volume_viterbi_branch(pushes[i].back, pushes[i].scores.view(torch.int32), pushes[i].restarted, anchor[t0:t1],
                                           d["cursor"], ru_index[t0:t1], ru_jumped[t0:t1], t1 - t0, J, f.voxels, direction, int(n > 0))
        for i in order:
            t0, t1 = starts[i], starts[i + 1]
            _lib.volume_viterbi_refine(pushes[i].volumes, coord_dev, ru_index[t0:t1], ru_joints[t0:t1], t1 - t0, J, f.voxels, f.grid,
                                       self.refine)
        nan = torch.full((), float("nan"), device=dev, dtype=torch.float32)

        def centres(idx):
            return torch.where((idx >= 0).unsqueeze(-1), coord_dev[idx.clamp(min=0).long()], nan)

        result["complete"] = out["complete"] != 0
        result["margin"] = torch.from_numpy(margin).to(dev)
        result["alt_index"] = out["alt_index"]
        result["alt_coord"] = centres(out["alt_index"])
        result["alt_log_score"] = torch.from_numpy(segment_broadcast(log_score, restarted) - margin).to(dev)
        result["max_marginal_peak_index"] = out["mm_peak"]
        result["path_is_peak"] = (out["mm_peak"] == index) & (index >= 0)
        result["runner_up_index"] = ru_index
        result["runner_up_coord"] = centres(ru_index)
        result["runner_up_joints"] = ru_joints
        result["runner_up_jumped"] = ru_jumped != 0
        result["runner_up_anchor"] = anchor >= 0
        result["runner_up_margin"] = torch.from_numpy(runner_margin).to(dev)
        if alt["max_marginals"]:
            t0 = 0
            for i, mm in enumerate(mms):
                B = int(mm.shape[0])
                mm.view(B, J, -1).div_(out["mm_best"][t0:t0 + B].unsqueeze(-1))
                t0 += B
            result["max_marginals"] = mms


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


def segment_broadcast(log_score, restarted):
    """Host: ``log_score`` [T,J] as ``segment_log_scores`` gives it (a value at the last frame of each segment) -> [T,J] with the
    segment's value at every one of its frames."""
    log_score, restarted = np.asarray(log_score, dtype=np.float64), np.asarray(restarted) != 0
    out = log_score.copy()
    for t in range(log_score.shape[0] - 2, -1, -1):
        out[t] = np.where(restarted[t + 1], log_score[t], out[t + 1])
    return out


def path_margins(path_value, alt_value, alt_index, index):
    """Host, float64: ln ``path_value`` - ln ``alt_value`` from the float32 values [T,J] of the backward pass and nothing else; +inf
    where the window leaves nothing (``alt_index`` -1); NaN where the frame has no path voxel or reports no max-marginal."""
    pv, av = np.asarray(path_value).astype(np.float64), np.asarray(alt_value).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.log(pv) - np.log(av)
    margin = np.where(np.asarray(alt_index) < 0, np.inf, margin)
    return np.where((np.asarray(index) < 0) | np.isnan(pv), np.nan, margin)


def runner_up_anchors(margin, alt_index, restarted):
    """Host: per segment of ``restarted`` [T,J] the anchor frame, the one with the smallest finite ``margin`` (the lowest frame among
    equals) -> (``anchor`` [T,J] int32: ``alt_index`` at the anchor frames, -1 elsewhere; ``runner_up_margin`` [T,J] float64: the
    anchor's margin at every frame of its segment, NaN for a segment without an alternative)."""
    margin, alt_index, restarted = np.asarray(margin, dtype=np.float64), np.asarray(alt_index), np.asarray(restarted) != 0
    T, J = margin.shape
    anchor = np.full((T, J), -1, dtype=np.int32)
    broadcast = np.full((T, J), np.nan)
    usable = np.where(np.isfinite(margin) & (alt_index >= 0), margin, np.inf)
    for j in range(J):
        starts = [t for t in range(T) if t == 0 or restarted[t, j]] + [T]
        for a, b in zip(starts[:-1], starts[1:]):
            t = a + int(np.argmin(usable[a:b, j]))          # the first of equal minima
            if np.isfinite(usable[t, j]):
                anchor[t, j] = alt_index[t, j]
                broadcast[a:b, j] = usable[t, j]
    return anchor, broadcast
