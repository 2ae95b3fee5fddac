"""Fit the motion model of the sequence operators to a sequence: Baum-Welch (EM) for ``sigma`` and ``floor``, the E-step on the device
(``csrc/volume_filter.hip``, ``se_volume_transition_stats_f32``), the M-step on the host in float64.

``VolumeFilter``, ``VolumeSmoother``, ``VolumeViterbi`` and ``track.select_modes`` run on one motion model: a truncated Gaussian step of
``sigma`` metres per frame plus a uniform ``floor`` for jumps.  The transition ``(1 - floor) W_sigma + floor / N`` is a two-component
mixture whose Gaussian part is an exponential family in ``|d|^2``, so the model can be fitted to the volumes of a sequence without
annotated data, and the M-step is closed:

    E-step   per linked pair of frames (t, t + 1) and joint, from the filter's belief b_t and the backward belief r_{t+1}:
                 step = keep A0 / S      jump = uniform Bsum Rsum / S      sq = keep A2 / S      (step + jump = 1)
             the posterior mass of a Gaussian step, of a jump, and the posterior expected squared step (voxels^2) over the step part;
             S, A0, A2, Bsum, Rsum are the six sums the kernel returns (include/sceneego_hip.h states them).
    M-step   floor' = sum jump / (sum step + sum jump), clamped to ``floor_bounds``
             sigma' = the root of 3 M(sigma) = sum sq / sum step, M(sigma) = sum_d d^2 w_sigma[d] the second moment of the normalised
             truncated taps at the FIXED radius R (bisection; M rises from 0 towards R (R + 1) / 3, where sigma is capped at 10 R h
             and ``saturated`` is set).

The radius does not change during a fit: with it the family is fixed, so EM cannot lower the likelihood ``sum_t ln Z_t`` (Z_t: the
filter's evidence), and the clamp and the cap are constrained maxima of a unimodal Q, which keep that property.  It holds while the set
of terms is the same: a ``Z`` restart that appears or disappears between two iterations changes which frames the sum runs over.
``truncation_binding`` (3 sigma' / h > R) says that the fitted step is cut by the radius: refit with a larger one.

Read the result for what it is: a maximum-likelihood fit to the network's own volumes read as likelihoods, on one sequence.  It says
which ``(sigma, floor)`` explains those volumes best under this model; it is not a validation against ground truth.  The kernels
take one tap vector for all rows: the per-joint values are a diagnostic, not a model the operators can run.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .volume_filter import StoredTrack, VolumeFilter, gaussian_taps

FIT_KEYS = ("sigma", "floor", "radius", "log_likelihood", "history", "mean_sq_step", "pairs", "converged", "saturated",
            "truncation_binding", "sigma_per_joint", "floor_per_joint")
SIGMA_CAP = 10.0           # sigma is capped at SIGMA_CAP * R * h where the moment equation has no root


# ---------------------------------------------------------------------------------------------------------------------------- M-step
def transition_moment(sigma, radius, h):
    """M(sigma) = sum_d d^2 w[d], d = -radius..radius in voxels, with w[d] = exp(-(d h)^2 / (2 sigma^2)) normalised to sum 1 in
    float64: the second moment of one axis of the truncated step.  0 for ``sigma == 0`` or ``radius == 0``; it rises with sigma
    towards radius (radius + 1) / 3, the moment of uniform taps."""
    sigma, radius, h = float(sigma), int(radius), float(h)
    if not sigma >= 0.0 or radius < 0 or not h > 0.0:
        raise ValueError(f"transition_moment: sigma = {sigma} (>= 0), radius = {radius} (>= 0), h = {h} (> 0) expected")
    if sigma == 0.0 or radius == 0:
        return 0.0
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-(d * h) ** 2 / (2.0 * sigma * sigma))
    return float((d * d * w).sum() / w.sum())


def solve_sigma(m2, radius, h):
    """``(sigma, saturated)``: the sigma (metres) at which 3 M(sigma) = ``m2``, the mean squared step in voxels^2 over the three
    axes, at the fixed ``radius``; bisection in float64.  ``m2 <= 0`` or ``radius == 0`` gives 0.  Where ``m2`` reaches what the
    radius can hold (m2 >= radius (radius + 1), or the root lies beyond the cap) sigma is 10 radius h and ``saturated`` is True."""
    m2, radius, h = float(m2), int(radius), float(h)
    if math.isnan(m2) or radius < 0 or not h > 0.0:
        raise ValueError(f"solve_sigma: m2 = {m2} (a number), radius = {radius} (>= 0), h = {h} (> 0) expected")
    if m2 <= 0.0 or radius == 0:
        return 0.0, False
    cap = SIGMA_CAP * radius * h
    if m2 >= radius * (radius + 1) or 3.0 * transition_moment(cap, radius, h) <= m2:
        return cap, True
    lo, hi = 0.0, cap                      # 3 M(lo) < m2 <= 3 M(hi) throughout
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if 3.0 * transition_moment(mid, radius, h) < m2:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi), False


def _pool(step, jump, sq, floor, radius, h, floor_bounds):
    """The M-step over the pairs given: (floor', sigma', saturated, m2 in voxels^2); the current floor and NaN where nothing can be
    said (no pair, no step mass)."""
    s_step, s_jump, s_sq = float(step.sum()), float(jump.sum()), float(sq.sum())
    new_floor = floor
    if s_step + s_jump > 0.0:
        new_floor = min(max(s_jump / (s_step + s_jump), floor_bounds[0]), floor_bounds[1])
    if not s_step > 0.0:
        return new_floor, float("nan"), False, float("nan")
    m2 = s_sq / s_step
    sigma, saturated = solve_sigma(m2, radius, h)
    return new_floor, sigma, saturated, m2


def m_step(stats, linked, floor, G, radius, h, floor_bounds=(1e-6, 0.5)):
    """The E-step's pooling and the M-step, in float64, from what ``se_volume_transition_stats_f32`` wrote: ``stats`` [T, rows, 6]
    (S, s, A0, A2, Bsum, Rsum) and ``linked`` [T, rows], under the ``floor`` the pass ran with (rounded to float32 as the kernel is
    given it).  Every pair with ``linked`` set and a finite S > 0 counts, pooled over rows and frames.  Returns a dict: ``floor`` and
    ``sigma`` (the new values; sigma NaN where no step mass is left to fit it to), ``saturated``, ``truncation_binding``,
    ``mean_sq_step`` (metres^2, over the step component), ``pairs``, ``step`` / ``jump`` / ``sq`` [T, rows] (NaN where the pair does
    not count; sq in voxels^2) and, as a diagnostic only (the kernels take one tap vector for all rows), the same M-step per row:
    ``sigma_per_joint`` and ``floor_per_joint`` [rows]."""
    stats = np.asarray(stats, dtype=np.float64)
    linked = np.asarray(linked) != 0
    G, radius, h = int(G), int(radius), float(h)
    lo, hi = float(floor_bounds[0]), float(floor_bounds[1])
    if stats.ndim != 3 or stats.shape[2] != _lib.STATS_SLOTS or linked.shape != stats.shape[:2]:
        raise ValueError(f"m_step: stats {stats.shape} ([T, rows, {_lib.STATS_SLOTS}]) and linked {linked.shape} ([T, rows]) expected")
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError(f"m_step: floor_bounds = {floor_bounds}: 0 <= low <= high <= 1 expected")
    eps = float(np.float32(floor))
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"m_step: floor = {floor} must lie in [0, 1]")
    keep, uniform = 1.0 - eps, eps / float(G) ** 3
    S, A0, A2, Bsum, Rsum = stats[..., 0], stats[..., 2], stats[..., 3], stats[..., 4], stats[..., 5]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = linked & np.isfinite(S) & (S > 0)
        step = np.where(ok, keep * A0 / S, np.nan)
        jump = np.where(ok, uniform * Bsum * Rsum / S, np.nan)
        sq = np.where(ok, keep * A2 / S, np.nan)
    ok &= np.isfinite(step) & np.isfinite(jump) & np.isfinite(sq)
    new_floor, sigma, saturated, m2 = _pool(step[ok], jump[ok], sq[ok], eps, radius, h, (lo, hi))
    rows = stats.shape[1]
    per_sigma, per_floor = np.full(rows, np.nan), np.full(rows, np.nan)
    for r in range(rows):
        o = ok[:, r]
        if o.any():
            per_floor[r], per_sigma[r], _, _ = _pool(step[o, r], jump[o, r], sq[o, r], eps, radius, h, (lo, hi))
    return {"floor": new_floor, "sigma": sigma, "saturated": bool(saturated),
            "truncation_binding": bool(sigma == sigma and 3.0 * sigma / h > radius),
            "mean_sq_step": m2 * h * h, "pairs": int(ok.sum()), "step": np.where(ok, step, np.nan), "jump": np.where(ok, jump, np.nan),
            "sq": np.where(ok, sq, np.nan), "sigma_per_joint": per_sigma, "floor_per_joint": per_floor}


def log_likelihood(evidence, restarted):
    """``(sum ln Z, terms)``: the filter's evidence over the frames and rows that did not restart, summed in float64."""
    z = np.asarray(evidence, dtype=np.float64)[np.asarray(restarted) == 0]
    return float(np.log(z).sum()), int(z.size)


def check_fit_args(iterations, tol, floor_bounds):
    """fit()'s own arguments, as (iterations, tol, (low, high)); ValueError before anything touches a device."""
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 1:
        raise ValueError(f"fit: iterations = {iterations} must be an integer >= 1")
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError(f"fit: tol = {tol} must be a number >= 0")
    try:
        lo, hi = (float(x) for x in floor_bounds)
    except (TypeError, ValueError):
        raise ValueError(f"fit: floor_bounds = {floor_bounds!r} must be a pair (low, high)") from None
    if not 0.0 <= lo <= hi <= 1.0:
        raise ValueError(f"fit: floor_bounds = {floor_bounds}: 0 <= low <= high <= 1 expected")
    return int(iterations), tol, (lo, hi)


def em_loop(e_step, sigma, floor, G, radius, h, iterations, tol, fit_sigma, fit_floor, floor_bounds):
    """The EM loop around ``e_step(sigma, floor, want_stats) -> (evidence, restarted, stats, linked)`` (stats and linked None without
    ``want_stats``): per iteration the likelihood under the current parameters, the stop test (a relative change below ``tol``), the
    statistics and the M-step.  ``MotionModelFit.fit`` runs it over the device passes and tests/motion_fit_model.py over the float64
    model, so both take the same decisions.  Returns the dict of ``fit``."""
    ll, history, last, converged = [], [], None, False
    for it in range(iterations + 1):
        final = it == iterations
        evidence, restarted, stats, linked = e_step(sigma, floor, not final)
        value, terms = log_likelihood(evidence, restarted)
        ll.append(value)
        history.append({"sigma": sigma, "floor": floor, "log_likelihood": value, "terms": terms})
        # it has stopped moving: a change, up or down, below tol.  A float32 likelihood can fall by rounding alone (1.4e-6 of 212 at
        # 15 x 64^3); that is convergence when it is below tol, and with tol = 0 nothing stops the loop before `iterations`
        converged = it > 0 and abs(value - ll[-2]) < tol * abs(ll[-2])
        if final or converged:
            break
        last = m_step(stats, linked, floor, G, radius, h, floor_bounds)
        if last["pairs"] == 0:
            break
        if fit_floor:
            floor = last["floor"]
        if fit_sigma and last["sigma"] == last["sigma"]:
            sigma = last["sigma"]
    rows_nan = np.full(0, np.nan)
    used_sigma = last is not None and fit_sigma and last["sigma"] == last["sigma"]
    return {"sigma": sigma, "floor": floor, "radius": radius, "log_likelihood": ll, "history": history,
            "mean_sq_step": float("nan") if last is None else last["mean_sq_step"], "pairs": 0 if last is None else last["pairs"],
            "converged": converged, "saturated": bool(used_sigma and last["saturated"]),
            "truncation_binding": bool(3.0 * sigma / h > radius),
            "sigma_per_joint": rows_nan if last is None else last["sigma_per_joint"],
            "floor_per_joint": rows_nan if last is None else last["floor_per_joint"]}


# ---------------------------------------------------------------------------------------------------------------------------- device
class _Push(NamedTuple):
    """One stored push: the copy of its volumes [B,J,G,G,G], the belief buffer of the same size and the restart flags [B,J] int32
    that every iteration's forward pass writes again, and the event behind the copy.  ``given``: what ``StoredTrack`` expects."""
    volumes: torch.Tensor
    beliefs: torch.Tensor
    restarted: torch.Tensor
    given: None
    event: torch.cuda.Event


class MotionModelFit(StoredTrack):
    """``m = MotionModelFit(coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3, max_bytes=None)``; ``m.push(volumes)`` per
    batch in frame order, ``m.fit()`` for the fitted ``sigma`` and ``floor``.  The parameters are ``VolumeFilter``'s, here the values
    the fit starts from, and a bad one raises its ValueError before anything touches the device; the radius stays fixed.
    ``max_bytes``: the most the stored volumes and the belief buffers may take (2 x B x J x G^3 x 4 bytes per push: 31.4 MB per frame
    at 15 x 64^3); default: half of the device memory that is free at the first push."""

    _budget_advice = "fit fewer frames or raise max_bytes"

    def __init__(self, coord, grid, cuboid_side, sigma=0.10, radius=None, floor=1e-3, max_bytes=None):
        self.filter = VolumeFilter(coord, grid, cuboid_side, sigma=sigma, radius=radius, floor=floor)    # the checks and the constants
        self._init_store(max_bytes)
        self._dev = {}

    @property
    def bytes_stored(self):
        return sum(2 * p.volumes.numel() * 4 for p in self._pushes)

    def reset(self):
        """Forget everything: the stored frames.  Nothing is queued on the device."""
        self._pushes = []

    @torch.no_grad()
    def push(self, volumes, stream=None):
        """The next B consecutive frames ``volumes`` [B,J,G,G,G] of the sequence: a copy is stored and a belief buffer of the same size
        reserved beside it (``forward()``'s volumes are static buffers under graphs and the pipeline).  Nothing is computed.  Raises
        ValueError, with nothing allocated, once the stored bytes plus this push would exceed ``max_bytes``."""
        f = self.filter
        B, J = f._check_step(volumes, None)
        if self._pushes and int(self._pushes[0].restarted.shape[1]) != J:
            raise ValueError(f"push: {J} joints per frame, the stored frames hold {int(self._pushes[0].restarted.shape[1])}")
        _lib.require_hip(volumes)
        self._admit(B, 2 * B * J * f.voxels * 4, volumes.device)
        stream = stream if stream is not None else torch.cuda.current_stream(volumes.device)
        with torch.cuda.stream(stream):
            vol = volumes.clone(memory_format=torch.contiguous_format)
            beliefs = torch.empty_like(vol)
            restarted = torch.zeros((B, J), device=volumes.device, dtype=torch.int32)
            event = torch.cuda.Event()
            event.record(stream)
            self._pushes.append(_Push(vol, beliefs, restarted, None, event))

    def _workspace(self, dev, J, T):
        f = self.filter
        key = (str(dev), J, T)
        if self._dev.get("key") != key:
            nbytes = max(_lib.volume_filter_scratch_bytes(J, f.grid, f.radius),
                         _lib.volume_transition_stats_scratch_bytes(J, f.grid, f.radius))
            self._dev = {"key": key,
                         "state": torch.empty((J, f.voxels), device=dev, dtype=torch.float32),
                         "scratch": torch.empty(nbytes, device=dev, dtype=torch.uint8),
                         "joints": torch.empty((T, J, 3), device=dev, dtype=torch.float32),
                         "evidence": torch.empty((T, J), device=dev, dtype=torch.float32),
                         "stats": torch.empty((T, J, _lib.STATS_SLOTS), device=dev, dtype=torch.float32),
                         "linked": torch.empty((T, J), device=dev, dtype=torch.int32)}
        return self._dev

    @torch.no_grad()
    def fit(self, iterations=8, tol=1e-6, fit_sigma=True, fit_floor=True, floor_bounds=(1e-6, 0.5), stream=None):
        """Fit ``sigma`` and ``floor`` to the stored frames by at most ``iterations`` EM iterations on ``stream`` (default: the current
        one; it waits for every push).  Per iteration: ``se_volume_filter_f32`` over the stored frames with the current taps (beliefs
        and restart flags kept), ``se_volume_transition_stats_f32`` over them, last push first, and the M-step on the host, which
        waits for the device once per iteration.  It stops early, as ``converged``, when the log-likelihood changes by less than ``tol`` of
        its magnitude, up or down (in float32 it can fall by rounding alone); ``tol=0`` never stops early, and a fall larger than
        ``tol`` (a ``Z`` restart that came or went) does not stop the loop either.
        ``fit_sigma=False`` / ``fit_floor=False`` hold one parameter; ``floor_bounds`` clamps the fitted floor.

        Returns a dict: ``sigma``, ``floor``, ``radius`` (unchanged), ``log_likelihood`` (a list: ``sum ln Z`` under the parameters of
        each iteration, the last one under the returned parameters), ``history`` (per entry of that list: sigma, floor,
        log_likelihood and the number of terms), ``mean_sq_step`` (metres^2, of the last E-step), ``pairs`` (linked pairs it pooled),
        ``converged``, ``saturated``, ``truncation_binding`` (3 sigma / h > radius: refit with a larger radius) and, as a diagnostic,
        ``sigma_per_joint`` and ``floor_per_joint`` [J] (numpy).  The stored frames stay: ``reset()`` forgets them.  An argument error,
        or a call with nothing stored, raises ValueError before anything touches the device."""
        iterations, tol, floor_bounds = check_fit_args(iterations, tol, floor_bounds)
        if not self._pushes:
            raise ValueError("fit: nothing is stored; push() the frames of the sequence first")
        pushes, dev, J, stream = self._begin_finish(stream)
        f = self.filter
        h = f.cuboid_side / f.grid
        with torch.cuda.stream(stream):
            T = self.frames_stored
            ws = self._workspace(dev, J, T)
            coord = f._device_constants(dev, J)["coord"]
            ones = f._device_constants(dev, J)["ones"]
            for p in pushes:
                for t in (p.volumes, p.beliefs, p.restarted):
                    t.record_stream(stream)

            def e_step(sigma, floor, want_stats):
                taps = torch.from_numpy(gaussian_taps(sigma, f.radius, h)).to(dev)
                t0 = 0
                for i, p in enumerate(pushes):
                    B = int(p.volumes.shape[0])
                    _lib.volume_filter(p.volumes, coord, taps, ws["state"], p.beliefs, ws["joints"][t0:t0 + B],
                                       ws["evidence"][t0:t0 + B], p.restarted, B, J, f.voxels, f.grid, f.radius, floor,
                                       have_prior=None if i == 0 else ones, scratch=ws["scratch"])
                    t0 += B
                restarted = torch.cat([p.restarted for p in pushes])
                if not want_stats:
                    return ws["evidence"].cpu().numpy(), restarted.cpu().numpy(), None, None
                t1 = T
                for i in range(len(pushes) - 1, -1, -1):
                    p = pushes[i]
                    B = int(p.volumes.shape[0])
                    link = None if i == len(pushes) - 1 else (pushes[i + 1].restarted[0] == 0).to(torch.int32)
                    _lib.volume_transition_stats(p.volumes, p.beliefs, p.restarted, taps, ws["state"], ws["stats"][t1 - B:t1],
                                                 ws["linked"][t1 - B:t1], B, J, f.voxels, f.grid, f.radius, floor, have_link=link,
                                                 scratch=ws["scratch"])
                    t1 -= B
                return ws["evidence"].cpu().numpy(), restarted.cpu().numpy(), ws["stats"].cpu().numpy(), ws["linked"].cpu().numpy()

            result = em_loop(e_step, f.sigma, f.floor, f.grid, f.radius, h, iterations, tol, bool(fit_sigma), bool(fit_floor),
                             floor_bounds)
            self._done = torch.cuda.Event()
            self._done.record(stream)
        return result
