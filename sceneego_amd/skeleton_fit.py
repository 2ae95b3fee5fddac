"""Fit the skeleton model of ``SkeletonPrior`` and ``SkeletonPose`` to a sequence: EM for the bone lengths, ``tau`` and ``floor``, the
E-step on the device (``csrc/skeleton_prior.hip``, ``se_skeleton_edge_stats_f32``), the M-step on the host in float64.

Both operators rest on three per-wearer guesses: the bone lengths (``--bone_lengths``, or the per-bone median of distances between raw
soft-argmax joints, which are expectations of sometimes two-lobed volumes), ``tau`` and ``floor``.  The edge factor
``(1 - floor) w_L,tau(d) + floor / N`` is a two-component mixture whose shell part is an exponential family in ``(|d|, |d|^2)`` on a
fixed set of taps, so the model can be fitted to the volumes of a sequence without annotated data:

    E-step   per frame and edge c (parent[c] -> c), from the messages ``couple`` forms (A_c, s_c upward; E_c, t_c downward):
                 S0 = sum E_c corr(A_c, w_c)    S1 = sum E_c corr(A_c, w_c r)    S2 = sum E_c corr(A_c, w_c r^2)    SJ = (floor / N) t_c s_c
                 m = (1 - floor) S0 / ((1 - floor) S0 + SJ)  the posterior mass of a shell step (1 - m: of a jump),
                 S1 / S0, S2 / S0                             the posterior expected bone length and its square given a step
             with (1 - floor) S0 + SJ = s_c Z_parent(c) and the frame's likelihood ln Z_0 + sum_c ln s_c.
    M-step   floor' = the share of jump mass over all edges and frames, clamped to ``floor_bounds``; per edge n_c = sum_f m and the
             m-weighted means rbar_c, r2bar_c; then six rounds of two exact one-dimensional maxima: L_c such that the mean of r under
             the taps equals rbar_c, and the shared tau such that sum_c n_c (E_w[(r - L_c)^2] - (r2bar_c - 2 L_c rbar_c + L_c^2)) = 0,
             both by bisection.

The support of every edge is cut once, at the start of ``fit()``: Sup_c = {d : |r(d) - L0_c| <= 3 tau0} inside the block of radius
R = default_radius(L0, tau0, h).  With it the family is fixed, so EM cannot lower the likelihood while the set of valid frames stays
the same; the clamps are constrained maxima of concave problems and keep that property.  ``truncation_binding[c]``
(|L_c - L0_c| + 3 tau > 3 tau0) says that the fitted shell is cut by its support: fit again from the fitted values, which cuts it anew.

Read the result for what it is: a maximum-likelihood fit to the network's own volumes read as likelihoods, on one sequence.  It says
which lengths, ``tau`` and ``floor`` explain those volumes best under this model; it is not a validation against ground truth, and a
lattice of edge h cannot resolve a shell thinner than about h / 2, which is why ``tau`` is bounded there.  ``SkeletonPrior`` takes one
``tau``: the per-edge values are a diagnostic.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .skeleton_prior import KINEMATIC_PARENTS, MAX_GRID, MAX_RADIUS, _edge_lengths, check_parents, default_radius
from .volume_filter import StoredTrack

FIT_KEYS = ("bone_lengths", "tau", "floor", "radius", "log_likelihood", "history", "step_mass", "mean_length", "tau_per_edge",
            "frames_used", "converged", "saturated", "truncation_binding")
ROUNDS = 6                 # coordinate-ascent rounds of one M-step
LENGTH_REACH = 6.0         # L_c is searched within L0_c +- LENGTH_REACH tau0 (twice the support's half width)


# ---------------------------------------------------------------------------------------------------------------------------- the family
class Support(NamedTuple):
    """The fixed support of one fit: ``r`` [(2R+1)^3] float64 (|d| h, metres), ``mask`` [J, (2R+1)^3] bool (row 0 empty), the values
    it was cut at and the block radius."""
    r: np.ndarray
    mask: np.ndarray
    rc: tuple                  # per edge the r of its support's taps alone
    lengths: np.ndarray
    tau: float
    h: float
    radius: int


def cut_support(lengths, tau, voxel_edge, radius=None):
    """Sup_c = {d : |r(d) - L0_c| <= 3 tau0} inside the block of ``radius`` (default: ``default_radius(L0, tau0, h)``).  ``lengths``
    [J] with entry 0 ignored.  ValueError where an edge has no tap."""
    L = np.asarray(lengths, dtype=np.float64).reshape(-1)
    tau, h = float(tau), float(voxel_edge)
    if L.size < 2 or not (np.isfinite(L[1:]).all() and (L[1:] > 0).all()):
        raise ValueError(f"lengths must hold an edge and be positive and finite (entry 0 is ignored), got {L.tolist()}")
    if not (tau > 0.0 and math.isfinite(tau)) or not (h > 0.0 and math.isfinite(h)):
        raise ValueError(f"tau = {tau} and the voxel edge {h} must be positive and finite")
    R = default_radius(L[1:], tau, h) if radius is None else int(radius)
    if not default_radius(L[1:], tau, h) <= R <= MAX_RADIUS:
        raise ValueError(f"radius = {R}: {default_radius(L[1:], tau, h)}..{MAX_RADIUS} expected")
    ax = np.arange(-R, R + 1, dtype=np.float64)
    dist = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) * h
    r = dist.reshape(-1)
    mask = np.zeros((L.size, r.size), dtype=bool)
    for j in range(1, L.size):
        mask[j] = np.abs(r - L[j]) <= 3.0 * tau
        if not mask[j].any():
            raise ValueError(f"no voxel lies within 3 tau = {3 * tau} m of the bone length {L[j]} m at a voxel edge of {h} m")
    L = L.copy()
    L[0] = 0.0
    return Support(r, mask, tuple(r[m] for m in mask), L, tau, h, R)


def _weights(r, L, tau):
    """exp(-(r - L)^2 / (2 tau^2)) normalised over the taps ``r`` of one support, in float64; the largest exponent is taken out first,
    so an L far from the support cannot underflow every tap."""
    off = r - L
    e = -(off * off) / (2.0 * tau * tau)
    w = np.exp(e - e.max())
    return w / w.sum()


def support_taps(support, lengths, tau):
    """The three tap blocks ``(w, w1, w2)`` [J, (2R+1)^3] float32 of the shells (``lengths``, ``tau``) on the fixed ``support``:
    w64 = exp(-(r - L_c)^2 / (2 tau^2)) on Sup_c and 0 elsewhere, normalised in float64; w = float32(w64), w1 = float32(w64 r),
    w2 = float32(w64 r^2).  At the values the support was cut at, ``w`` equals ``shell_taps`` bit for bit."""
    L = np.asarray(lengths, dtype=np.float64).reshape(-1)
    J, n = support.mask.shape
    if L.size != J:
        raise ValueError(f"lengths holds {L.size} values, {J} expected")
    out = [np.zeros((J, n), dtype=np.float32) for _ in range(3)]
    tau, r = float(tau), support.r
    for j in range(1, J):
        # over the whole block, zeros included, as shell_taps sums it: the same pairwise sum, so the same bits
        off = r - L[j]
        w = np.where(support.mask[j], np.exp(-(off * off) / (2.0 * tau * tau)), 0.0)
        total = w.sum()
        if total > 0.0:
            w = w / total
        else:
            w[support.mask[j]] = _weights(r[support.mask[j]], L[j], tau)
        out[0][j] = w.astype(np.float32)
        out[1][j] = (w * r).astype(np.float32)
        out[2][j] = (w * r * r).astype(np.float32)
    return tuple(out)


def tap_moments(support, j, L, tau):
    """(E_w[r], E_w[(r - L)^2]) under the normalised taps of edge ``j`` at (L, tau), float64."""
    r = support.rc[j]
    w = _weights(r, float(L), float(tau))
    return float((w * r).sum()), float((w * (r - L) ** 2).sum())


def _bisect(f, lo, hi):
    """The root of the rising function ``f`` in [lo, hi] (f(lo) <= 0 <= f(hi)), to the last bit."""
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if f(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def solve_length(support, j, rbar, tau):
    """``(L, clamped)``: the L at which the taps' mean of r over Sup_j equals ``rbar`` at the fixed ``tau`` - the exact maximum of the
    length step, whose objective is concave in L / tau^2 - searched in L0_j +- 6 tau0 (and above h / 100); where the root lies outside,
    the nearer end and ``clamped``."""
    L0 = float(support.lengths[j])
    lo, hi = max(L0 - LENGTH_REACH * support.tau, 0.01 * support.h), L0 + LENGTH_REACH * support.tau
    f = lambda L: tap_moments(support, j, L, tau)[0] - rbar        # noqa: E731  rises with L: its slope is Var_w[r] / tau^2
    if f(lo) >= 0.0:
        return lo, True
    if f(hi) <= 0.0:
        return hi, True
    return _bisect(f, lo, hi), False


def tau_residual(support, lengths, tau, n, rbar, r2bar, edges=None):
    """sum_c n_c (E_w[(r - L_c)^2] - (r2bar_c - 2 L_c rbar_c + L_c^2)) over ``edges`` (default: all with n_c > 0): rises with tau."""
    total = 0.0
    for c in (range(1, len(lengths)) if edges is None else edges):
        if n[c] > 0.0:
            total += n[c] * (tap_moments(support, c, lengths[c], tau)[1] - (r2bar[c] - 2.0 * lengths[c] * rbar[c] + lengths[c] ** 2))
    return total


def solve_tau(support, lengths, n, rbar, r2bar, tau_bounds, edges=None):
    """``(tau, clamped)``: the root of ``tau_residual`` inside ``tau_bounds`` - the exact maximum of the tau step, concave in
    1 / tau^2 - or the bound it lies beyond."""
    lo, hi = tau_bounds
    f = lambda t: tau_residual(support, lengths, t, n, rbar, r2bar, edges)      # noqa: E731
    if f(lo) >= 0.0:
        return lo, True
    if f(hi) <= 0.0:
        return hi, True
    return _bisect(f, lo, hi), False


def shell_objective(support, lengths, tau, n, rbar, r2bar):
    """The shell part of the expected complete log-likelihood Q: sum_c n_c (-(r2bar_c - 2 L_c rbar_c + L_c^2) / (2 tau^2) - ln sum_{d in
    Sup_c} exp(-(r - L_c)^2 / (2 tau^2))), in float64."""
    q = 0.0
    for c in range(1, len(lengths)):
        if n[c] > 0.0:
            off = support.rc[c] - lengths[c]
            e = -(off * off) / (2.0 * tau * tau)
            top = e.max()
            q += n[c] * (-(r2bar[c] - 2.0 * lengths[c] * rbar[c] + lengths[c] ** 2) / (2.0 * tau * tau) - (top + math.log(np.exp(e - top).sum())))
    return q


# ---------------------------------------------------------------------------------------------------------------------------- E and M
def edge_posteriors(stats, valid, floor):
    """From ``stats`` [F, J, 4] (S0, S1, S2, SJ as ``se_skeleton_edge_stats_f32`` writes them) and ``valid`` [F], under the ``floor``
    the pass ran with (rounded to float32 as the kernel is given it), in float64: ``mass`` [F, J] = (1 - floor) S0 / ((1 - floor) S0 +
    SJ), ``er`` = S1 / S0, ``er2`` = S2 / S0, and ``ok`` [F, J]: the frame is valid and all three are finite.  Column 0 is never ok."""
    stats = np.asarray(stats, dtype=np.float64)
    valid = np.asarray(valid) != 0
    if stats.ndim != 3 or stats.shape[2] != _lib.EDGE_STATS_SLOTS or valid.shape != stats.shape[:1]:
        raise ValueError(f"stats {stats.shape} ([F, J, {_lib.EDGE_STATS_SLOTS}]) and valid {valid.shape} ([F]) expected")
    keep = float(np.float32(1.0) - np.float32(floor))
    S0, S1, S2, SJ = (stats[..., k] for k in range(4))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mass = keep * S0 / (keep * S0 + SJ)
        er, er2 = S1 / S0, S2 / S0
    ok = valid[:, None] & np.isfinite(mass) & np.isfinite(er) & np.isfinite(er2)
    ok[:, 0] = False
    return {"mass": mass, "er": er, "er2": er2, "ok": ok}


def log_likelihood(norms, valid):
    """``(sum over the valid frames of ln Z_0 + sum_{c >= 1} ln s_c, frames)`` from ``norms`` [F, J, 3] (s, t, Z), in float64."""
    norms = np.asarray(norms, dtype=np.float64)
    valid = np.asarray(valid) != 0
    rows = norms[valid]
    return float(np.log(rows[:, 0, 2]).sum() + np.log(rows[:, 1:, 0]).sum()), int(valid.sum())


def m_step(stats, valid, floor, support, lengths, tau, fit_lengths=True, fit_tau=True, floor_bounds=(1e-6, 0.5), tau_bounds=None,
           trace=None):
    """The pooling and the M-step in float64 from one E-step.  Returns a dict: ``floor``, ``bone_lengths`` [J], ``tau`` (the new
    values), ``saturated``, ``step_mass`` [J] (n_c over the frames used), ``mean_length`` [J] (rbar_c), ``tau_per_edge`` [J],
    ``frames_used`` and ``edges`` (edge-frames pooled).  ``trace``: a list that receives (step, Q before, Q after) of every coordinate
    step."""
    L = np.array(lengths, dtype=np.float64)
    J = L.size
    tb = (support.h / 2.0, 3.0 * support.tau) if tau_bounds is None else (float(tau_bounds[0]), float(tau_bounds[1]))
    post = edge_posteriors(stats, valid, floor)
    ok, mass = post["ok"], np.where(post["ok"], post["mass"], 0.0)
    n = mass.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rbar = np.where(n > 0, np.where(ok, mass * post["er"], 0.0).sum(axis=0) / n, np.nan)
        r2bar = np.where(n > 0, np.where(ok, mass * post["er2"], 0.0).sum(axis=0) / n, np.nan)
    edges = int(ok.sum())
    new_floor, saturated = float(floor), False
    if edges:
        share = float(np.where(ok, 1.0 - post["mass"], 0.0).sum()) / edges
        new_floor = min(max(share, floor_bounds[0]), floor_bounds[1])
        saturated = new_floor != share
    tau = float(tau)
    clamp_L, clamp_tau = np.zeros(J, dtype=bool), False
    for _ in range(ROUNDS if edges else 0):
        if fit_lengths:
            for c in range(1, J):
                if n[c] > 0.0:
                    before = None if trace is None else shell_objective(support, L, tau, n, rbar, r2bar)
                    L[c], clamp_L[c] = solve_length(support, c, rbar[c], tau)
                    if trace is not None:
                        trace.append(("length", before, shell_objective(support, L, tau, n, rbar, r2bar)))
        if fit_tau and n.sum() > 0.0:
            before = None if trace is None else shell_objective(support, L, tau, n, rbar, r2bar)
            tau, clamp_tau = solve_tau(support, L, n, rbar, r2bar, tb)
            if trace is not None:
                trace.append(("tau", before, shell_objective(support, L, tau, n, rbar, r2bar)))
    per_edge = np.full(J, np.nan)
    for c in range(1, J):
        if n[c] > 0.0:
            per_edge[c] = solve_tau(support, L, n, rbar, r2bar, tb, edges=(c,))[0]
    used = int((np.asarray(valid) != 0).sum())
    return {"floor": new_floor, "bone_lengths": L, "tau": tau, "saturated": bool(saturated or clamp_tau or clamp_L.any()),
            "step_mass": n / max(used, 1), "mean_length": rbar, "tau_per_edge": per_edge, "frames_used": used, "edges": edges}


def truncation_binding(support, lengths, tau):
    """[J] bool: |L_c - L0_c| + 3 tau > 3 tau0 (entry 0 False)."""
    out = np.abs(np.asarray(lengths, dtype=np.float64) - support.lengths) + 3.0 * float(tau) > 3.0 * support.tau
    out[0] = False
    return out


def check_fit_args(iterations, tol, floor_bounds, tau_bounds):
    """fit()'s own arguments, as (iterations, tol, floor bounds, tau bounds or None); ValueError before anything touches a device."""
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
    if tau_bounds is not None:
        try:
            tlo, thi = (float(x) for x in tau_bounds)
        except (TypeError, ValueError):
            raise ValueError(f"fit: tau_bounds = {tau_bounds!r} must be None or a pair (low, high)") from None
        if not (0.0 < tlo <= thi and math.isfinite(thi)):
            raise ValueError(f"fit: tau_bounds = {tau_bounds}: 0 < low <= high expected")
        tau_bounds = (tlo, thi)
    return int(iterations), tol, (lo, hi), tau_bounds


def em_loop(e_step, support, floor, iterations, tol, fit_lengths, fit_tau, fit_floor, floor_bounds, tau_bounds):
    """The EM loop around ``e_step(taps, floor) -> (stats [F, J, 4], norms [F, J, 3], valid [F])`` with ``taps`` the three blocks of
    ``support_taps``: per iteration the likelihood under the current parameters, the stop test (a relative change below ``tol``, up or
    down) and the M-step.  ``SkeletonModelFit.fit`` runs it over the device pass and tests/skeleton_fit_model.py over the float64
    model, so both take the same decisions.  Returns the dict of ``fit``."""
    L, tau, floor = support.lengths.copy(), support.tau, float(floor)
    ll, history, last, converged = [], [], None, False
    for it in range(iterations + 1):
        stats, norms, valid = e_step(support_taps(support, L, tau), floor)
        value, used = log_likelihood(norms, valid)
        ll.append(value)
        history.append({"bone_lengths": L[1:].tolist(), "tau": tau, "floor": floor, "log_likelihood": value, "frames": used})
        converged = it > 0 and abs(value - ll[-2]) < tol * abs(ll[-2])
        if it == iterations or converged or used == 0:
            break
        last = m_step(stats, valid, floor, support, L, tau, fit_lengths, fit_tau, floor_bounds, tau_bounds)
        if last["edges"] == 0:
            break
        L, tau = last["bone_lengths"], last["tau"]
        if fit_floor:
            floor = last["floor"]
    J = L.size
    nan = np.full(J, np.nan)
    return {"bone_lengths": L, "tau": tau, "floor": floor, "radius": support.radius, "log_likelihood": ll, "history": history,
            "step_mass": nan if last is None else last["step_mass"], "mean_length": nan if last is None else last["mean_length"],
            "tau_per_edge": nan if last is None else last["tau_per_edge"], "frames_used": history[-1]["frames"],
            "converged": converged, "saturated": bool(last is not None and last["saturated"]),
            "truncation_binding": truncation_binding(support, L, tau)}


# ---------------------------------------------------------------------------------------------------------------------------- device
class _Push(NamedTuple):
    """One stored push: the copy of its volumes [B,J,G,G,G] and the event behind the copy.  ``restarted`` [B,J] and ``given`` are what
    ``StoredTrack`` expects of a push; neither is used here."""
    volumes: torch.Tensor
    restarted: torch.Tensor
    given: None
    event: torch.cuda.Event


class SkeletonModelFit(StoredTrack):
    """``m = SkeletonModelFit(grid, cuboid_side, bone_lengths, tau=0.03, floor=1e-3, parents=KINEMATIC_PARENTS, max_bytes=None)``;
    ``m.push(volumes)`` per batch (the frames need not be consecutive), ``m.fit()`` for the fitted bone lengths, ``tau`` and ``floor``.
    The parameters are ``SkeletonPrior``'s, here the values the fit starts from, and a bad one raises ValueError before anything
    touches the device.  ``max_bytes``: the most the stored volumes may take (B x J x G^3 x 4 bytes per push: 15.7 MB per frame at
    15 x 64^3); default: half of the device memory that is free at the first push."""

    _budget_advice = "fit fewer frames or raise max_bytes"

    def __init__(self, grid, cuboid_side, bone_lengths, tau=0.03, floor=1e-3, parents=KINEMATIC_PARENTS, max_bytes=None):
        grid, cuboid_side, tau, floor = int(grid), float(cuboid_side), float(tau), float(floor)
        self.parents = check_parents(parents)
        J = len(self.parents)
        if J < 2:
            raise ValueError("a skeleton of one joint has no edge to fit")
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
        self.grid, self.cuboid_side, self.tau, self.floor, self.radius, self.joints = grid, cuboid_side, tau, floor, radius, J
        self.voxels = grid ** 3
        self._init_store(max_bytes)
        self._dev = {}

    @property
    def bytes_stored(self):
        return sum(p.volumes.numel() * 4 for p in self._pushes)

    def reset(self):
        """Forget everything: the stored frames.  Nothing is queued on the device."""
        self._pushes = []

    @torch.no_grad()
    def push(self, volumes, stream=None):
        """``volumes`` [B,J,G,G,G] float32 (softmaxed, as ``forward()`` returns them): a copy is stored (``forward()``'s volumes are
        static buffers under graphs and the pipeline).  Nothing is computed.  Raises ValueError, with nothing allocated, once the
        stored bytes plus this push would exceed ``max_bytes``."""
        G, J = self.grid, self.joints
        if not isinstance(volumes, torch.Tensor) or volumes.dim() != 5 or tuple(volumes.shape[1:]) != (J, G, G, G) \
                or volumes.dtype != torch.float32 or volumes.shape[0] < 1:
            raise ValueError("push: volumes must be a [B,%d,%d,%d,%d] float32 tensor with B >= 1, got %s"
                             % (J, G, G, G, (tuple(volumes.shape), volumes.dtype) if isinstance(volumes, torch.Tensor) else type(volumes)))
        _lib.require_hip(volumes)
        B = int(volumes.shape[0])
        self._admit(B, B * J * self.voxels * 4, volumes.device)
        stream = stream if stream is not None else torch.cuda.current_stream(volumes.device)
        with torch.cuda.stream(stream):
            vol = volumes.clone(memory_format=torch.contiguous_format)
            event = torch.cuda.Event()
            event.record(stream)
            self._pushes.append(_Push(vol, torch.empty((B, J), device=volumes.device, dtype=torch.int32), None, event))

    def _workspace(self, dev, T, B):
        key = (str(dev), T, B)
        if self._dev.get("key") != key:
            J = self.joints
            self._dev = {"key": key,
                         "scratch": torch.empty(_lib.skeleton_edge_stats_scratch_bytes(B, J, self.grid, self.radius), device=dev,
                                                dtype=torch.uint8),
                         "stats": torch.empty((T, J, _lib.EDGE_STATS_SLOTS), device=dev, dtype=torch.float32),
                         "norms": torch.empty((T, J, 3), device=dev, dtype=torch.float32),
                         "valid": torch.empty((T,), device=dev, dtype=torch.int32)}
        return self._dev

    @torch.no_grad()
    def e_step(self, taps, floor, stream=None):
        """One pass of ``se_skeleton_edge_stats_f32`` over the stored frames with the three tap blocks ``taps`` (``support_taps``):
        host arrays ``(stats [T, J, 4], norms [T, J, 3], valid [T])``.  Waits for the device."""
        pushes, dev, J, stream = self._begin_finish(stream)
        with torch.cuda.stream(stream):
            ws = self._workspace(dev, self.frames_stored, max(int(p.volumes.shape[0]) for p in pushes))
            w = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in taps]
            t0 = 0
            for p in pushes:
                p.volumes.record_stream(stream)
                B = int(p.volumes.shape[0])
                _lib.skeleton_edge_stats(p.volumes, w[0], w[1], w[2], self.parents, ws["stats"][t0:t0 + B], ws["norms"][t0:t0 + B],
                                         ws["valid"][t0:t0 + B], B, self.voxels, self.grid, self.radius, floor, scratch=ws["scratch"])
                t0 += B
            out = ws["stats"].cpu().numpy(), ws["norms"].cpu().numpy(), ws["valid"].cpu().numpy()
            self._done = torch.cuda.Event()
            self._done.record(stream)
        return out

    @torch.no_grad()
    def fit(self, iterations=8, tol=1e-6, fit_lengths=True, fit_tau=True, fit_floor=True, floor_bounds=(1e-6, 0.5), tau_bounds=None,
            stream=None):
        """Fit the bone lengths, ``tau`` and ``floor`` to the stored frames by at most ``iterations`` EM iterations on ``stream``
        (default: the current one; it waits for every push).  The support of every edge is cut here, at the constructor's values, and
        stays; per iteration one ``se_skeleton_edge_stats_f32`` pass over the stored frames and the M-step on the host, which waits
        for the device once.  A frame in which ``couple`` would fall back is skipped.  It stops early, as ``converged``, when the
        log-likelihood changes by less than ``tol`` of its magnitude, up or down; ``tol=0`` never stops early.
        ``fit_lengths=False`` / ``fit_tau=False`` / ``fit_floor=False`` hold a parameter; ``floor_bounds`` clamps the fitted floor and
        ``tau_bounds`` (default ``(h / 2, 3 tau)``) the fitted tau.

        Returns a dict: ``bone_lengths`` [J] float64 (entry 0 is 0), ``tau``, ``floor``, ``radius`` (unchanged),
        ``log_likelihood`` (a list: the sum over the valid frames of ln Z_0 + sum ln s_c under the parameters of each iteration, the
        last one under the returned parameters), ``history`` (per entry of that list: bone_lengths, tau, floor, log_likelihood and the
        valid frames), ``step_mass`` [J] (the mean posterior mass of a shell step), ``mean_length`` [J] (the posterior mean bone length
        of the last E-step), ``tau_per_edge`` [J] (a diagnostic: the operators take one tau), ``frames_used``, ``converged``,
        ``saturated`` (a bound was active in the last M-step) and ``truncation_binding`` [J] (|L_c - L0_c| + 3 tau > 3 tau0: fit again
        from the fitted values).  The stored frames stay: ``reset()`` forgets them.  An argument error, or a call with nothing
        stored, raises ValueError before anything touches the device."""
        iterations, tol, floor_bounds, tau_bounds = check_fit_args(iterations, tol, floor_bounds, tau_bounds)
        if not self._pushes:
            raise ValueError("fit: nothing is stored; push() the frames of the sequence first")
        support = cut_support(self.bone_lengths, self.tau, self.cuboid_side / self.grid, self.radius)
        return em_loop(lambda taps, floor: self.e_step(taps, floor, stream), support, self.floor, iterations, tol, bool(fit_lengths),
                       bool(fit_tau), bool(fit_floor), floor_bounds, tau_bounds)
