"""CPU: the float64 model of the edge statistics (tests/skeleton_fit_model.py) gives the expectations over the pairwise posterior of the
skeleton tree it claims to, the three identities hold, the tap builder starts from ``shell_taps`` bit for bit, the M-step solves its
moment equations and raises its objective at every coordinate step, EM on the model does not lower the likelihood, and the Python
surface refuses bad arguments before anything touches a device.

TOLERANCES.  The dense and brute-force comparisons are float64 against float64: 1e-10 and 1e-12 as the definition states them.  The
likelihood of an EM run may fall by rounding alone: the E-step takes its taps rounded to float32 while the M-step maximises over the
float64 family, so each of the frames x (J - 1) edge terms of the log-likelihood can be off by one float32 rounding of its taps, 2^-24
relative, on either side of a comparison: a fall of up to frames x (J - 1) x 2^-23 is not a failure of EM.  Q is compared with itself
across an exact maximisation, evaluated in float64 from sums of a few thousand terms: 1e-12 of its magnitude.
"""
import functools

import numpy as np
import pytest

from sceneego_amd import skeleton_fit
from sceneego_amd.skeleton_fit import SkeletonModelFit, cut_support, edge_posteriors, log_likelihood, m_step, support_taps
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, default_radius, shell_taps
from skeleton_fit_model import edge_stats_model, fit_model
from skeleton_prior_cases import CHAIN3, SIDE, STAR5, lengths_for, make_logits
from skeleton_prior_model import children
from volume_filter_cases import softmax32

TREES = {"tree15": KINEMATIC_PARENTS, "star5": STAR5, "chain3": CHAIN3}


def float64_blocks(lengths, tau, h, R):
    """(w, w r, w r^2) unrounded, [J, (2R+1)^3] float64, and r [(2R+1)^3]: the blocks the identities hold with exactly."""
    sup = cut_support(lengths, tau, h, R)
    w = np.zeros(sup.mask.shape)
    for j in range(1, len(lengths)):
        off = sup.r - lengths[j]
        v = np.where(sup.mask[j], np.exp(-(off * off) / (2.0 * tau * tau)), 0.0)
        w[j] = v / v.sum()
    return w, w * sup.r, w * sup.r ** 2, sup.r


def dense_factor(w, G, R):
    """W[x, y] = w(y - x) over all pairs of the G^3 states, 0 outside the block; and the offsets' flat tap index (-1 outside)."""
    ax = np.arange(G)
    idx = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    d = idx[None, :, :] - idx[:, None, :]                     # y - x
    inside = (np.abs(d) <= R).all(axis=-1)
    tap = ((d[..., 0] + R) * (2 * R + 1) + d[..., 1] + R) * (2 * R + 1) + d[..., 2] + R
    tap = np.where(inside, tap, 0)
    return np.where(inside, np.asarray(w, dtype=np.float64)[tap], 0.0), np.where(inside, tap, -1)


# ------------------------------------------------------------------------------------------------------------------ the claim
@pytest.mark.parametrize("tree", ["tree15", "star5", "chain3"])
def test_the_statistics_are_expectations_over_the_dense_pairwise_posterior(tree):
    """G = 4, floor 1e-2: unnormalised sum-product over the tree with dense 64 x 64 factors M_c = keep W_c + uniform.  The pairwise
    posterior of edge c is e_c(x) M_c[x, y] a_c(y); its shell share, its jump share and the shell part's means of r and r^2 are what the
    model's S0, S1, S2, SJ give.  Unrounded float64 blocks, so that S1 / S0 is the mean of r itself."""
    parents = TREES[tree]
    G, R, floor = 4, 3, 1e-2
    J, N, h = len(parents), G ** 3, SIDE / G
    lengths = lengths_for(parents, G, R, 40 + J)
    w, w1, w2, r = float64_blocks(lengths, 0.5 * h, h, R)
    p32 = softmax32(0.5 * make_logits(1, parents, lengths, G, 41 + J)[0])
    stats, norms, valid = edge_stats_model(p32, w, w1, w2, parents, G, floor)
    post = edge_posteriors(stats, valid, floor)
    assert valid.all()

    eps = float(np.float32(floor))
    keep = float(np.float32(1.0) - np.float32(floor))
    p = p32[0].astype(np.float64)
    ch = children(parents)
    Wd, M, Rd = [None] * J, [None] * J, [None] * J
    for c in range(1, J):
        Wd[c], tap = dense_factor(w[c], G, R)
        Rd[c] = np.where(tap >= 0, r[np.maximum(tap, 0)], 0.0)
        M[c] = keep * Wd[c] + eps / N
    a, u, dn = [None] * J, [None] * J, [None] * J
    for j in range(J - 1, 0, -1):
        a[j] = p[j] * np.prod([u[k] for k in ch[j]], axis=0) if ch[j] else p[j].copy()
        u[j] = M[j] @ a[j]
    for j in range(J):
        base = p[j] if j == 0 else p[j] * dn[j]
        for c in ch[j]:
            e = base * np.prod([u[k] for k in ch[j] if k != c], axis=0) if len(ch[j]) > 1 else base.copy()
            dn[c] = e @ M[c]
            pair = e[:, None] * a[c][None, :]
            shell, jump = (pair * keep * Wd[c]).sum(), (pair * eps / N).sum()
            want = {"mass": shell / (shell + jump), "jump": jump / (shell + jump),
                    "er": (pair * Wd[c] * Rd[c]).sum() / (pair * Wd[c]).sum(), "er2": (pair * Wd[c] * Rd[c] ** 2).sum() / (pair * Wd[c]).sum()}
            got = {"mass": post["mass"][0, c], "jump": 1.0 - post["mass"][0, c], "er": post["er"][0, c], "er2": post["er2"][0, c]}
            for key in want:
                assert abs(got[key] - want[key]) <= 1e-10 * max(abs(want[key]), 1e-3), (tree, c, key, got[key], want[key])


def test_the_likelihood_is_the_sum_over_all_poses():
    """A chain of three joints at G = 3: sum over all 27^3 poses of prod p_j(x_j) prod_c M_c[x_parent, x_c] against
    exp(ln Z_0 + ln s_1 + ln s_2), 1e-12 relative.  The shortest bone puts d = 0 inside its shell (w1 = w2 = 0 where w != 0)."""
    G, R, floor = 3, 2, 1e-2
    N, h = G ** 3, SIDE / G
    lengths = lengths_for(CHAIN3, G, R, 7)
    sup = cut_support(lengths, 0.5 * h, h, R)
    taps = support_taps(sup, lengths, 0.5 * h)
    centre = ((2 * R + 1) ** 3 - 1) // 2
    assert taps[0][1, centre] != 0 and taps[1][1, centre] == 0 and taps[2][1, centre] == 0
    p32 = softmax32(0.5 * make_logits(1, CHAIN3, lengths, G, 8)[0])
    stats, norms, valid = edge_stats_model(p32, *taps, CHAIN3, G, floor)
    got, frames = log_likelihood(norms, valid)
    eps = float(np.float32(floor))
    M = [None] + [(1.0 - eps) * dense_factor(taps[0][c], G, R)[0] + eps / N for c in (1, 2)]
    p = p32[0].astype(np.float64)
    brute = np.einsum("x,y,z,xy,yz->", p[0], p[1], p[2], M[1], M[2])          # edges 0 -> 1 and 1 -> 2
    assert frames == 1 and abs(got - np.log(brute)) <= 1e-12 * abs(np.log(brute)), (got, np.log(brute))


@pytest.mark.parametrize("tree,G,R", [("tree15", 8, 4), ("star5", 6, 3), ("chain3", 8, 5)])
def test_shell_and_jump_mass_sum_to_the_evidence(tree, G, R):
    """(1 - floor) S0 + SJ = s_c Z_parent(c), 1e-12 relative, with the float32 taps the kernels take."""
    parents = TREES[tree]
    h, floor = SIDE / G, 1e-3
    lengths = lengths_for(parents, G, R, 3 * G + R)
    taps = support_taps(cut_support(lengths, 0.5 * h, h, R), lengths, 0.5 * h)
    p32 = softmax32(make_logits(2, parents, lengths, G, 5 * G + R)[0])
    stats, norms, valid = edge_stats_model(p32, *taps, parents, G, floor)
    keep = 1.0 - float(np.float32(floor))
    assert valid.all() and (stats[:, 0] == 0).all()
    for c in range(1, len(parents)):
        lhs = keep * stats[:, c, 0] + stats[:, c, 3]
        rhs = norms[:, c, 0] * norms[:, parents[c], 2]
        assert (np.abs(lhs - rhs) <= 1e-12 * rhs).all(), (c, lhs, rhs)


# ------------------------------------------------------------------------------------------------------------------ taps and M-step
@pytest.mark.parametrize("G,R,tau_vox", [(16, 6, 0.5), (8, 5, 1.0), (64, 18, 0.96)])
def test_the_first_taps_are_shell_taps_bit_for_bit(G, R, tau_vox):
    h = SIDE / G
    if G == 64:
        lengths = np.concatenate([[0.0], np.random.default_rng(64).permutation(np.linspace(0.15, 0.45, 14))])
        tau = 0.03
    else:
        lengths, tau = lengths_for(KINEMATIC_PARENTS, G, R, G, tau_vox), tau_vox * h
    sup = cut_support(lengths, tau, h)
    assert sup.radius == R == default_radius(lengths[1:], tau, h)
    w, w1, w2 = support_taps(sup, lengths, tau)
    want = shell_taps(lengths, tau, h, R)
    assert w.dtype == np.float32 and np.array_equal(w.view(np.int32), want.view(np.int32))
    assert ((w1 == 0) | (w != 0)).all() and ((w2 == 0) | (w != 0)).all()


@functools.lru_cache(maxsize=None)
def chain16():
    """The 3-chain at 16^3: bones of 4.3 and 4.9 voxels, started 0.46 and 0.66 voxels off, tau0 one voxel (R = 9), four frames of
    two-lobed make_logits volumes."""
    G, h = 16, SIDE / 16
    truth = np.array([0.0, 4.3, 4.9]) * h
    start = truth + np.array([0.0, 0.46, 0.66]) * h
    assert default_radius(start[1:], h, h) == 9
    p32 = softmax32(make_logits(4, CHAIN3, truth, G, 1604)[0])
    return {"G": G, "h": h, "truth": truth, "start": start, "tau": h, "floor": 1e-3, "p": p32, "parents": CHAIN3}


@functools.lru_cache(maxsize=None)
def tree8():
    """The 15-joint tree at 8^3: bones of 1.6 to 2.0 voxels, tau0 one voxel (R = 5), two frames."""
    G, h = 8, SIDE / 8
    truth = np.concatenate([[0.0], np.random.default_rng(8).uniform(1.6, 2.0, 14)]) * h
    assert default_radius(truth[1:], h, h) == 5
    p32 = softmax32(make_logits(2, KINEMATIC_PARENTS, truth, G, 815)[0])
    return {"G": G, "h": h, "truth": truth, "start": truth, "tau": h, "floor": 1e-3, "p": p32, "parents": KINEMATIC_PARENTS}


@functools.lru_cache(maxsize=None)
def fitted(name, iterations=6):
    k = {"chain16": chain16, "tree8": tree8}[name]()
    return fit_model(k["p"], k["parents"], k["G"], SIDE, k["start"], k["tau"], k["floor"], iterations=iterations)


def test_the_bisections_meet_their_moment_equations_and_q_rises():
    k = chain16()
    sup = cut_support(k["start"], k["tau"], k["h"])
    stats, norms, valid = edge_stats_model(k["p"], *support_taps(sup, k["start"], k["tau"]), k["parents"], k["G"], k["floor"])
    trace = []
    out = m_step(stats, valid, k["floor"], sup, k["start"], k["tau"], trace=trace)
    post = edge_posteriors(stats, valid, k["floor"])
    n = post["mass"][:, 1:].sum(axis=0)
    rbar = (post["mass"] * post["er"])[:, 1:].sum(axis=0) / n
    r2bar = (post["mass"] * post["er2"])[:, 1:].sum(axis=0) / n
    assert np.allclose(out["mean_length"][1:], rbar, rtol=1e-14) and out["frames_used"] == 4
    L, tau = out["bone_lengths"], out["tau"]
    assert not out["saturated"]
    # the last coordinate step was the tau step: its equation holds at the returned values, the length equations at the tau before
    resid = skeleton_fit.tau_residual(sup, L, tau, np.concatenate([[0.0], n]), np.concatenate([[0.0], rbar]), np.concatenate([[0.0], r2bar]))
    scale = sum(n[c - 1] * skeleton_fit.tap_moments(sup, c, L[c], tau)[1] for c in (1, 2))
    assert abs(resid) <= 1e-12 * scale, (resid, scale)
    for c in (1, 2):
        Lc, clamped = skeleton_fit.solve_length(sup, c, rbar[c - 1], tau)
        assert not clamped and abs(skeleton_fit.tap_moments(sup, c, Lc, tau)[0] - rbar[c - 1]) <= 1e-12 * rbar[c - 1]
    assert len(trace) == skeleton_fit.ROUNDS * 3
    for step, before, after in trace:
        assert after >= before - 1e-12 * abs(before), (step, before, after)
    # the floor is the share of jump mass
    share = float((1.0 - post["mass"][:, 1:]).sum()) / post["mass"][:, 1:].size
    assert out["floor"] == min(max(share, 1e-6), 0.5)


# ------------------------------------------------------------------------------------------------------------------ EM
@pytest.mark.parametrize("name", ["chain16", "tree8"])
def test_em_does_not_lower_the_likelihood(name):
    k = {"chain16": chain16, "tree8": tree8}[name]()
    fit = fitted(name)
    ll = fit["log_likelihood"]
    print(name, "log-likelihood per iteration", [round(v, 6) for v in ll])
    assert len(ll) == 7 and fit["frames_used"] == k["p"].shape[0]
    slack = k["p"].shape[0] * (len(k["parents"]) - 1) * 2.0 ** -23
    for a, b in zip(ll, ll[1:]):
        assert b >= a - slack, ll
    assert ll[-1] > ll[0]
    assert sorted(fit) == sorted(skeleton_fit.FIT_KEYS)
    assert fit["history"][-1]["log_likelihood"] == ll[-1] and fit["history"][-1]["tau"] == fit["tau"]


def test_the_fitted_lengths_move_towards_the_truth():
    k = chain16()
    fit = fitted("chain16")
    before = np.abs(k["start"][1:] - k["truth"][1:]) / k["h"]
    after = np.abs(fit["bone_lengths"][1:] - k["truth"][1:]) / k["h"]
    print("length error in voxels: start", before, "fitted", after, "tau", fit["tau"] / k["h"], "floor", fit["floor"])
    assert after.mean() < before.mean()


def test_tau_stops_at_half_a_voxel():
    """At 8^3 with bones of about 2 voxels the shells collapse onto lattice distances: tau runs into its lower bound h / 2."""
    k = tree8()
    fit = fitted("tree8")
    print("tau / h", fit["tau"] / k["h"], "per edge", fit["tau_per_edge"][1:] / k["h"])
    assert fit["tau"] == k["h"] / 2 and fit["saturated"]


def test_truncation_binding_is_set_when_the_start_is_a_shell_width_off():
    k = chain16()
    start = k["truth"] + np.array([0.0, 3.0, 0.0]) * k["h"]                   # edge 1 starts 3 tau0 off, edge 2 at the truth
    fit = fit_model(k["p"], CHAIN3, k["G"], SIDE, start, k["tau"], k["floor"], iterations=3, fit_tau=False)
    print("fitted", fit["bone_lengths"] / k["h"], "binding", fit["truncation_binding"])
    assert fit["truncation_binding"][1] and not fit["truncation_binding"][0]
    assert fit["bone_lengths"][1] < start[1]


# ------------------------------------------------------------------------------------------------------------------ the surface
def test_bad_parameters_raise_before_anything_touches_a_device():
    good = dict(grid=16, cuboid_side=2.0, bone_lengths=[0.3, 0.4], tau=0.06, floor=1e-3, parents=CHAIN3)
    SkeletonModelFit(**good)
    for key, bad in [("grid", 1), ("grid", 129), ("cuboid_side", 0.0), ("bone_lengths", [0.3]), ("bone_lengths", [0.3, -0.1]),
                     ("bone_lengths", [0.3, 3.5]), ("tau", 0.0), ("tau", float("nan")), ("floor", 1.5), ("floor", -0.1),
                     ("parents", (0, 2, 1)), ("parents", (0,)), ("max_bytes", -1)]:
        with pytest.raises(ValueError):
            SkeletonModelFit(**{**good, key: bad})
    m = SkeletonModelFit(**good)
    for kw in [dict(iterations=0), dict(iterations=1.5), dict(tol=-1.0), dict(floor_bounds=(0.5, 0.1)), dict(floor_bounds=3),
               dict(tau_bounds=(0.0, 1.0)), dict(tau_bounds=(0.2, 0.1)), dict(tau_bounds=5)]:
        with pytest.raises(ValueError):
            m.fit(**kw)
    with pytest.raises(ValueError, match="nothing is stored"):
        m.fit()
    with pytest.raises(ValueError):
        m.push(np.zeros((1, 3, 16, 16, 16), dtype=np.float32))
    with pytest.raises(ValueError):
        cut_support([0.0, 0.3], 0.06, 0.125, radius=1)
    with pytest.raises(ValueError):
        edge_posteriors(np.zeros((2, 3, 3)), np.ones(2), 1e-3)
