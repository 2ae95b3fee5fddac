"""CPU: the float64 model of the transition statistics (tests/motion_fit_model.py) gives the expectations over the pairwise posterior
of the hidden Markov model it claims to, the M-step solves its moment equation, EM on the model does not lower the likelihood, and the
Python surface refuses bad arguments before anything touches a device."""
import numpy as np
import pytest
import torch

from motion_fit_model import fit_model, transition_stats_model
from sceneego_amd import _lib, load_config, motion_fit
from sceneego_amd.motion_fit import MotionModelFit, m_step, solve_sigma, transition_moment
from sceneego_amd.volume_filter import gaussian_taps
from volume_filter_cases import SIDE, coord_grid, make_logits, softmax32, taps_for
from volume_filter_model import volume_filter_model
from volume_smoother_model import volume_smoother_model

# G, R, T, rows, sigma0, floor0, seed: the sequences the recursion was checked on before it was built
EM_CASES = [(8, 3, 8, 4, 0.05, 1e-3, 1), (8, 3, 8, 4, 0.6, 0.2, 2), (10, 4, 6, 3, 0.1, 1e-2, 3)]


def _stats(p, c, w, G, floor):
    """The filter's model with its beliefs rounded to float32 as the kernel hands them on, then the statistics' model and the pooled
    M-step: (belief32, restarted, stats model dict, m_step dict)."""
    b, _, _, rs = volume_filter_model(p, c, w, G, floor)
    b32 = b.astype(np.float32)
    m = transition_stats_model(p, b32, rs, w, G, floor)
    R = (len(w) - 1) // 2
    return b32, rs, m, m_step(m["stats"], m["linked"], floor, G, R, SIDE / G)


def _rows_that_sum_to_one(p):
    """``p`` [..., N] float32 with every value rounded to a multiple of 2^-20 and the largest of each row moved by the remainder, so
    that each row sums to 1 exactly.  The last frame of a track hands r = p to the pair before it, and the identities of the dense
    test hold where sum r = 1; a float32 softmax meets that only to 1e-8 (which is why step + jump = 1 is tested to 1e-7, below)."""
    q = np.round(p.astype(np.float64) * 2.0 ** 20)
    top = np.argmax(q, axis=-1)[..., None]
    np.put_along_axis(q, top, np.take_along_axis(q, top, axis=-1) + (2.0 ** 20 - q.sum(axis=-1, keepdims=True)), axis=-1)
    out = (q / 2.0 ** 20).astype(np.float32)
    assert (out.astype(np.float64).sum(axis=-1) == 1.0).all() and (out >= 0).all()
    return out


# ------------------------------------------------------------------------------------------------------------------ the claim
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("floor", [0.0, 1e-3, 0.2])
def test_the_statistics_are_expectations_over_the_dense_pairwise_posterior(R, floor):
    """G = 4: xi(x, x') = b_t(x) T(x, x') r_{t+1}(x') / S over all 64 x 64 pairs of states, with the dense transition
    T = keep W + uniform, W(x, x') = prod_axis w[x_a - x'_a] (the weight blur3 gives the move x -> x') and |x' - x|^2 from the voxel
    indices.  step, jump and sq of the model are the expectations of the step component, the jump component and the squared step;
    the marginal of xi over x' is the smoother model's gamma_t.
    Inputs: make_logits scaled by 0.3, as the smoother's dense test scales them: at G = 4 the unscaled logits (std 5 - 10 over 64
    voxels) softmax to nearly one voxel, and the expectations would test a handful of the 4096 pairs.  The rows are then made to sum
    to 1 exactly (_rows_that_sum_to_one says why)."""
    G, T, rows = 4, 4, 3
    N = G ** 3
    p = _rows_that_sum_to_one(softmax32(make_logits(T, rows, G, R, seed=21 + R) * 0.3))
    c, w = coord_grid(G), taps_for(G, R)
    b32, rs, m, ms = _stats(p, c, w, G, floor)
    gamma = volume_smoother_model(p, b32, rs, c, w, G, floor)["gamma"]
    assert not rs[1:].any() and m["linked"][:-1].all() and not m["linked"][-1].any()
    eps = float(np.float32(floor))
    keep, uniform = 1.0 - eps, eps / N
    idx = np.stack(np.unravel_index(np.arange(N), (G, G, G)), axis=1)                     # [N, 3]: (i, j, k)
    d = idx[:, None, :] - idx[None, :, :]                                                 # x - x' per axis
    w64 = w.astype(np.float64)
    W = np.where((np.abs(d) <= R).all(axis=2), np.prod(w64[np.clip(d + R, 0, 2 * R)], axis=2), 0.0)
    sqd = (d * d).sum(axis=2).astype(np.float64)
    worst = {"step": 0.0, "jump": 0.0, "sq": 0.0, "gamma": 0.0}
    for t in range(T - 1):
        for r in range(rows):
            b, rn = b32[t, r].astype(np.float64), m["r"][t + 1, r]
            xs, xj = keep * b[:, None] * W * rn[None, :], uniform * b[:, None] * rn[None, :]
            S = m["stats"][t, r, 0]                             # S = sum b_t u, the definition's normaliser
            assert abs((xs + xj).sum() / S - 1.0) <= 1e-12      # ... which is the mass of xi where sum r_{t+1} = 1
            want = {"step": xs.sum() / S, "jump": xj.sum() / S, "sq": (xs * sqd).sum() / S}
            for key in want:
                err = abs(ms[key][t, r] - want[key])
                worst[key] = max(worst[key], err / want[key] if want[key] else err)
                assert err <= 1e-10 * want[key], (key, t, r, ms[key][t, r], want[key])
            marg = (xs + xj).sum(axis=1) / S
            worst["gamma"] = max(worst["gamma"], float(np.abs(marg - gamma[t, r]).max() / gamma[t, r].max()))
            assert np.abs(marg - gamma[t, r]).max() <= 1e-12 * gamma[t, r].max()
    assert np.isnan(m["stats"][-1]).all() and np.isnan(ms["step"][-1]).all() and ms["pairs"] == (T - 1) * rows
    print(f"R {R} floor {floor}: worst relative differences " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("G,R,T,rows,sigma0,floor0,seed", EM_CASES)
def test_step_and_jump_share_the_pair(G, R, T, rows, sigma0, floor0, seed):
    """step + jump = 1 on every linked pair (to 1e-7: r is normalised in float64, the belief is the rounded float32 one)."""
    p = softmax32(make_logits(T, rows, G, R, seed))
    w = gaussian_taps(sigma0, R, SIDE / G)
    _, rs, m, ms = _stats(p, coord_grid(G), w, G, floor0)
    lk = m["linked"]
    assert lk[:-1].all() and ms["pairs"] == (T - 1) * rows
    total = ms["step"][lk] + ms["jump"][lk]
    print(f"G {G} R {R}: |step + jump - 1| up to {np.abs(total - 1).max():.2e}, jump mass {ms['jump'][lk].min():.3g} .. {ms['jump'][lk].max():.3g}")
    assert np.abs(total - 1.0).max() <= 1e-7
    assert (ms["step"][lk] >= 0).all() and (ms["jump"][lk] >= 0).all() and (ms["sq"][lk] >= 0).all()
    assert (ms["sq"][lk] <= 3 * R * R * ms["step"][lk] * (1 + 1e-12)).all()              # a step is at most R voxels per axis


# ------------------------------------------------------------------------------------------------------------------ the M-step
@pytest.mark.parametrize("R", [1, 5, 16])
def test_solve_sigma_inverts_the_moment(R):
    h = 0.03125
    worst = 0.0
    for sigma in np.linspace(0.2 * h, 0.8 * R * h, 13):
        got, saturated = solve_sigma(3.0 * transition_moment(sigma, R, h), R, h)
        worst = max(worst, abs(got - sigma) / sigma)
        assert not saturated and abs(got - sigma) <= 1e-9 * sigma, (sigma, got)
    print(f"R {R}: sigma recovered to {worst:.2e} relative")
    # M rises from 0 towards R (R + 1) / 3; at and beyond it sigma is capped and the flag raised
    moments = [transition_moment(s * h, R, h) for s in (0.1, 0.5, 1.0, 3.0, 30.0, 1e4)]
    assert all(a <= b for a, b in zip(moments, moments[1:])) and moments[-1] <= R * (R + 1) / 3.0 + 1e-12
    for m2 in (R * (R + 1), R * (R + 1) * 1.5, float("inf")):
        assert solve_sigma(m2, R, h) == (10.0 * R * h, True)
    assert solve_sigma(R * (R + 1) * (1 - 1e-3), R, h)[0] <= 10.0 * R * h
    assert solve_sigma(0.0, R, h) == (0.0, False) and solve_sigma(1.0, 0, h) == (0.0, False)
    assert transition_moment(0.0, R, h) == 0.0 and transition_moment(0.1, 0, h) == 0.0
    for bad in ((float("nan"), R, h), (1.0, -1, h), (1.0, R, 0.0)):
        with pytest.raises(ValueError):
            solve_sigma(*bad)
    with pytest.raises(ValueError):
        transition_moment(-1.0, R, h)


def test_m_step_pools_and_reports_per_joint():
    """Hand-made stats: two rows, two counted pairs each, one unlinked frame and one pair with S = 0 that must not count."""
    G, R, h, floor = 8, 3, 0.25, 0.25
    N = G ** 3
    keep, uniform = 0.75, 0.25 / N
    stats = np.full((4, 2, 6), np.nan)
    linked = np.ones((4, 2), dtype=np.int32)
    linked[3] = 0

    def pair(step, jump, m2):
        S = 2.0
        return [S, 1.0, step * S / keep, m2 * step * S / keep, jump * S / uniform, 1.0]

    stats[0, 0], stats[1, 0] = pair(0.9, 0.1, 2.0), pair(0.7, 0.3, 4.0)
    stats[0, 1], stats[1, 1] = pair(1.0, 0.0, 1.0), pair(0.5, 0.5, 1.0)
    stats[2, 0] = [0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    stats[2, 1] = [float("inf"), 1.0, 1.0, 1.0, 1.0, 1.0]
    out = m_step(stats, linked, floor, G, R, h)
    assert out["pairs"] == 4 and np.isnan(out["step"][2:]).all()
    assert abs(out["floor"] - 0.9 / 4.0) <= 1e-12
    m2 = (0.9 * 2.0 + 0.7 * 4.0 + 1.0 + 0.5) / 3.1
    assert abs(out["mean_sq_step"] - m2 * h * h) <= 1e-12 and abs(out["sigma"] - solve_sigma(m2, R, h)[0]) <= 1e-12
    assert np.allclose(out["floor_per_joint"], [0.2, 0.25], rtol=0, atol=1e-12)
    assert np.allclose(out["sigma_per_joint"], [solve_sigma(4.6 / 1.6, R, h)[0], solve_sigma(1.0, R, h)[0]], rtol=0, atol=1e-12)
    assert out["truncation_binding"] == (3 * out["sigma"] / h > R) and not out["saturated"]
    # the clamp, and a saturated moment
    assert m_step(stats, linked, floor, G, R, h, floor_bounds=(0.3, 0.5))["floor"] == 0.3
    assert m_step(stats, linked, floor, G, R, h, floor_bounds=(0.0, 0.1))["floor"] == 0.1
    stats[:2, :, 3] *= 100.0
    sat = m_step(stats, linked, floor, G, R, h)
    assert sat["saturated"] and sat["sigma"] == 10.0 * R * h and sat["truncation_binding"]
    # nothing linked: the floor stays, sigma is not a number
    none = m_step(stats, np.zeros((4, 2), dtype=np.int32), floor, G, R, h)
    assert none["pairs"] == 0 and none["floor"] == floor and np.isnan(none["sigma"]) and np.isnan(none["sigma_per_joint"]).all()
    for bad in ({"stats": stats[..., :5]}, {"linked": linked[:3]}, {"floor": 1.5}, {"floor_bounds": (0.5, 0.1)}):
        a = {"stats": stats, "linked": linked, "floor": floor, "G": G, "radius": R, "h": h}
        a.update(bad)
        with pytest.raises(ValueError):
            m_step(**a)


# ------------------------------------------------------------------------------------------------------------------ EM
@pytest.mark.parametrize("floor_bounds", [(1e-6, 0.5), (1e-2, 0.5)])
@pytest.mark.parametrize("G,R,T,rows,sigma0,floor0,seed", EM_CASES)
def test_em_does_not_lower_the_likelihood(G, R, T, rows, sigma0, floor0, seed, floor_bounds):
    """Eight iterations on the float64 models: the log-likelihood never falls by more than 1e-9 of its magnitude, with the default
    bounds and with a lower bound of 1e-2 on the floor (the clamp is a constrained maximum of a unimodal Q)."""
    p = softmax32(make_logits(T, rows, G, R, seed))
    fit = fit_model(p, coord_grid(G), G, SIDE, sigma0, R, floor0, iterations=8, tol=0.0, floor_bounds=floor_bounds)
    ll = np.array(fit["log_likelihood"])
    gains = np.diff(ll)
    print(f"G {G} R {R} from sigma {sigma0} floor {floor0}, bounds {floor_bounds}: log-likelihood {ll[0]:.6f} -> {ll[-1]:.6f}, gains "
          + " ".join(f"{g:+.2e}" for g in gains) + f"; sigma {fit['sigma']:.5f} floor {fit['floor']:.3e} saturated {fit['saturated']} "
          f"binding {fit['truncation_binding']}")
    assert len(ll) == 9 and len(fit["history"]) == 9 and not fit["converged"]
    assert len({e["terms"] for e in fit["history"]}) == 1 and fit["history"][0]["terms"] == (T - 1) * rows   # the same terms throughout
    assert (gains >= -1e-9 * np.abs(ll[:-1])).all(), gains
    assert gains[0] > 0 and ll[-1] > ll[0]
    assert floor_bounds[0] <= fit["floor"] <= floor_bounds[1] and fit["radius"] == R and fit["pairs"] == (T - 1) * rows
    assert fit["history"][-1]["sigma"] == fit["sigma"] and fit["history"][-1]["log_likelihood"] == ll[-1]
    assert fit["sigma_per_joint"].shape == fit["floor_per_joint"].shape == (rows,)
    assert tuple(k for k in motion_fit.FIT_KEYS if k not in fit) == ()


def test_holding_one_parameter_and_stopping_early():
    G, R, T, rows, sigma0, floor0, seed = EM_CASES[2]
    p, c = softmax32(make_logits(T, rows, G, R, seed)), coord_grid(G)
    a = fit_model(p, c, G, SIDE, sigma0, R, floor0, iterations=3, fit_sigma=False)
    assert a["sigma"] == sigma0 and a["floor"] != floor0 and all(e["sigma"] == sigma0 for e in a["history"]) and not a["saturated"]
    b = fit_model(p, c, G, SIDE, sigma0, R, floor0, iterations=3, fit_floor=False)
    assert b["floor"] == floor0 and b["sigma"] != sigma0 and all(e["floor"] == floor0 for e in b["history"])
    both = fit_model(p, c, G, SIDE, sigma0, R, floor0, iterations=3, fit_sigma=False, fit_floor=False)
    assert both["sigma"] == sigma0 and both["floor"] == floor0 and both["log_likelihood"][1] == both["log_likelihood"][0]
    # a loose tolerance stops at the first iteration whose relative gain is below it; the last value is under the returned values
    full = fit_model(p, c, G, SIDE, sigma0, R, floor0, iterations=8)
    ll = np.array(full["log_likelihood"])
    rel = np.diff(ll) / np.abs(ll[:-1])
    tol = float(np.sqrt(rel[1] * rel[2]))                      # between the gains of the second and the third iteration
    assert rel[0] > tol and rel[1] > tol > rel[2]
    early = fit_model(p, c, G, SIDE, sigma0, R, floor0, iterations=8, tol=tol)
    assert early["converged"] and early["log_likelihood"] == full["log_likelihood"][:4]
    assert early["sigma"] == full["history"][3]["sigma"] and early["floor"] == full["history"][3]["floor"]


def test_the_stop_rule_takes_a_change_in_either_direction():
    """em_loop over a scripted likelihood: a fall by rounding alone (below tol) is convergence, tol = 0 never stops early, and a fall
    larger than tol (the set of terms changed) does not stop the loop."""
    stats = np.array([[[2.0, 1.0, 2.0, 4.0, 64.0 * 8, 1.0]]])                            # one pair: finite S > 0
    linked = np.ones((1, 1), dtype=np.int32)

    def scripted(values):
        it = iter(values)

        def e_step(sigma, floor, want_stats):
            return np.array([[np.exp(next(it))]]), np.zeros((1, 1), dtype=np.int32), stats, linked
        return e_step

    def run(values, tol, iterations=4):
        return motion_fit.em_loop(scripted(values), 0.1, 0.25, 8, 3, 0.25, iterations, tol, True, True, (1e-6, 0.5))

    values = [-10.0, -9.0, -9.000001, -8.5, -8.4]
    a = run(values, 1e-6)
    assert a["converged"] and np.allclose(a["log_likelihood"], values[:3], rtol=0, atol=1e-12)
    b = run(values, 0.0)
    assert not b["converged"] and len(b["log_likelihood"]) == 5 and len(b["history"]) == 5
    c = run([-10.0, -12.0, -11.0, -10.9999999, -3.0], 1e-6)                              # a real fall goes on; the next standstill stops
    assert c["converged"] and len(c["log_likelihood"]) == 4
    d = run([-10.0, -9.0, -8.0, -7.0, -7.0], 1e-6)                                       # the value under the final parameters counts too
    assert d["converged"] and len(d["log_likelihood"]) == 5


def test_recovery_of_a_sampled_model_is_printed():
    """Printed, not gated: EM has local optima and no bound on the recovered values is derivable.  A path sampled from the model
    (sigma* = 0.5 voxel, floor* = 0.1) on an 8^3 grid, seen through a sharp bump of logits at the true voxel plus noise."""
    G, R, T, rows = 8, 3, 24, 4
    h = SIDE / G
    sigma_true, floor_true = 0.5 * h, 0.1
    rng = np.random.default_rng(5)
    ax = np.arange(G, dtype=np.float64)
    logits = np.empty((T, rows, G, G, G))
    for r in range(rows):
        x = rng.uniform(2, G - 3, size=3)
        for t in range(T):
            if t:
                x = rng.uniform(0, G - 1, size=3) if rng.uniform() < floor_true else np.clip(x + rng.normal(0, sigma_true / h, 3), 0, G - 1)
            g = [np.exp(-(ax - x[a]) ** 2 / (2 * 0.6 ** 2)) for a in range(3)]
            logits[t, r] = 12.0 * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :] + 0.01 * rng.standard_normal((G, G, G))
    p = softmax32(logits.reshape(T, rows, G ** 3).astype(np.float32))
    fit = fit_model(p, coord_grid(G), G, SIDE, 0.1, R, 1e-3, iterations=8)
    print(f"sampled with sigma {sigma_true:.4f} m, floor {floor_true}: fitted sigma {fit['sigma']:.4f} m, floor {fit['floor']:.4f} "
          f"(log-likelihood {fit['log_likelihood'][0]:.3f} -> {fit['log_likelihood'][-1]:.3f})")
    assert np.isfinite(fit["sigma"]) and np.isfinite(fit["floor"])


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_motion_model_fit_refuses_bad_arguments_without_a_device():
    c = coord_grid(8)
    for kw in ({"sigma": -0.1}, {"sigma": float("nan")}, {"floor": -1e-3}, {"floor": 1.5}, {"floor": float("nan")}, {"radius": -1},
               {"radius": 8}, {"radius": 17}, {"radius": 1.5}, {"max_bytes": -1}, {"max_bytes": float("nan")}):
        with pytest.raises(ValueError):
            MotionModelFit(c, 8, SIDE, **kw)
    with pytest.raises(ValueError):
        MotionModelFit(c, 129, SIDE)
    with pytest.raises(ValueError):
        MotionModelFit(c[:-1], 8, SIDE)
    m = MotionModelFit(c, 8, SIDE, sigma=0.2, max_bytes=1 << 20)
    assert m.filter.radius == 3 and m.frames_stored == 0 and m.bytes_stored == 0 and m.max_bytes == 1 << 20
    good = torch.zeros((2, 3, 8, 8, 8))
    for bad in (torch.zeros((3, 8, 8, 8)), torch.zeros((2, 3, 8, 8, 4)), torch.zeros((2, 3, 6, 6, 6)), good.double(),
                torch.zeros((0, 3, 8, 8, 8)), good.numpy()):
        with pytest.raises(ValueError):
            m.push(bad)
    for kw in ({"iterations": 0}, {"iterations": 1.5}, {"iterations": True}, {"tol": -1.0}, {"tol": float("nan")},
               {"floor_bounds": (0.5, 0.1)}, {"floor_bounds": (-0.1, 0.5)}, {"floor_bounds": (0.0, 1.5)}, {"floor_bounds": 0.1}, {}):
        with pytest.raises(ValueError):
            m.fit(**kw)                                     # a bad argument, or (the last) nothing stored
    with pytest.raises(ValueError, match="fit: nothing is stored"):
        m.fit()
    assert "finish" not in MotionModelFit._budget_advice
    m.reset()
    with pytest.raises(_lib.HipExtensionError):             # a well-formed call gets as far as the device check: there is no CPU path
        m.push(good)
    assert m.frames_stored == 0


def test_the_network_entry_point_validates_on_the_host():
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    cfg = load_config()
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    m = net.motion_fit()
    assert isinstance(m, MotionModelFit) and m.filter.grid == net.volume_size and m.filter.radius == 10 and m.filter.floor == 1e-3
    assert m.max_bytes is None and net.motion_fit(max_bytes=123).max_bytes == 123 and net.motion_fit(sigma=0.05, radius=4).filter.radius == 4
    with pytest.raises(ValueError):
        net.motion_fit(sigma=-1.0)
    cfg.model.volume_softmax = False
    with pytest.raises(ValueError):
        VoxelNetwork_depth(cfg, device="cpu", verbose=False).motion_fit()


def test_binding_lists_the_transition_statistics():
    assert _lib.ABI_VERSION >= 38
    assert "se_volume_transition_stats_f32" in _lib.SIGNATURES and "se_volume_transition_stats_scratch_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["se_volume_transition_stats_f32"][1]) == 17
    lib = _lib.load()
    assert lib.se_volume_transition_stats_scratch_bytes(15, 64, 10) >= 15 * (2 * 64 ** 3 + 8 * 64) * 4
    assert lib.se_volume_transition_stats_scratch_bytes(15, 64, 17) == 0 and lib.se_volume_transition_stats_scratch_bytes(3, 6, 6) == 0
    assert lib.se_volume_transition_stats_scratch_bytes(0, 64, 10) == 0 and lib.se_volume_transition_stats_scratch_bytes(1, 128, 16) > 0
    assert _lib.STATS_CHAIN <= 512 and _lib.STATS_SLOTS == 6        # the GPU test's tolerance is built on the chain
    with pytest.raises(_lib.HipExtensionError):                     # CPU tensors: refused before anything is launched
        z = torch.zeros((1, 1, 8))
        _lib.volume_transition_stats(z, z, torch.zeros((1, 1), dtype=torch.int32), torch.ones(1), torch.zeros((1, 8)),
                                     torch.zeros((1, 1, 6)), torch.zeros((1, 1), dtype=torch.int32), 1, 1, 8, 2, 0, 0.0)


def test_motion_fit_to_json_is_plain():
    import json
    from sceneego_amd import op
    G, R, T, rows, sigma0, floor0, seed = EM_CASES[2]
    fit = fit_model(softmax32(make_logits(T, rows, G, R, seed)), coord_grid(G), G, SIDE, sigma0, R, floor0, iterations=1)
    fit["sigma_per_joint"][0] = np.nan
    out = json.loads(json.dumps(op.motion_fit_to_json(fit, frames=T)))
    assert tuple(out) == motion_fit.FIT_KEYS + ("frames",) and out["frames"] == T and out["sigma_per_joint"][0] is None
    assert out["sigma"] == fit["sigma"] and out["log_likelihood"] == fit["log_likelihood"] and len(out["history"]) == 2


def test_run_sequence_parser_takes_the_fit_flags():
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    a = run_sequence.parse_args(base)
    assert a.fit is None and a.fit_output is None
    a = run_sequence.parse_args(base + ["--fit_frames", "16", "--filter_output", "f.pkl"])
    assert a.fit == {"frames": 16, "iterations": 8} and a.filter == {"sigma": 0.1, "radius": None, "floor": 1e-3}
    a = run_sequence.parse_args(base + ["--fit_frames", "16", "--fit_iterations", "3", "--fit_output", "fit.json"])
    assert a.fit == {"frames": 16, "iterations": 3} and a.fit_output == "fit.json" and a.filter is None
    for bad in (["--fit_frames", "1"], ["--fit_frames", "8", "--fit_iterations", "0"], ["--fit_iterations", "3"], ["--fit_output", "f.json"]):
        with pytest.raises(SystemExit):
            run_sequence.parse_args(base + bad)
