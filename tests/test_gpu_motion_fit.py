"""GPU: the transition statistics (csrc/volume_filter.hip, se_volume_transition_stats_f32) against their float64 model
(tests/motion_fit_model.py), their bit-equality with the smoother's backward walk, their independence of how a sequence is cut into
calls, restarts, the argument gate, MotionModelFit and the command line.

Inputs: those of tests/test_gpu_volume_smoother.py (its ``filtered``: the shared sequence softmaxed on the device with the forward pass
se_volume_filter_f32 taken once); the kernel's float32 beliefs and restart flags go to the kernel and to the model alike.

TOLERANCE (derived, not measured).  Every term of every sum is non-negative, so a stat's relative error from its own roundings is at
most
    e_s = (6 R + 8 + L) 2^-24
(the tap product m' (1), three blurs of 2R + 1 fused multiply-adds (6 R + 3), the add that forms P1 and the add that forms q2 (2), keep
and floor / N as the kernel rounds them and the fused floor, or the product with b (2); the sum of chain length L = _lib.STATS_CHAIN
as the kernel's header states it), to first order in 2^-24.  On top comes the error of the incoming r_{t+1}, which the smoother's test
bounds elementwise by 2 k e1 with k the backward steps behind frame t + 1 and e1 = (6 R + 20 + L) 2^-24:
    stats[t]       |got - want| <= (e_s + 2 k_{t+1} e1) want + 2^-60     (the absolute term: float32 underflow in the tails of r)
    state          the smoother's `state`, bit for bit;   S: the smoother's `agreement`, bit for bit
    linked         exact;  unlinked frames: six NaN, r_t bit-equal to p_t
MotionModelFit: the M-step's mean_sq_step and floor are ratios of such stats, held to twice the largest stat bound of the sequence; a
log-likelihood is a sum of n ln Z terms, each within the filter's 2 k e1 (k <= T - 1 forward steps), so EM's monotone likelihood is
asserted as ll[i + 1] >= ll[i] - n 2 (T - 1) e1.
"""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD
from motion_fit_model import transition_stats_model
from sceneego_amd import _lib, motion_fit, synth
from sceneego_amd.motion_fit import MotionModelFit, m_step
from test_gpu_volume_filter import same_bits
from test_gpu_volume_smoother import filtered, forward, smooth, steps_behind
from volume_filter_cases import SIDE, coord_grid, make_logits, softmax32, taps_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
L = _lib.STATS_CHAIN

# rows, G, R, floor, T: a copy of the CASES of tests/test_gpu_volume_smoother.py
CASES = [
    (1, 8, 0, 0.0, 5),
    (1, 8, 2, 1e-3, 5),
    (15, 8, 3, 0.0, 5),
    (3, 6, 5, 1e-3, 4),          # R = G - 1: every window clipped on both sides
    (4, 10, 3, 1e-3, 5),         # G % 4 = 2, yet 1000 voxels are whole quads: the vector finish pass (scalar: test_gpu_sequence_domain.py)
    (15, 16, 5, 0.0, 5),
    (30, 16, 5, 1e-3, 3),
    (2, 24, 8, 1e-3, 4),
    (15, 64, 10, 1e-3, 3),       # the batch-1 production shape
    (1, 128, 16, 1e-3, 2),       # three planes pass the LDS of a CU: the k-blurred planes by halves of the columns
]


def e1(R):
    return (6 * R + 20 + L) * U


def e_s(R):
    return (6 * R + 8 + L) * U


def stat_bound(linked, R):
    """[T, rows]: e_s + 2 k_{t+1} e1, k the backward steps behind the frame whose r the pair reads."""
    k = steps_behind(linked)
    k_next = np.concatenate([k[1:], np.zeros_like(k[:1])])
    return e_s(R) + 2 * k_next * e1(R)


# ------------------------------------------------------------------------------------------------------------------ launch
def stats_pass(prob, belief, restarted, taps_dev, G, R, floor, cuts=None):
    """The _lib-level pass over ``prob`` [T, rows, N] in calls of ``cuts`` frames each (in frame order; issued last chunk first,
    ``state`` and ``have_link`` carried).  Host arrays: stats [T, rows, 6], linked [T, rows], state (r of frame 0), r (after every
    call: r of each chunk's first frame)."""
    T, rows, N = prob.shape
    cuts = (T,) if cuts is None else tuple(cuts)
    assert sum(cuts) == T
    state = torch.full((rows, N), float("nan"), device=DEV)
    stats = torch.full((T, rows, 6), -7.0, device=DEV)
    linked = torch.full((T, rows), -1, device=DEV, dtype=torch.int32)
    starts = np.concatenate([[0], np.cumsum(cuts)]).tolist()
    r = {}
    for i in range(len(cuts) - 1, -1, -1):
        t0, t1 = starts[i], starts[i + 1]
        link = None if t1 == T else (restarted[t1] == 0).to(torch.int32)
        _lib.volume_transition_stats(prob[t0:t1], belief[t0:t1], restarted[t0:t1], taps_dev, state, stats[t0:t1], linked[t0:t1],
                                     t1 - t0, rows, N, G, R, floor, have_link=link)
        r[t0] = state.cpu().numpy()
    torch.cuda.synchronize()
    return {"stats": stats.cpu().numpy(), "linked": linked.cpu().numpy(), "state": state.cpu().numpy(), "r": r}


def check_stats(got, want, R, label):
    """``got`` [T, rows, 6] of the kernel against the model's within the derived bound; returns the worst error in units of 2^-24."""
    lk = want["linked"]
    bound = stat_bound(lk, R)
    names = ("S", "s", "A0", "A2", "Bsum", "Rsum")
    worst = dict.fromkeys(names, 0.0)
    assert np.isnan(got[~lk]).all()
    for n, name in enumerate(names):
        g, w = got[..., n][lk].astype(np.float64), want["stats"][..., n][lk]
        err = np.abs(g - w)
        tol = bound[lk] * w + 2.0 ** -60
        worst[name] = float((err / (w + 2.0 ** -40)).max()) / U if err.size else 0.0
        assert (err <= tol).all(), f"{label}: {name} off by up to {float((err / w).max()):.3e} relative, bound {float(bound[lk].max()):.3e}"
    return worst


# ------------------------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("rows,G,R,floor,T", CASES)
def test_against_the_model_and_the_smoother(rows, G, R, floor, T):
    check_case(filtered(rows, G, R, floor, T), rows, G, R, floor, T)


def check_case(k, rows, G, R, floor, T, stats_pass=stats_pass, smooth=smooth):
    """``stats_pass``, ``smooth``: the launchers, with the signatures and the results of ``stats_pass`` above and of the smoother test's
    ``smooth`` (the defaults)."""
    N = G ** 3
    want = transition_stats_model(k["p"], k["b"], k["rs"], k["taps"], G, floor)
    lk = want["linked"]
    # the condition on the inputs, on the model: a bad seed cannot hide behind the floor
    assert lk[:-1].all() and not lk[-1].any()
    assert (want["stats"][..., 0][lk] * N >= 1e-3).all() and (want["stats"][..., 1][lk] * N >= 1e-3).all()
    got = stats_pass(k["prob"], k["belief"], k["restarted"], k["taps_dev"], G, R, floor)
    assert np.array_equal(got["linked"], lk.astype(np.int32))
    worst = check_stats(got["stats"], want, R, f"rows {rows} G {G} R {R} floor {floor}")
    if R == 0:
        assert (got["stats"][..., 3][lk] == 0).all()             # no step, no squared step
    # the backward walk is the smoother's: state and S bit for bit
    sm = smooth(k["prob"], k["belief"], k["restarted"], k["coord"], k["taps_dev"], G, R, floor, out=None)
    assert same_bits(got["state"], sm["state"])
    assert same_bits(got["stats"][..., 0], sm["agreement"])
    # the last frame is not linked: NaN stats, r_t = p_t bit for bit
    last = stats_pass(k["prob"][-1:], k["belief"][-1:], k["restarted"][-1:], k["taps_dev"], G, R, floor)
    assert np.isnan(last["stats"]).all() and (last["linked"] == 0).all() and same_bits(last["state"], k["p"][-1])
    # what the statistics are for: step + jump = 1 on every pair, from the kernel's own sums (step is a ratio of two stats, jump a
    # product of two over a third: three stat bounds, and sum r_{t+1} - 1 of a float32 softmax)
    ms = m_step(got["stats"], got["linked"], floor, G, R, SIDE / G)
    total = (ms["step"] + ms["jump"])[lk]
    assert ms["pairs"] == int(lk.sum()) and np.abs(total - 1.0).max() <= 3 * stat_bound(lk, R).max() + 1e-7
    print(f"rows {rows} G {G} R {R} floor {floor}: bound {stat_bound(lk, R).max() / U:.0f} u at frame 0; worst (units of 2^-24) "
          + ", ".join(f"{n} {v:.1f}" for n, v in worst.items()) + f"; |step + jump - 1| up to {np.abs(total - 1).max():.2e}")


@pytest.mark.parametrize("G", [116, 117])
def test_both_sides_of_the_lds_limit(G):
    """The blur pass keeps three whole planes in LDS up to G = 116 (161,472 B of dynamic LDS, the most it ever asks for) and forms the
    k-blurred planes by halves of the columns from G = 117 on, where the halves are unequal (59 and 58 columns).  The same checks as
    above, on two rows and one linked pair.  117^3 is odd and the device softmax takes whole quads, so the volumes of both are
    softmaxed on the host (volume_filter_cases.softmax32)."""
    rows, R, floor, T = 2, 6, 1e-3, 2
    N = G ** 3
    p = softmax32(make_logits(T, rows, G, R, seed=1000 * G + 10 * rows + R))
    taps = taps_for(G, R)
    k = {"p": p, "prob": torch.from_numpy(p).to(DEV), "c": coord_grid(G), "taps": taps, "taps_dev": torch.from_numpy(taps).to(DEV)}
    k["coord"] = torch.from_numpy(k["c"]).to(DEV)
    k["belief"], k["restarted"] = forward(k["prob"], k["coord"], k["taps_dev"], G, R, floor)
    k["b"], k["rs"] = k["belief"].cpu().numpy(), k["restarted"].cpu().numpy()
    assert _lib.volume_transition_stats_scratch_bytes(rows, G, R) >= 2 * rows * N * 4
    check_case(k, rows, G, R, floor, T)


def test_asymmetric_taps_are_reversed():
    """The entry point takes any taps and reverses them itself, as the smoother does."""
    rows, G, R, floor, T = 2, 8, 2, 1e-3, 4
    k = filtered(rows, G, R, floor, T)
    w = np.array([0.05, 0.10, 0.20, 0.30, 0.35], dtype=np.float64)
    taps = (w / w.sum()).astype(np.float32)
    taps_dev = torch.from_numpy(taps).to(DEV)
    belief, restarted = forward(k["prob"], k["coord"], taps_dev, G, R, floor)
    b, rs = belief.cpu().numpy(), restarted.cpu().numpy()
    got = stats_pass(k["prob"], belief, restarted, taps_dev, G, R, floor)
    want = transition_stats_model(k["p"], b, rs, taps, G, floor)
    check_stats(got["stats"], want, R, "asymmetric taps")
    sm = smooth(k["prob"], belief, restarted, k["coord"], taps_dev, G, R, floor, out=None)
    assert same_bits(got["state"], sm["state"]) and same_bits(got["stats"][..., 0], sm["agreement"])
    # ... with the taps as given (blur3 instead of its adjoint) S of this case is off by far more than the bound
    wrong = transition_stats_model(k["p"], b, rs, np.ascontiguousarray(taps[::-1]), G, floor)["stats"][:-1, :, 0]
    right = got["stats"][:-1, :, 0].astype(np.float64)
    assert (np.abs(right - wrong) / wrong).min() > 100 * stat_bound(want["linked"], R).max()


# ------------------------------------------------------------------------------------------------------------------ 2. cuts
@pytest.mark.parametrize("rows,G,R,floor,T", [c for c in CASES if c[4] == 5])
def test_results_do_not_depend_on_how_the_frames_are_cut(rows, G, R, floor, T):
    k = filtered(rows, G, R, floor, T)
    args = (k["prob"], k["belief"], k["restarted"], k["taps_dev"], G, R, floor)
    runs = [stats_pass(*args, cuts=cuts) for cuts in ((5,), (2, 3), (1, 1, 3), (5,))]
    for other in runs[1:]:
        for key in ("stats", "state"):
            assert same_bits(runs[0][key], other[key]), key
        assert np.array_equal(runs[0]["linked"], other["linked"])
    assert same_bits(runs[1]["r"][2], runs[2]["r"][2])


# ------------------------------------------------------------------------------------------------------------------ 3. restarts
def test_a_nan_stays_in_its_row():
    """The smoother's NaN test: one voxel of row 7 of frame 2 is NaN, so the filter restarts that row at frames 2 and 3."""
    rows, G, R, T, floor = 15, 16, 5, 5, 1e-3
    k = filtered(rows, G, R, floor, T)
    clean = stats_pass(k["prob"], k["belief"], k["restarted"], k["taps_dev"], G, R, floor)
    prob = k["prob"].clone()
    prob[2, 7, 1234] = float("nan")
    belief, restarted = forward(prob, k["coord"], k["taps_dev"], G, R, floor)
    assert restarted.cpu().numpy()[:, 7].tolist() == [1, 0, 1, 1, 0]
    got = stats_pass(prob, belief, restarted, k["taps_dev"], G, R, floor, cuts=(3, 2))
    want = np.ones((T, rows), dtype=np.int32)
    want[-1] = 0
    want[1, 7] = want[2, 7] = 0                                  # not linked to the restarted frames 2 and 3
    assert np.array_equal(got["linked"], want)
    assert np.isnan(got["stats"][[1, 2, 4], 7]).all() and np.isfinite(got["stats"][[0, 3], 7]).all()
    assert np.isfinite(got["state"]).all()
    sm = smooth(prob, belief, restarted, k["coord"], k["taps_dev"], G, R, floor, cuts=(3, 2), out=None)
    assert same_bits(got["state"], sm["state"]) and same_bits(got["stats"][..., 0], sm["agreement"])
    others = [r for r in range(rows) if r != 7]
    assert same_bits(got["stats"][:, others], clean["stats"][:, others]) and same_bits(got["state"][others], clean["state"][others])
    # the unlinked frames of the row hand on r_t = p_t bit for bit (frame 2: with its NaN)
    r2 = stats_pass(prob[2:], belief[2:], restarted[2:], k["taps_dev"], G, R, floor)["state"]
    assert same_bits(r2[7], prob[2, 7].cpu().numpy()) and np.isnan(r2[7]).sum() == 1
    # the M-step leaves the row's NaN pairs out
    ms = m_step(got["stats"], got["linked"], floor, G, R, SIDE / G)
    assert ms["pairs"] == int(want.sum()) and np.isfinite(ms["sigma"]) and np.isfinite(ms["floor"])


# ------------------------------------------------------------------------------------------------------------------ 4. arguments
def test_bad_arguments_raise_and_do_not_launch():
    rows, G, R, T, floor = 4, 10, 3, 5, 1e-3
    k = filtered(rows, G, R, floor, T)
    N = G ** 3
    prob, belief, restarted = k["prob"][:2].contiguous(), k["belief"][:2].clone(), k["restarted"][:2].contiguous()
    state = torch.zeros((rows, N), device=DEV)
    stats = torch.full((2, rows, 6), -7.0, device=DEV)
    linked = torch.full((2, rows), -7, device=DEV, dtype=torch.int32)

    def call(**kw):
        a = {"prob": prob, "belief": belief, "restarted": restarted, "taps": k["taps_dev"], "state": state, "stats": stats,
             "linked": linked, "frames": 2, "rows": rows, "voxels": N, "grid": G, "radius": R, "floor": floor}
        a.update(kw)
        return _lib.volume_transition_stats(**a)

    for kw in ({"radius": 17}, {"radius": -1}, {"radius": G}, {"floor": -0.1}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0},
               {"frames": 3}, {"rows": 0}, {"grid": G + 1}, {"voxels": N + 1}, {"grid": 1, "voxels": 1, "radius": 0},
               {"prob": prob.cpu()}, {"prob": prob.double()}, {"prob": prob[:, :, ::2]}, {"belief": belief[:1]}, {"belief": belief.cpu()},
               {"restarted": restarted != 0}, {"restarted": restarted[:1]}, {"taps": k["taps_dev"][:-1]}, {"taps": k["taps"]},
               {"state": torch.zeros((rows, N - 1), device=DEV)}, {"state": prob[0]}, {"state": belief[1]},
               {"stats": stats[:, :, :5]}, {"stats": stats[:1]}, {"stats": stats.double()}, {"linked": linked[:1]},
               {"linked": torch.empty((2, rows), device=DEV)},
               {"have_link": torch.ones(rows, device=DEV)}, {"have_link": torch.ones(rows + 1, device=DEV, dtype=torch.int32)},
               {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    torch.cuda.synchronize()
    assert (stats == -7).all() and (linked == -7).all() and (state == 0).all()                       # nothing was launched
    call()
    # the C entry point refuses on its own what the wrapper checks first
    lib = _lib.load()
    ws = torch.empty(_lib.volume_transition_stats_scratch_bytes(rows, G, R), device=DEV, dtype=torch.uint8)
    P = _lib._ptr
    torch.cuda.synchronize()
    stats.fill_(-7.0)

    def raw(radius=R, floor=1e-3, frames=2, grid=G, voxels=N, scratch_bytes=ws.numel(), state=state, stats=stats, rows=rows):
        return lib.se_volume_transition_stats_f32(P(prob), P(belief), P(restarted), P(k["taps_dev"]), P(state), P(stats), P(linked),
                                                  P(ws), scratch_bytes, frames, rows, voxels, grid, radius, floor, None, _lib._stream())
    assert raw(radius=17) == raw(radius=G) == raw(radius=-1) == raw(floor=2.0) == raw(floor=-0.5) == raw(floor=float("nan")) \
        == raw(frames=0) == raw(voxels=N + 4) == raw(grid=129) == raw(grid=1) == raw(rows=0) == raw(rows=65536) == -1
    assert raw(scratch_bytes=ws.numel() - 1) == -1 and raw(state=None) == -1 and raw(stats=None) == -1
    torch.cuda.synchronize()
    assert (stats == -7).all()
    assert raw() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 5. MotionModelFit
def make_fit(k, G, R, floor, **kw):
    return MotionModelFit(k["coord"], G, SIDE, sigma=R * (SIDE / G) / 3.0, radius=R, floor=floor, **kw)


def run_fit(k, G, R, floor, cuts, **kw):
    T, rows, N = k["prob"].shape
    m = make_fit(k, G, R, floor)
    t = 0
    for n in cuts:
        m.push(k["prob"][t:t + n].view(n, rows, G, G, G))
        t += n
    assert m.frames_stored == T and m.bytes_stored == 2 * T * rows * N * 4
    return m, m.fit(**kw)


@pytest.mark.parametrize("rows,G,R,T,cuts", [(15, 16, 5, 6, (2, 4)), (15, 64, 10, 3, (1, 2))])
def test_motion_model_fit(rows, G, R, T, cuts):
    floor, h = 1e-3, SIDE / G
    N = G ** 3
    k = filtered(rows, G, R, floor, T)
    sigma0 = R * h / 3.0
    # one iteration: the M-step of the model, on the kernel's own beliefs (the fit's first forward pass is this one, bit for bit)
    m, one = run_fit(k, G, R, floor, cuts, iterations=1)
    assert tuple(one) == motion_fit.FIT_KEYS and one["radius"] == R and one["pairs"] == (T - 1) * rows
    want = transition_stats_model(k["p"], k["b"], k["rs"], k["taps"], G, floor)
    ms = m_step(want["stats"], want["linked"], floor, G, R, h)
    bound = 2 * stat_bound(want["linked"], R).max()
    print(f"rows {rows} G {G} R {R} T {T}: mean_sq_step {one['mean_sq_step']:.6e} (model {ms['mean_sq_step']:.6e}), floor "
          f"{one['floor']:.6e} (model {ms['floor']:.6e}), bound {bound:.2e} relative; sigma {sigma0:.4f} -> {one['sigma']:.4f}")
    assert abs(one["mean_sq_step"] - ms["mean_sq_step"]) <= bound * ms["mean_sq_step"]
    assert abs(one["floor"] - ms["floor"]) <= bound * ms["floor"]
    assert one["history"][0]["sigma"] == sigma0 and one["history"][0]["floor"] == floor and len(one["log_likelihood"]) == 2
    assert one["history"][1]["sigma"] == one["sigma"] and one["history"][1]["floor"] == one["floor"]
    assert one["sigma_per_joint"].shape == one["floor_per_joint"].shape == (rows,)
    # four iterations: the likelihood does not fall beyond what float32 can do to n terms of ln Z
    _, four = run_fit(k, G, R, floor, cuts, iterations=4, tol=0.0)
    ll = np.array(four["log_likelihood"])
    terms = {e["terms"] for e in four["history"]}
    assert len(ll) == 5 and terms == {(T - 1) * rows}                                   # no Z restart: the same terms throughout
    slack = (T - 1) * rows * 2 * (T - 1) * e1(R)
    print(f"log-likelihood {ll.tolist()} (slack {slack:.2e}); sigma {four['sigma']:.4f} floor {four['floor']:.3e} "
          f"saturated {four['saturated']} binding {four['truncation_binding']}")
    assert (np.diff(ll) >= -slack).all() and ll[-1] > ll[0]
    assert four["log_likelihood"][:2] == one["log_likelihood"] and four["history"][1]["sigma"] == one["sigma"]
    # the result does not depend on how the frames were pushed, and a second fit() of the same object repeats it
    _, whole = run_fit(k, G, R, floor, (T,), iterations=4, tol=0.0)
    again = m.fit(iterations=4, tol=0.0)
    for other in (whole, again):
        assert other["log_likelihood"] == four["log_likelihood"] and other["sigma"] == four["sigma"] and other["floor"] == four["floor"]
        assert other["mean_sq_step"] == four["mean_sq_step"] and np.array_equal(other["sigma_per_joint"], four["sigma_per_joint"])
    # holding a parameter
    _, held = run_fit(k, G, R, floor, cuts, iterations=2, fit_sigma=False)
    assert held["sigma"] == sigma0 and held["floor"] != floor
    _, held = run_fit(k, G, R, floor, cuts, iterations=2, fit_floor=False, floor_bounds=(0.0, 1.0))
    assert held["floor"] == floor and held["sigma"] != sigma0
    m.reset()
    assert m.frames_stored == 0
    with pytest.raises(ValueError):
        m.fit()
    # the byte budget: refused with nothing allocated and nothing stored
    small = make_fit(k, G, R, floor, max_bytes=2 * 2 * rows * N * 4 - 1)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="0 frames are stored"):
        small.push(k["prob"][:2].view(2, rows, G, G, G))
    assert torch.cuda.memory_allocated() == before and small.frames_stored == 0 and small.bytes_stored == 0


# ------------------------------------------------------------------------------------------------------------------ 6. command line
def test_run_sequence_fit_frames(tmp_path, capsys):
    import run_sequence
    from sceneego_amd import load_config as load
    from sceneego_amd.jpeg_device import JpegFile
    demo_exr = os.path.join(GOLD, "demo", "img_001000.jpg.exr")
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 5, [demo_exr], estimated_depth_name="est_depth", seed=5)
    cfg_path = tmp_path / "batch2.yaml"
    with open(os.path.join(os.path.dirname(GOLD), "..", "experiments", "sceneego", "test", "sceneego.yaml")) as f:
        text = f.read()
    assert text.count("  batch_size: 8\n") == 1
    cfg_path.write_text(text.replace("  batch_size: 8\n", "  batch_size: 2\n"))
    common = ["--config", str(cfg_path), "--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth",
              "--weights", "synthetic"]
    res = run_sequence.main(common + ["--fit_frames", "4", "--fit_iterations", "2", "--fit_output", str(tmp_path / "f" / "fit.json"),
                                      "--filter_output", str(tmp_path / "f" / "filtered.pkl"),
                                      "--filter_info_output", str(tmp_path / "f" / "info.pkl")])
    out = capsys.readouterr().out
    line = [x for x in out.splitlines() if x.startswith("motion model fitted to 4 frames")]
    assert len(line) == 1 and "sigma 0.1000 -> " in line[0] and "log-likelihood" in line[0]
    with open(tmp_path / "f" / "fit.json") as f:
        fit = json.load(f)
    assert tuple(fit) == motion_fit.FIT_KEYS + ("frames", "start") and fit["frames"] == 4
    assert fit["start"] == {"sigma": 0.1, "radius": None, "floor": 1e-3} and fit["radius"] == 10
    assert 2 <= len(fit["log_likelihood"]) <= 3 and len(fit["history"]) == len(fit["log_likelihood"]) and fit["pairs"] == 3 * 15
    assert fit["log_likelihood"][-1] >= fit["log_likelihood"][0] - 45 * 2 * 3 * e1(10) and len(fit["sigma_per_joint"]) == 15
    assert res["fit"]["sigma"] == fit["sigma"] and res["fit"]["floor"] == fit["floor"]
    with open(tmp_path / "f" / "info.pkl", "rb") as f:
        info = pickle.load(f)
    with open(tmp_path / "f" / "filtered.pkl", "rb") as f:
        fitted_joints = pickle.load(f)
    assert len(info) == len(fitted_joints) == 5
    for fr in info:
        assert tuple(fr) == ("joints", "evidence", "restarted", "shift", "sigma", "radius", "floor")
        assert fr["sigma"] == fit["sigma"] and fr["floor"] == fit["floor"] and fr["radius"] == 10
    # without --fit_frames nothing changes: the bytes of --filter_output are those of the filter driven by hand on the flags' values
    run_sequence.main(common + ["--filter_output", str(tmp_path / "p" / "filtered.pkl"), "--filter_info_output", str(tmp_path / "p" / "info.pkl")])
    assert "motion model fitted" not in capsys.readouterr().out
    with open(tmp_path / "p" / "info.pkl", "rb") as f:
        assert all(tuple(fr) == ("joints", "evidence", "restarted", "shift") for fr in pickle.load(f))
    runner = run_sequence.SequenceRunner(load(str(cfg_path)), weights="synthetic")
    images, _, depths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")

    def by_hand(**model):
        vf, joints = runner.net.volume_filter(**model), []
        for i in range(0, 5, 2):
            img = runner._images([JpegFile(p) for p in images[i:i + 2]])
            depth = runner._depths(depths[i:i + 2])
            with torch.no_grad():
                kp, _, vol, _ = runner.net(img, runner.net.grid_coord_proj_batch, runner.net.coord_volumes, depth_map_batch=depth)
            joints.extend(vf.step(vol, joints=kp)["joints"].cpu().numpy())
        return joints

    def same(a, b):
        return len(a) == len(b) == 5 and all(x.dtype == np.float32 and x.shape == (15, 3) and same_bits(x, y) for x, y in zip(a, b))

    with open(tmp_path / "p" / "filtered.pkl", "rb") as f:
        plain = pickle.load(f)
    assert same(plain, by_hand(sigma=0.1, radius=None, floor=1e-3))
    assert same(fitted_joints, by_hand(sigma=fit["sigma"], radius=10, floor=fit["floor"])) and not same(fitted_joints, plain)
