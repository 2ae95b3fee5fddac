"""GPU: the grid Bayes filter (csrc/volume_filter.hip, se_volume_filter_f32) against its float64 model (tests/volume_filter_model.py),
its independence of how a sequence is cut into calls, its restarts, the public surface and the command line.

Inputs (tests/volume_filter_cases.py): logits of a bump that takes a random walk, odd rows with a second static bump, standardised to
a std of 5-10 plus 0.01 noise, softmaxed by se_softargmax3d_f32 on the device, as tests/test_gpu_joint_modes.py builds its volumes.

TOLERANCE (derived, not measured).  Every term of the recursion is non-negative, so one step's relative error is at most
    e1 = (6 R + 20 + L) 2^-24
(three blurs of 2R + 1 fused multiply-adds, the floor, the product, the sum Z of chain length L = _lib.FILTER_CHAIN as the kernel's
header states it, the division), and a non-negative linear step plus a normalisation at most doubles an incoming relative error.  With
t the index of the frame (frame 0 is the restart: a copy):
    beliefs    |got - want| <= 2 t e1 want + 2^-90      (the absolute term: float32 underflow, denormals flushed or not)
    evidence   relative 2 t e1
    joints     absolute max(2 t e1, (L + 2) 2^-24) sum b |c| per axis: the float32 summation bound of the scene-constraint test; the
               second term is the joint's own sum, which frame 0 (sum p c, no step before it) has as well
    restarted  exact
"""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD, synthetic_state_dict
from sceneego_amd import _lib, load_config, op, synth
from sceneego_amd.volume_filter import VolumeFilter, gaussian_taps
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
from volume_filter_cases import SIDE, make_logits, taps_for
from volume_filter_model import blur3, volume_filter_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
L = _lib.FILTER_CHAIN

# rows, G, R, floor, T
CASES = [
    (1, 8, 0, 0.0, 5),
    (1, 8, 2, 1e-3, 5),
    (15, 8, 3, 0.0, 5),
    (3, 6, 5, 1e-3, 4),          # R = G - 1: every window clipped on both sides
    (4, 10, 3, 1e-3, 5),         # G % 4 = 2
    (15, 16, 5, 0.0, 5),
    (30, 16, 5, 1e-3, 3),
    (2, 24, 8, 1e-3, 4),
    (15, 64, 10, 1e-3, 3),       # the batch-1 production shape
    (1, 128, 16, 1e-3, 2),
]


def e1(R):
    return (6 * R + 20 + L) * U


# ------------------------------------------------------------------------------------------------------------------ inputs, launch
@functools.lru_cache(maxsize=None)
def sequence(rows, G, R, T):
    """Softmaxed volumes [T, rows, N] on the device and on the host, computed once and shared (nothing below modifies them)."""
    N = G ** 3
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    logits = torch.from_numpy(make_logits(T, rows, G, R, seed=1000 * G + 10 * rows + R)).to(DEV).reshape(T * rows, N)
    prob = torch.empty_like(logits)
    joints = torch.empty((T * rows, 3), device=DEV, dtype=torch.float32)
    _lib.softargmax3d(logits, coord, prob, joints, T * rows, N, 1)
    torch.cuda.synchronize()
    prob = prob.view(T, rows, N)
    taps = taps_for(G, R)
    return {"prob": prob, "coord": coord, "p": prob.cpu().numpy(), "c": coord.cpu().numpy(), "taps": taps,
            "taps_dev": torch.from_numpy(taps).to(DEV)}


def launch(prob, coord, taps, G, R, floor, state=None, have_prior=None, beliefs=True):
    """One _lib-level call over all frames of ``prob`` [T, rows, N]: host arrays (belief, joints, evidence, restarted, state)."""
    T, rows, N = prob.shape
    state = torch.full((rows, N), float("nan"), device=DEV) if state is None else state.clone()
    out = torch.empty_like(prob) if beliefs else None
    joints = torch.empty((T, rows, 3), device=DEV, dtype=torch.float32)
    evidence = torch.empty((T, rows), device=DEV, dtype=torch.float32)
    restarted = torch.empty((T, rows), device=DEV, dtype=torch.int32)
    _lib.volume_filter(prob.contiguous(), coord, taps, state, out, joints, evidence, restarted, T, rows, N, G, R, floor,
                       have_prior=have_prior)
    torch.cuda.synchronize()
    return (None if out is None else out.cpu().numpy(), joints.cpu().numpy(), evidence.cpu().numpy(), restarted.cpu().numpy(),
            state.cpu().numpy())


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_filter(k, G, R, floor):
    return VolumeFilter(k["coord"], G, SIDE, sigma=R * (SIDE / G) / 3.0, radius=R, floor=floor)


def steps(f, prob, cuts, G, **kw):
    """``prob`` [T, rows, N] through ``f.step`` in calls of ``cuts`` frames each: the concatenated host results and the final state."""
    T, rows, N = prob.shape
    assert sum(cuts) == T
    parts, t = [], 0
    for n in cuts:
        parts.append(f.step(prob[t:t + n].view(n, rows, G, G, G), return_beliefs=True, **kw))
        t += n
    torch.cuda.synchronize()
    out = {key: torch.cat([p[key] for p in parts]).cpu().numpy() for key in ("beliefs", "joints", "evidence", "restarted")}
    out["state"] = f.state.cpu().numpy().copy()
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("rows,G,R,floor,T", CASES)
def test_against_the_model_over_chained_frames(rows, G, R, floor, T):
    k = sequence(rows, G, R, T)
    N = G ** 3
    wb, wj, we, wr = volume_filter_model(k["p"], k["c"], k["taps"], G, floor)
    # the condition on the inputs, on the model: a bad seed cannot hide behind the floor
    assert (we[1:] * N >= 1e-3).all(), f"evidence x N down to {np.nanmin(we[1:]) * N}"
    assert wr[0].all() and not wr[1:].any()
    gb, gj, ge, gr, gs = launch(k["prob"], k["coord"], k["taps_dev"], G, R, floor)
    assert np.array_equal(gr != 0, wr)
    assert same_bits(gb[0], k["p"][0]) and same_bits(gs, gb[-1])
    assert np.isnan(ge[0]).all()
    sabs = np.einsum("trn,na->tra", wb, np.abs(k["c"].astype(np.float64)))
    worst = {"belief": 0.0, "evidence": 0.0, "joints": 0.0}
    for t in range(T):
        bound = 2 * t * e1(R)
        err = np.abs(gb[t].astype(np.float64) - wb[t])
        tol = bound * wb[t] + 2.0 ** -90
        if t:
            worst["belief"] = max(worst["belief"], float((err / (wb[t] + 2.0 ** -60)).max()) / U)
            rel = np.abs(ge[t].astype(np.float64) - we[t]) / we[t]
            worst["evidence"] = max(worst["evidence"], float(rel.max()) / U)
        jerr = np.abs(gj[t].astype(np.float64) - wj[t])
        jtol = max(bound, (L + 2) * U) * sabs[t]
        worst["joints"] = max(worst["joints"], float((jerr / sabs[t]).max()) / U)
        print(f"rows {rows} G {G} R {R} floor {floor} frame {t}: bound {bound / U:.0f} u; worst so far (units of 2^-24) {worst}; "
              f"evidence x N min {np.nanmin(we[t]) * N if t else float('nan'):.3g}")
        assert (err <= tol).all(), f"frame {t}: belief off by up to {float((err - tol).max()):.3e} beyond the bound"
        if t:
            assert (rel <= bound).all(), f"frame {t}: evidence relative error {float(rel.max()):.3e} > {bound:.3e}"
        assert (jerr <= jtol).all(), f"frame {t}: joints off by {float((jerr / sabs[t]).max()):.3e} sum b|c|"


# ------------------------------------------------------------------------------------------------------------------ 2. chunking
@pytest.mark.parametrize("rows,G,R", [(15, 16, 5), (4, 10, 3)])
def test_results_do_not_depend_on_how_the_frames_are_cut(rows, G, R):
    T = 5
    k = sequence(rows, G, R, T)
    runs = [steps(make_filter(k, G, R, 1e-3), k["prob"], cuts, G) for cuts in ((5,), (2, 3), (1, 1, 1, 1, 1), (5,))]
    for other in runs[1:]:
        for key in ("beliefs", "joints", "evidence", "state"):
            assert same_bits(runs[0][key], other[key]), key
        assert np.array_equal(runs[0]["restarted"], other["restarted"])
    assert runs[0]["restarted"].dtype == np.bool_ and runs[0]["restarted"][0].all() and not runs[0]["restarted"][1:].any()
    # ... and the class is the _lib-level call
    gb, gj, ge, gr, gs = launch(k["prob"], k["coord"], k["taps_dev"], G, R, 1e-3)
    assert same_bits(runs[0]["beliefs"].reshape(gb.shape), gb) and same_bits(runs[0]["joints"], gj) and same_bits(runs[0]["evidence"], ge)
    assert same_bits(runs[0]["state"].reshape(gs.shape), gs)


def test_frames_seen_and_shift():
    rows, G, R, T = 4, 10, 3, 5
    k = sequence(rows, G, R, T)
    f = make_filter(k, G, R, 1e-3)
    assert f.frames_seen == 0 and f.state is None
    given = torch.zeros((2, rows, 3), device=DEV)
    r = f.step(k["prob"][:2].view(2, rows, G, G, G), joints=given)
    assert f.frames_seen == 2 and tuple(r) == ("joints", "evidence", "restarted", "shift") and tuple(r["shift"].shape) == (2, rows)
    assert torch.equal(r["shift"], r["joints"].norm(dim=-1))
    frames = op.volume_filter_to_numpy(r)
    assert len(frames) == 2 and tuple(frames[0]) == ("joints", "evidence", "restarted", "shift")
    assert frames[1]["joints"].shape == (rows, 3) and frames[1]["restarted"].dtype == np.bool_ and frames[1]["evidence"].shape == (rows,)
    f.step(k["prob"][2:3].view(1, rows, G, G, G))
    assert f.frames_seen == 3 and tuple(f.state.shape) == (rows, G, G, G)
    with pytest.raises(ValueError):
        f.step(k["prob"][:1, :2].reshape(1, 2, G, G, G))       # another number of joints than the state holds
    f.reset()
    assert f.frames_seen == 0
    r = f.step(k["prob"][3:4].view(1, rows, G, G, G))
    assert r["restarted"].all() and torch.isnan(r["evidence"]).all()


# ------------------------------------------------------------------------------------------------------------------ 3. restarts
def test_restart_where_the_prediction_has_no_mass():
    """floor = 0, R = 1: row 1 starts from a compact box, and its frame-2 volume is given exact zeros wherever blur3(b_1) > 0."""
    rows, G, R, T = 4, 10, 1, 4
    N = G ** 3
    k = sequence(rows, G, 3, 5)
    prob = k["prob"][:T].clone()
    box = torch.zeros((G, G, G), device=DEV)
    box[1:3, 1:3, 1:3] = 0.125
    prob[0, 1] = box.reshape(-1)
    prob[1, 1] = box.reshape(-1)
    taps = taps_for(G, R)
    f = VolumeFilter(k["coord"], G, SIDE, sigma=R * (SIDE / G) / 3.0, radius=R, floor=0.0)
    first = f.step(prob[:2].view(2, rows, G, G, G), return_beliefs=True)
    b1 = first["beliefs"][1, 1].reshape(1, N).cpu().numpy().astype(np.float64)
    reach = blur3(b1, taps, G)[0] > 0                          # in float64: at least where the float32 blur is positive
    assert 0 < reach.sum() < N // 2
    prob[2, 1][torch.from_numpy(reach).to(DEV)] = 0.0
    p2 = prob[2, 1].cpu().numpy()
    assert (p2 > 0).any()
    rest = f.step(prob[2:].view(T - 2, rows, G, G, G), return_beliefs=True)
    torch.cuda.synchronize()
    restarted = rest["restarted"].cpu().numpy()
    assert restarted[0].tolist() == [False, True, False, False] and not restarted[1].any()
    assert not first["restarted"][1].any() and first["restarted"][0].all()
    ev = rest["evidence"].cpu().numpy()
    assert bits(ev[0, 1:2])[0] == 0 and (ev[0, [0, 2, 3]] > 0).all()           # exactly +0
    assert same_bits(rest["beliefs"][0, 1].reshape(-1).cpu().numpy(), p2)
    want_j = (p2.astype(np.float64) @ k["c"].astype(np.float64))
    sabs = p2.astype(np.float64) @ np.abs(k["c"].astype(np.float64))
    assert (np.abs(rest["joints"][0, 1].cpu().numpy() - want_j) <= (L + 2) * U * sabs).all()
    # the frame after it is an ordinary update from b_2 = p_2
    wb, wj, we, wr = volume_filter_model(prob[3:4, 1:2].cpu().numpy(), k["c"], taps, G, 0.0, state=p2[None], have_prior=np.ones(1, bool))
    assert not wr.any() and we[0, 0] * N >= 1e-3
    got = rest["beliefs"][1, 1].reshape(-1).cpu().numpy().astype(np.float64)
    assert (np.abs(got - wb[0, 0]) <= 2 * e1(R) * wb[0, 0] + 2.0 ** -90).all()


def test_a_nan_restarts_its_own_row_twice():
    rows, G, R, T = 15, 16, 5, 5
    k = sequence(rows, G, R, T)
    clean = steps(make_filter(k, G, R, 1e-3), k["prob"], (5,), G)
    prob = k["prob"].clone()
    prob[2, 7, 1234] = float("nan")
    bad = steps(make_filter(k, G, R, 1e-3), prob, (3, 2), G)
    want = np.zeros((T, rows), dtype=bool)
    want[0] = True
    want[2, 7] = want[3, 7] = True
    assert np.array_equal(bad["restarted"], want)
    others = [r for r in range(rows) if r != 7]
    for key in ("beliefs", "joints", "evidence", "state"):
        assert same_bits(bad[key][:, others] if key != "state" else bad[key][others],
                         clean[key][:, others] if key != "state" else clean[key][others]), key
    assert same_bits(bad["beliefs"][2, 7].reshape(-1), prob[2, 7].cpu().numpy())
    assert same_bits(bad["beliefs"][3, 7].reshape(-1), k["p"][3, 7])
    assert np.isnan(bad["evidence"][2, 7]) and np.isnan(bad["evidence"][3, 7]) and np.isfinite(bad["evidence"][4, 7])
    assert np.isnan(bad["joints"][2, 7]).all() and np.isfinite(bad["joints"][3:, 7]).all()
    assert same_bits(bad["beliefs"][:2, 7], clean["beliefs"][:2, 7])


def test_reset_of_one_row():
    rows, G, R, T = 15, 16, 5, 5
    k = sequence(rows, G, R, T)
    clean = steps(make_filter(k, G, R, 1e-3), k["prob"], (5,), G)
    f = make_filter(k, G, R, 1e-3)
    a = steps(f, k["prob"][:2], (2,), G)
    f.reset(rows=[3])
    assert f.frames_seen == 2
    b = steps(f, k["prob"][2:], (1, 2), G)
    want = np.zeros((3, rows), dtype=bool)
    want[0, 3] = True
    assert np.array_equal(b["restarted"], want)
    others = [r for r in range(rows) if r != 3]
    for key in ("beliefs", "joints", "evidence"):
        assert same_bits(a[key], clean[key][:2]) and same_bits(b[key][:, others], clean[key][2:, others]), key
    assert same_bits(b["beliefs"][0, 3].reshape(-1), k["p"][2, 3]) and np.isnan(b["evidence"][0, 3])
    assert np.isfinite(b["evidence"][1:, 3]).all() and not same_bits(b["beliefs"][1, 3], clean["beliefs"][3, 3])
    with pytest.raises(ValueError):
        f.reset(rows=[rows])


def test_bad_arguments_raise_and_do_not_launch():
    rows, G, R, T = 4, 10, 3, 5
    k = sequence(rows, G, R, T)
    N = G ** 3
    prob = k["prob"][:2].contiguous()

    def call(**kw):
        a = {"prob": prob, "coord": k["coord"], "taps": k["taps_dev"], "state": torch.zeros((rows, N), device=DEV), "belief_out": None,
             "joints": torch.empty((2, rows, 3), device=DEV), "evidence": torch.empty((2, rows), device=DEV),
             "restarted": torch.empty((2, rows), device=DEV, dtype=torch.int32), "frames": 2, "rows": rows, "voxels": N, "grid": G,
             "radius": R, "floor": 1e-3}
        a.update(kw)
        return _lib.volume_filter(**a)

    call()
    both = torch.empty((3, rows, N), device=DEV)
    for kw in ({"radius": 17}, {"radius": -1}, {"radius": G}, {"floor": -0.1}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0},
               {"frames": 3}, {"rows": 0}, {"grid": G + 1}, {"voxels": N + 1}, {"grid": 1, "voxels": 1, "radius": 0},
               {"prob": prob.cpu()}, {"prob": prob.double()}, {"prob": prob[:, :, ::2]}, {"taps": k["taps_dev"][:-1]},
               {"taps": k["taps"]}, {"state": torch.zeros((rows, N - 1), device=DEV)}, {"belief_out": prob},
               {"prob": both[:2], "belief_out": both[1:]}, {"state": both[0], "belief_out": both[:2]},
               {"belief_out": torch.empty((1, rows, N), device=DEV)}, {"restarted": torch.empty((2, rows), device=DEV)},
               {"have_prior": torch.ones(rows, device=DEV)}, {"have_prior": torch.ones(rows + 1, device=DEV, dtype=torch.int32)},
               {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}, {"coord": k["coord"][:-1]}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    torch.cuda.synchronize()
    # the C entry point refuses on its own what the wrapper checks first
    lib = _lib.load()
    st = torch.zeros((rows, N), device=DEV)
    j, e, r = torch.empty((2, rows, 3), device=DEV), torch.empty((2, rows), device=DEV), torch.empty((2, rows), device=DEV, dtype=torch.int32)
    ws = torch.empty(_lib.volume_filter_scratch_bytes(rows, G, R), device=DEV, dtype=torch.uint8)
    P = _lib._ptr

    def raw(radius=R, floor=1e-3, frames=2, grid=G, voxels=N, scratch_bytes=ws.numel(), state=st):
        return lib.se_volume_filter_f32(P(prob), P(k["coord"]), P(k["taps_dev"]), P(state), None, P(j), P(e), P(r), P(ws), scratch_bytes,
                                        frames, rows, voxels, grid, radius, floor, None, _lib._stream())
    assert raw() == 0
    assert raw(radius=17) == raw(radius=G) == raw(floor=2.0) == raw(frames=0) == raw(voxels=N + 4) == raw(grid=129) == -1
    assert raw(scratch_bytes=ws.numel() - 1) == -1 and raw(state=None) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 4. public surface
@pytest.fixture(scope="module")
def net64():
    net = VoxelNetwork_depth(load_config(), device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def two_forwards(net64):
    """Two consecutive B = 2 forwards: [(joints, volumes)] cloned."""
    out = []
    for seed in (31, 32):
        img, depth = synth.make_inputs(seed, 2, "floor")
        with torch.no_grad():
            kp, _, vols, _ = net64(img.to(DEV), net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth.to(DEV))
        out.append((kp.clone(), vols.clone()))
    torch.cuda.synchronize()
    return out


def test_module_filter_equals_the_library_call(net64, two_forwards):
    G, J = net64.volume_size, 15
    assert G == 64
    N = G ** 3
    f = net64.volume_filter()
    assert isinstance(f, VolumeFilter) and f.radius == 10 and f.floor == 1e-3 and f.sigma == 0.10
    res = [f.step(vols, joints=kp, return_beliefs=True) for kp, vols in two_forwards]
    torch.cuda.synchronize()
    assert f.frames_seen == 4
    for r in res:
        assert tuple(r["joints"].shape) == (2, J, 3) and tuple(r["evidence"].shape) == (2, J) and tuple(r["beliefs"].shape) == (2, J, G, G, G)
        assert r["restarted"].dtype == torch.bool and tuple(r["shift"].shape) == (2, J)
        assert r["joints"].dtype == r["evidence"].dtype == r["beliefs"].dtype == torch.float32
    assert res[0]["restarted"][0].all() and not res[0]["restarted"][1].any() and not res[1]["restarted"].any()
    coord = net64.coord_volumes[0].reshape(N, 3).float().contiguous().to(DEV)
    vols = torch.cat([v for _, v in two_forwards]).reshape(4, J, N)
    taps = gaussian_taps(0.10, 10, net64.cuboid_side / G)
    gb, gj, ge, gr, gs = launch(vols, coord, torch.from_numpy(taps).to(DEV), G, 10, 1e-3)
    assert same_bits(torch.cat([r["beliefs"] for r in res]).reshape(4, J, N).cpu().numpy(), gb)
    assert same_bits(torch.cat([r["joints"] for r in res]).cpu().numpy(), gj)
    assert same_bits(torch.cat([r["evidence"] for r in res]).cpu().numpy(), ge)
    assert same_bits(f.state.reshape(J, N).cpu().numpy(), gs)
    kp = torch.cat([k for k, _ in two_forwards])
    shift = torch.cat([r["shift"] for r in res])
    assert torch.equal(shift, (torch.from_numpy(gj).to(DEV) - kp).norm(dim=-1))
    ev = ge[1:] * N
    print(f"synthetic weights: evidence x N {ev.min():.3g} .. {ev.max():.3g}, shift up to {float(shift.max()):.4f} m")
    assert np.isfinite(gj).all() and (ge[1:] > 0).all()

    # the beliefs are volumes: the per-frame tools take them unchanged
    b = res[0]["beliefs"]
    stats = net64.joint_statistics(b, res[0]["joints"])
    modes = net64.joint_modes(b, k=4, radius=2)
    torch.cuda.synchronize()
    assert torch.isfinite(stats["entropy"]).all() and (modes["count"] >= 1).all()
    assert torch.equal(modes["index"][..., 0], stats["peak_index"])
    # the peak of the frame-1 belief is the arg-max voxel of the model's belief (or a voxel the model holds equal to it within the
    # belief tolerance of frame 1)
    wb, _, _, _ = volume_filter_model(vols[:2].cpu().numpy(), coord.cpu().numpy(), taps, G, 1e-3)
    peak = stats["peak_index"][1].cpu().numpy()
    want = wb[1].argmax(axis=1)
    at_peak = wb[1][np.arange(J), peak]
    assert (at_peak >= wb[1].max(axis=1) * (1 - 4 * e1(10))).all()
    top2 = np.partition(wb[1], -2, axis=1)[:, -2:]
    clear = top2[:, 0] < top2[:, 1] * (1 - 4 * e1(10))          # the runner-up lies below the peak by more than both may be off
    assert clear.any() and np.array_equal(peak[clear], want[clear]), (peak, want)
    c = coord.cpu().numpy()
    assert same_bits(stats["peak_coord"][1].cpu().numpy(), c[peak])


def test_three_streams_with_the_event_chain_equal_one_stream():
    rows, G, R, T = 15, 16, 5, 5
    k = sequence(rows, G, R, T)
    one = steps(make_filter(k, G, R, 1e-3), k["prob"], (1, 1, 1, 1, 1), G)
    streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    f = make_filter(k, G, R, 1e-3)
    parts = []
    for t in range(T):                                       # no host synchronisation between the calls
        parts.append(f.step(k["prob"][t:t + 1].view(1, rows, G, G, G), return_beliefs=True, stream=streams[t % 3]))
    torch.cuda.synchronize()
    for key in ("beliefs", "joints", "evidence", "restarted"):
        got = torch.cat([p[key] for p in parts]).cpu().numpy()
        assert same_bits(got, one[key]) if key != "restarted" else np.array_equal(got, one[key]), key
    assert same_bits(f.state.cpu().numpy(), one["state"])
    # the same through torch.cuda.stream contexts, as run_sequence.py issues it
    f = make_filter(k, G, R, 1e-3)
    parts = []
    for t in range(T):
        with torch.cuda.stream(streams[(t + 1) % 3]):
            parts.append(f.step(k["prob"][t:t + 1].view(1, rows, G, G, G)))
    torch.cuda.synchronize()
    assert same_bits(torch.cat([p["joints"] for p in parts]).cpu().numpy(), one["joints"])


# ------------------------------------------------------------------------------------------------------------------ 5. command line
def test_run_sequence_filter_outputs(tmp_path, capsys):
    import evaluate
    import run_sequence
    from sceneego_amd.jpeg_device import JpegFile
    demo_exr = os.path.join(GOLD, "demo", "img_001000.jpg.exr")
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 3, [demo_exr], estimated_depth_name="est_depth", seed=5)
    cfg_path = tmp_path / "batch2.yaml"
    with open(os.path.join(os.path.dirname(GOLD), "..", "experiments", "sceneego", "test", "sceneego.yaml")) as f:
        text = f.read()
    assert text.count("  batch_size: 8\n") == 1
    cfg_path.write_text(text.replace("  batch_size: 8\n", "  batch_size: 2\n"))
    common = ["--config", str(cfg_path), "--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth",
              "--weights", "synthetic"]
    res = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl"), "--filter_output", str(tmp_path / "f" / "filtered.pkl"),
                                      "--filter_info_output", str(tmp_path / "f" / "info.pkl"), "--render_volumes", "filtered",
                                      "--render_dir", str(tmp_path / "frames"), "--render_every", "2", "--render_format", "jpg"])
    out = capsys.readouterr().out
    assert "filtered volumes" in out.splitlines()[-1]
    with open(tmp_path / "f" / "filtered.pkl", "rb") as f:
        filtered = pickle.load(f)
    with open(tmp_path / "f" / "info.pkl", "rb") as f:
        info = pickle.load(f)
    with open(tmp_path / "plain.pkl", "rb") as f:
        preds = pickle.load(f)
    assert type(filtered) is type(preds) and len(filtered) == len(preds) == len(info) == 3
    for a, b, fr in zip(filtered, preds, info):
        assert type(a) is type(b) and a.dtype == b.dtype == np.float32 and a.shape == b.shape == (15, 3) and np.isfinite(a).all()
        assert tuple(fr) == ("joints", "evidence", "restarted", "shift") and np.array_equal(fr["joints"], a)
        assert np.allclose(fr["shift"], np.linalg.norm(a.astype(np.float64) - b, axis=1), rtol=1e-5, atol=1e-7)
    assert info[0]["restarted"].all() and not info[1]["restarted"].any() and not info[2]["restarted"].any()
    assert np.isnan(info[0]["evidence"]).all() and (info[1]["evidence"] > 0).all() and (info[2]["evidence"] > 0).all()
    names = sorted(os.listdir(tmp_path / "frames"))
    assert len(names) == 8 and sum(n.endswith(".volumes.render.jpg") for n in names) == 2 \
        and sum(n.endswith(".volumes.overlay.jpg") for n in names) == 2, names
    # evaluate.py reads the filtered pickle as it reads --output
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((3, 15, 3)), f)
    ev = evaluate.main(["--pred_dir", str(tmp_path / "f" / "filtered.pkl"), "--gt", str(tmp_path / "gt.pkl")])
    capsys.readouterr()
    assert ev["frames"] == 3 and np.isfinite(ev["mpjpe"])
    assert np.isfinite(res["filtered_mpjpe"]) and len(res["filtered"]) == 3 == len(res["filter"])
    # driving VolumeFilter.step by hand on the same volumes gives the same joints, bit for bit
    from sceneego_amd import load_config as load
    runner = run_sequence.SequenceRunner(load(str(cfg_path)), weights="synthetic")
    images, _, depths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    filt = runner.net.volume_filter(sigma=0.1, radius=None, floor=1e-3)
    by_hand = []
    for i in range(0, 3, 2):
        img = runner._images([JpegFile(p) for p in images[i:i + 2]])
        depth = runner._depths(depths[i:i + 2])
        with torch.no_grad():
            kp, _, vol, _ = runner.net(img, runner.net.grid_coord_proj_batch, runner.net.coord_volumes, depth_map_batch=depth)
        by_hand.extend(filt.step(vol, joints=kp)["joints"].cpu().numpy())
    assert len(by_hand) == 3 and all(same_bits(a, b) for a, b in zip(by_hand, filtered))
