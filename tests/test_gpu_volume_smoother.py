"""GPU: the filter's backward pass (csrc/volume_filter.hip, se_volume_smooth_f32) against its float64 model
(tests/volume_smoother_model.py), its independence of how a sequence is cut into calls, in-place output, restarts, the public surface
and the command line.

Inputs: those of tests/test_gpu_volume_filter.py (``sequence``: make_logits with seed 1000 G + 10 rows + R, softmaxed by
se_softargmax3d_f32 on the device).  The forward pass is se_volume_filter_f32 on the device; its float32 beliefs and restart flags go to
the kernel and to the model alike, so the model's input is the kernel's input.

TOLERANCE (derived, not measured).  Every term of the backward recursion is non-negative, so one step's relative error is at most
    e1 = (6 R + 20 + L) 2^-24
(three blurs of 2R + 1 fused multiply-adds, the floor, the product, the sum of chain length L = _lib.SMOOTH_CHAIN as the kernel's header
states it, the division): the filter's figure, because the step is the filter's with other taps, and the second product g = b u shares
u with the first.  A non-negative linear step plus a normalisation at most doubles an incoming relative error.  With k the number of
backward steps behind frame t since the chain's last cut (k = 0: the frame is not linked; its outputs are copies):
    gamma_t, r_t   |got - want| <= 2 k e1 want + 2^-90      (the absolute term: float32 underflow, denormals flushed or not)
    agreement      relative 2 k e1
    joints         absolute max(2 k e1, (L + 2) 2^-24) sum gamma |c| per axis: the float32 summation bound of the filter's test; the
                   second term is the joint's own sum, which a k = 0 frame (sum b c, no step behind it) has as well
    flags          exact;  k = 0 frames: gamma_t bit-equal to b_t and r_t to p_t
"""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD
from sceneego_amd import _lib, op, synth
from sceneego_amd.volume_filter import gaussian_taps
from sceneego_amd.volume_smoother import VolumeSmoother
from test_gpu_volume_filter import bits, net64, same_bits, sequence, two_forwards  # noqa: F401  (the two fixtures)
from volume_filter_cases import SIDE
from volume_smoother_model import volume_smoother_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
L = _lib.SMOOTH_CHAIN

# rows, G, R, floor, T
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
    (1, 128, 16, 1e-3, 2),
]


def e1(R):
    return (6 * R + 20 + L) * U


# ------------------------------------------------------------------------------------------------------------------ inputs, launch
def forward(prob, coord, taps_dev, G, R, floor):
    """se_volume_filter_f32 over ``prob`` [T, rows, N] on the device: (beliefs [T, rows, N], restarted [T, rows] int32), device tensors."""
    T, rows, N = prob.shape
    state = torch.full((rows, N), float("nan"), device=DEV)
    beliefs = torch.empty_like(prob)
    joints = torch.empty((T, rows, 3), device=DEV)
    evidence = torch.empty((T, rows), device=DEV)
    restarted = torch.empty((T, rows), device=DEV, dtype=torch.int32)
    _lib.volume_filter(prob.contiguous(), coord, taps_dev, state, beliefs, joints, evidence, restarted, T, rows, N, G, R, floor)
    torch.cuda.synchronize()
    return beliefs, restarted


@functools.lru_cache(maxsize=None)
def filtered(rows, G, R, floor, T):
    """The shared sequence with the forward pass taken once (nothing below modifies it)."""
    k = dict(sequence(rows, G, R, T))
    k["belief"], k["restarted"] = forward(k["prob"], k["coord"], k["taps_dev"], G, R, floor)
    k["b"], k["rs"] = k["belief"].cpu().numpy(), k["restarted"].cpu().numpy()
    return k


def smooth(prob, belief, restarted, coord, taps_dev, G, R, floor, cuts=None, out="new"):
    """The _lib-level backward pass over ``prob`` [T, rows, N] in calls of ``cuts`` frames each (in frame order; issued last chunk
    first, ``state`` and ``have_link`` carried).  ``out``: "new", "inplace" (over a clone of ``belief``) or None.  Host arrays: gamma
    (None without ``out``), joints, agreement, smoothed, state (r of frame 0), r (after every call: r of each chunk's first frame)."""
    T, rows, N = prob.shape
    cuts = (T,) if cuts is None else tuple(cuts)
    assert sum(cuts) == T
    belief = belief.clone() if out == "inplace" else belief
    gamma = belief if out == "inplace" else torch.empty_like(prob) if out == "new" else None
    state = torch.full((rows, N), float("nan"), device=DEV)
    joints = torch.empty((T, rows, 3), device=DEV)
    agreement = torch.empty((T, rows), device=DEV)
    smoothed = torch.full((T, rows), -1, device=DEV, dtype=torch.int32)
    starts = np.concatenate([[0], np.cumsum(cuts)]).tolist()
    r = {}
    for i in range(len(cuts) - 1, -1, -1):
        t0, t1 = starts[i], starts[i + 1]
        link = None if t1 == T else (restarted[t1] == 0).to(torch.int32)
        _lib.volume_smooth(prob[t0:t1], belief[t0:t1], restarted[t0:t1], coord, taps_dev, state, None if gamma is None else gamma[t0:t1],
                           joints[t0:t1], agreement[t0:t1], smoothed[t0:t1], t1 - t0, rows, N, G, R, floor, have_link=link)
        r[t0] = state.cpu().numpy()
    torch.cuda.synchronize()
    return {"gamma": None if gamma is None else gamma.cpu().numpy(), "joints": joints.cpu().numpy(), "agreement": agreement.cpu().numpy(),
            "smoothed": smoothed.cpu().numpy(), "state": state.cpu().numpy(), "r": r}


def steps_behind(linked):
    """k [T, rows]: backward steps behind each frame since the chain's last cut (0 where the frame is not linked)."""
    k = np.zeros(linked.shape, dtype=np.int64)
    for t in range(linked.shape[0] - 2, -1, -1):
        k[t] = np.where(linked[t], k[t + 1] + 1, 0)
    return k


def check_against_model(k, G, R, floor, taps, taps_dev, label, smooth=smooth):
    """``smooth``: the launcher, with the signature and the result of ``smooth`` above (the default)."""
    T, rows, N = k["p"].shape
    belief, restarted = (k["belief"], k["restarted"]) if taps is k["taps"] else forward(k["prob"], k["coord"], taps_dev, G, R, floor)
    b, rs = belief.cpu().numpy(), restarted.cpu().numpy()
    want = volume_smoother_model(k["p"], b, rs, k["c"], taps, G, floor)
    # the condition on the inputs, on the model: a bad seed cannot hide behind the floor
    lk = want["linked"]
    assert lk[:-1].all() and not lk[-1].any() and want["smoothed"][:-1].all()
    assert (want["agreement"][lk] * N >= 1e-3).all() and (want["s"][lk] * N >= 1e-3).all(), \
        f"agreement x N down to {want['agreement'][lk].min() * N}, s x N down to {want['s'][lk].min() * N}"
    one = smooth(k["prob"], belief, restarted, k["coord"], taps_dev, G, R, floor, cuts=(1,) * T)    # frame by frame: r_t of every frame
    whole = smooth(k["prob"], belief, restarted, k["coord"], taps_dev, G, R, floor)
    for key in ("gamma", "joints", "agreement", "state"):
        assert same_bits(one[key], whole[key]), key
    assert np.array_equal(one["smoothed"], whole["smoothed"]) and np.array_equal(one["smoothed"] != 0, want["smoothed"])
    assert set(np.unique(one["smoothed"])) <= {0, 1}
    steps = steps_behind(lk)
    sabs = np.einsum("trn,na->tra", want["gamma"], np.abs(k["c"].astype(np.float64)))
    worst = {"gamma": 0.0, "r": 0.0, "agreement": 0.0, "joints": 0.0}
    for t in range(T):
        kk = steps[t]                                           # [rows]
        bound = 2 * kk * e1(R)
        got_g, got_r = one["gamma"][t].astype(np.float64), one["r"][t].astype(np.float64)
        for name, got, ref, copy_of in (("gamma", got_g, want["gamma"][t], b[t]), ("r", got_r, want["r"][t], k["p"][t])):
            err = np.abs(got - ref)
            tol = bound[:, None] * ref + 2.0 ** -90
            worst[name] = max(worst[name], float((err / (ref + 2.0 ** -60)).max()) / U)
            assert (err <= tol).all(), f"{label} frame {t}: {name} off by up to {float((err - tol).max()):.3e} beyond the bound"
            cut = kk == 0
            assert same_bits((one["gamma"][t] if name == "gamma" else one["r"][t])[cut], copy_of[cut]), f"frame {t}: {name} is not the copy"
        linked = kk > 0
        assert np.isnan(one["agreement"][t][~linked]).all()
        if linked.any():
            rel = np.abs(one["agreement"][t][linked].astype(np.float64) - want["agreement"][t][linked]) / want["agreement"][t][linked]
            worst["agreement"] = max(worst["agreement"], float(rel.max()) / U)
            assert (rel <= bound[linked]).all(), f"{label} frame {t}: agreement relative error {float(rel.max()):.3e}"
        jerr = np.abs(one["joints"][t].astype(np.float64) - want["joints"][t])
        jtol = np.maximum(bound, (L + 2) * U)[:, None] * sabs[t]
        worst["joints"] = max(worst["joints"], float((jerr / sabs[t]).max()) / U)
        assert (jerr <= jtol).all(), f"{label} frame {t}: joints off by {float((jerr / sabs[t]).max()):.3e} sum gamma|c|"
    amin, smin = want["agreement"][lk].min() * N, want["s"][lk].min() * N
    print(f"{label}: bound {2 * (T - 1) * e1(R) / U:.0f} u at frame 0; worst (units of 2^-24) "
          + ", ".join(f"{n} {v:.1f}" for n, v in worst.items()) + f"; agreement x N min {amin:.3g}, s x N min {smin:.3g}")


# ------------------------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("rows,G,R,floor,T", CASES)
def test_against_the_model_over_chained_frames(rows, G, R, floor, T):
    k = filtered(rows, G, R, floor, T)
    check_against_model(k, G, R, floor, k["taps"], k["taps_dev"], f"rows {rows} G {G} R {R} floor {floor}")


def test_against_the_model_with_asymmetric_taps():
    """The C entry point takes any taps and must reverse them: with the taps as given (blur3 instead of its adjoint) the agreement of this
    case differs from the model's by far more than the bound (checked on the model itself below)."""
    rows, G, R, floor, T = 2, 8, 2, 1e-3, 4
    k = filtered(rows, G, R, floor, T)
    w = np.array([0.05, 0.10, 0.20, 0.30, 0.35], dtype=np.float64)
    taps = (w / w.sum()).astype(np.float32)
    check_against_model(k, G, R, floor, taps, torch.from_numpy(taps).to(DEV), "asymmetric taps, G 8 R 2")
    belief, restarted = forward(k["prob"], k["coord"], torch.from_numpy(taps).to(DEV), G, R, floor)
    b, rs = belief.cpu().numpy(), restarted.cpu().numpy()
    right = volume_smoother_model(k["p"], b, rs, k["c"], taps, G, floor)
    wrong = volume_smoother_model(k["p"], b, rs, k["c"], np.ascontiguousarray(taps[::-1]), G, floor)
    rel = np.abs(right["agreement"][:-1] - wrong["agreement"][:-1]) / right["agreement"][:-1]
    assert rel.min() > 100 * 2 * (T - 1) * e1(R), rel.min()


# ------------------------------------------------------------------------------------------------------------------ 2. cuts, in place
def make_smoother(k, G, R, floor, **kw):
    return VolumeSmoother(k["coord"], G, SIDE, sigma=R * (SIDE / G) / 3.0, radius=R, floor=floor, **kw)


def pushes(s, prob, cuts, G, return_beliefs=True, streams=None, **kw):
    T, rows, N = prob.shape
    assert sum(cuts) == T
    live, t = [], 0
    for i, n in enumerate(cuts):
        extra = {} if streams is None else {"stream": streams[i % len(streams)]}
        live.append(s.push(prob[t:t + n].view(n, rows, G, G, G), **extra, **kw))
        t += n
    res = s.finish(return_beliefs=return_beliefs)
    torch.cuda.synchronize()
    out = {key: res[key].cpu().numpy() for key in res if key != "beliefs"}
    if return_beliefs:
        assert [int(x.shape[0]) for x in res["beliefs"]] == list(cuts)
        out["beliefs"] = torch.cat(res["beliefs"]).reshape(T, rows, N).cpu().numpy()
    out["live"] = live
    return out


@pytest.mark.parametrize("rows,G,R", [(15, 16, 5), (4, 10, 3)])
def test_results_do_not_depend_on_how_the_frames_are_cut(rows, G, R):
    T, floor = 5, 1e-3
    k = filtered(rows, G, R, floor, T)
    runs = [pushes(make_smoother(k, G, R, floor), k["prob"], cuts, G) for cuts in ((5,), (2, 3), (1, 1, 1, 1, 1), (5,))]
    keys = ("joints", "agreement", "filtered_joints", "shift_filtered", "beliefs")
    for other in runs[1:]:
        for key in keys:
            assert same_bits(runs[0][key], other[key]), key
        assert np.array_equal(runs[0]["smoothed"], other["smoothed"])
    assert runs[0]["smoothed"].dtype == np.bool_ and runs[0]["smoothed"][:-1].all() and not runs[0]["smoothed"][-1].any()
    assert "shift" not in runs[0]
    # ... across _lib-level chunkings with state and have_link carried, and the class is the _lib-level call
    args = (k["prob"], k["belief"], k["restarted"], k["coord"], k["taps_dev"], G, R, floor)
    lib = [smooth(*args, cuts=cuts) for cuts in ((5,), (2, 3), (3, 2), (1, 1, 1, 1, 1))]
    for other in lib[1:]:
        for key in ("gamma", "joints", "agreement", "state"):
            assert same_bits(lib[0][key], other[key]), key
        assert np.array_equal(lib[0]["smoothed"], other["smoothed"])
    # (where a frame is not smoothed the class hands on the filter's own joint, bit for bit, instead of the kernel's sum b c)
    assert same_bits(runs[0]["beliefs"], lib[0]["gamma"]) and same_bits(runs[0]["joints"][:-1], lib[0]["joints"][:-1])
    assert same_bits(runs[0]["agreement"], lib[0]["agreement"]) and np.array_equal(runs[0]["smoothed"], lib[0]["smoothed"] != 0)
    # the last frame is the filtered belief, and push returned the filter's own result
    assert same_bits(runs[0]["beliefs"][-1], k["b"][-1]) and same_bits(runs[0]["joints"][-1], runs[0]["filtered_joints"][-1])
    assert (runs[0]["shift_filtered"][-1] == 0).all()
    live = torch.cat([x["beliefs"] for x in runs[1]["live"]]).reshape(T, rows, -1).cpu().numpy()
    assert same_bits(live, k["b"])                              # finish() wrote over the smoother's copies, not over what push returned


@pytest.mark.parametrize("rows,G,R", [(15, 16, 5), (4, 10, 3)])
def test_in_place_and_without_beliefs(rows, G, R):
    T, floor = 5, 1e-3
    k = filtered(rows, G, R, floor, T)
    args = (k["prob"], k["belief"], k["restarted"], k["coord"], k["taps_dev"], G, R, floor)
    new, inplace, none = smooth(*args), smooth(*args, cuts=(2, 3), out="inplace"), smooth(*args, out=None)
    assert same_bits(inplace["gamma"], new["gamma"]) and same_bits(k["belief"].cpu().numpy(), k["b"])
    for other in (inplace, none):
        for key in ("joints", "agreement", "state"):
            assert same_bits(new[key], other[key]), key
        assert np.array_equal(new["smoothed"], other["smoothed"])
    assert none["gamma"] is None
    a = pushes(make_smoother(k, G, R, floor), k["prob"], (2, 3), G, return_beliefs=False)
    assert "beliefs" not in a and same_bits(a["joints"][:-1], new["joints"][:-1]) and same_bits(a["agreement"], new["agreement"])
    assert same_bits(a["joints"][-1], a["filtered_joints"][-1])


def test_storage_shift_and_reset():
    rows, G, R, T, floor = 4, 10, 3, 5, 1e-3
    k = filtered(rows, G, R, floor, T)
    N = G ** 3
    s = make_smoother(k, G, R, floor, max_bytes=2 * 3 * rows * N * 4)
    given = torch.zeros((2, rows, 3), device=DEV)
    r = s.push(k["prob"][:2].view(2, rows, G, G, G), joints=given)
    assert tuple(r) == ("joints", "evidence", "restarted", "beliefs", "shift")
    assert s.frames_stored == 2 and s.bytes_stored == 2 * 2 * rows * N * 4 and s.filter.frames_seen == 2
    with pytest.raises(ValueError, match="2 frames are stored"):
        s.push(k["prob"][2:4].view(2, rows, G, G, G))          # 4 frames would exceed max_bytes: nothing stepped, nothing stored
    assert s.frames_stored == 2 and s.filter.frames_seen == 2
    s.push(k["prob"][2:3].view(1, rows, G, G, G))
    res = s.finish()
    assert tuple(res) == ("joints", "smoothed", "agreement", "filtered_joints", "shift_filtered", "shift")
    assert tuple(res["shift"].shape) == (3, rows) and torch.equal(res["shift"][:2], res["joints"][:2].norm(dim=-1))
    assert torch.isnan(res["shift"][2]).all() and s.frames_stored == 0
    frames = op.volume_smoother_to_numpy(res)
    assert len(frames) == 3 and tuple(frames[0]) == ("joints", "smoothed", "agreement", "filtered_joints", "shift_filtered", "shift")
    assert frames[1]["joints"].shape == (rows, 3) and frames[1]["smoothed"].dtype == np.bool_ and frames[1]["agreement"].shape == (rows,)
    with pytest.raises(ValueError):
        s.finish()
    s.reset()
    assert s.filter.frames_seen == 0
    assert s.push(k["prob"][:1].view(1, rows, G, G, G))["restarted"].all()


# ------------------------------------------------------------------------------------------------------------------ 3. restarts
def test_a_forward_restart_cuts_the_chain_both_ways():
    """The filter test's box construction: floor = 0, R = 1, row 1 starts from a compact box and its frame-2 volume is given exact zeros
    wherever blur3(b_1) > 0, so the filter restarts the row at frame 2."""
    from volume_filter_cases import taps_for
    from volume_filter_model import blur3
    rows, G, R, T = 4, 10, 1, 4
    N = G ** 3
    k = sequence(rows, G, 3, 5)
    prob = k["prob"][:T].clone()
    box = torch.zeros((G, G, G), device=DEV)
    box[1:3, 1:3, 1:3] = 0.125
    prob[0, 1] = box.reshape(-1)
    prob[1, 1] = box.reshape(-1)
    taps = taps_for(G, R)
    taps_dev = torch.from_numpy(taps).to(DEV)
    b1 = forward(prob[:2], k["coord"], taps_dev, G, R, 0.0)[0][1, 1].reshape(1, N).cpu().numpy().astype(np.float64)
    reach = blur3(b1, taps, G)[0] > 0
    assert 0 < reach.sum() < N // 2
    clean_belief, clean_rs = forward(prob, k["coord"], taps_dev, G, R, 0.0)
    assert clean_rs.cpu().numpy()[1:].sum() == 0
    clean = smooth(prob, clean_belief, clean_rs, k["coord"], taps_dev, G, R, 0.0)
    cut = prob.clone()
    cut[2, 1][torch.from_numpy(reach).to(DEV)] = 0.0
    belief, restarted = forward(cut, k["coord"], taps_dev, G, R, 0.0)
    rs = restarted.cpu().numpy()
    assert rs[1:].tolist() == [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    got = smooth(cut, belief, restarted, k["coord"], taps_dev, G, R, 0.0, cuts=(2, 2))
    p, b = cut.cpu().numpy(), belief.cpu().numpy()
    want = volume_smoother_model(p, b, rs, k["c"], taps, G, 0.0)
    assert want["smoothed"].tolist() == [[True] * 4, [True, False, True, True], [True] * 4, [False] * 4]
    assert np.array_equal(got["smoothed"] != 0, want["smoothed"])
    # frame 1 of row 1 is not linked to the restarted frame 2: copies, bit for bit, and frame 0 is smoothed over frames 0..1 alone
    assert same_bits(got["gamma"][1, 1], b[1, 1]) and np.isnan(got["agreement"][1, 1])
    head = smooth(cut[:2], belief[:2], restarted[:2], k["coord"], taps_dev, G, R, 0.0)
    assert same_bits(got["gamma"][:2, 1], head["gamma"][:, 1]) and same_bits(got["joints"][:2, 1], head["joints"][:, 1])
    assert same_bits(got["state"][1], head["state"][1])
    # behind the cut the row is smoothed as usual
    assert (np.abs(got["gamma"][2, 1] - want["gamma"][2, 1]) <= 2 * e1(R) * want["gamma"][2, 1] + 2.0 ** -90).all()
    # untouched rows: bit-equal to the clean run
    others = [0, 2, 3]
    for key in ("gamma", "joints", "agreement"):
        assert same_bits(got[key][:, others], clean[key][:, others]), key
    assert same_bits(got["state"][others], clean["state"][others])


def test_a_nan_stays_in_its_frame():
    rows, G, R, T, floor = 15, 16, 5, 5, 1e-3
    k = filtered(rows, G, R, floor, T)
    clean = smooth(k["prob"], k["belief"], k["restarted"], k["coord"], k["taps_dev"], G, R, floor)
    prob = k["prob"].clone()
    prob[2, 7, 1234] = float("nan")
    belief, restarted = forward(prob, k["coord"], k["taps_dev"], G, R, floor)
    rs = restarted.cpu().numpy()
    assert rs[:, 7].tolist() == [1, 0, 1, 1, 0]
    got = smooth(prob, belief, restarted, k["coord"], k["taps_dev"], G, R, floor, cuts=(3, 2))
    want = np.ones((T, rows), dtype=bool)
    want[-1] = False
    want[1, 7] = want[2, 7] = False                              # not linked to the restarted frames 2 and 3
    assert np.array_equal(got["smoothed"] != 0, want)
    b, p = belief.cpu().numpy(), prob.cpu().numpy()
    assert same_bits(got["gamma"][2, 7], b[2, 7]) and same_bits(got["gamma"][2, 7], p[2, 7]) and np.isnan(got["gamma"][2, 7]).sum() == 1
    assert same_bits(got["gamma"][1, 7], b[1, 7]) and np.isnan(got["joints"][2, 7]).all()
    assert np.isnan(got["agreement"][[1, 2, 4], 7]).all() and np.isfinite(got["agreement"][[0, 3], 7]).all()
    for t in (0, 1, 3, 4):
        assert np.isfinite(got["gamma"][t, 7]).all() and np.isfinite(got["joints"][t, 7]).all()
    assert np.isfinite(got["state"]).all()
    others = [r for r in range(rows) if r != 7]
    for key in ("gamma", "joints", "agreement"):
        assert same_bits(got[key][:, others], clean[key][:, others]), key
    assert same_bits(got["state"][others], clean["state"][others])
    # a NaN handed over in the state: both fallbacks, decided for the one row
    state_link = smooth(prob[3:], belief[3:], restarted[3:], k["coord"], k["taps_dev"], G, R, floor)["state"]
    bad = torch.from_numpy(state_link).to(DEV)
    bad[3, 99] = float("nan")
    joints, agreement = torch.empty((1, rows, 3), device=DEV), torch.empty((1, rows), device=DEV)
    flag = torch.empty((1, rows), device=DEV, dtype=torch.int32)
    gamma = torch.empty_like(prob[2:3])
    _lib.volume_smooth(k["prob"][2:3], k["belief"][2:3], k["restarted"][2:3], k["coord"], k["taps_dev"], bad, gamma, joints, agreement, flag,
                       1, rows, G ** 3, G, R, floor, have_link=torch.ones(rows, device=DEV, dtype=torch.int32))
    torch.cuda.synchronize()
    assert flag[0].cpu().tolist() == [int(r != 3) for r in range(rows)] and bool(torch.isnan(agreement[0, 3]))
    assert same_bits(gamma[0, 3].cpu().numpy(), k["b"][2, 3]) and same_bits(bad[3].cpu().numpy(), k["p"][2, 3])


# ------------------------------------------------------------------------------------------------------------------ 4. arguments
def test_bad_arguments_raise_and_do_not_launch():
    rows, G, R, T, floor = 4, 10, 3, 5, 1e-3
    k = filtered(rows, G, R, floor, T)
    N = G ** 3
    prob, belief, restarted = k["prob"][:2].contiguous(), k["belief"][:2].clone(), k["restarted"][:2].contiguous()
    state = torch.zeros((rows, N), device=DEV)
    joints, agreement = torch.full((2, rows, 3), -7.0, device=DEV), torch.full((2, rows), -7.0, device=DEV)
    flag = torch.full((2, rows), -7, device=DEV, dtype=torch.int32)

    def call(**kw):
        a = {"prob": prob, "belief": belief, "restarted": restarted, "coord": k["coord"], "taps": k["taps_dev"], "state": state,
             "smoothed_out": None, "joints": joints, "agreement": agreement, "smoothed": flag, "frames": 2, "rows": rows, "voxels": N,
             "grid": G, "radius": R, "floor": floor}
        a.update(kw)
        return _lib.volume_smooth(**a)

    both = torch.empty((3, rows, N), device=DEV)
    for kw in ({"radius": 17}, {"radius": -1}, {"radius": G}, {"floor": -0.1}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0},
               {"frames": 3}, {"rows": 0}, {"grid": G + 1}, {"voxels": N + 1}, {"grid": 1, "voxels": 1, "radius": 0},
               {"prob": prob.cpu()}, {"prob": prob.double()}, {"prob": prob[:, :, ::2]}, {"belief": belief[:1]}, {"belief": belief.cpu()},
               {"restarted": restarted != 0}, {"restarted": restarted[:1]}, {"taps": k["taps_dev"][:-1]}, {"taps": k["taps"]},
               {"state": torch.zeros((rows, N - 1), device=DEV)}, {"state": prob[0]}, {"state": belief[1]},
               {"smoothed_out": prob}, {"smoothed_out": torch.empty((1, rows, N), device=DEV)}, {"smoothed_out": both[:2], "belief": both[1:]},
               {"smoothed_out": torch.empty((2, rows, N), device=DEV, dtype=torch.float64)}, {"smoothed": torch.empty((2, rows), device=DEV)},
               {"agreement": agreement[:1]}, {"joints": joints[:, :, :2]},
               {"have_link": torch.ones(rows, device=DEV)}, {"have_link": torch.ones(rows + 1, device=DEV, dtype=torch.int32)},
               {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}, {"coord": k["coord"][:-1]}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    torch.cuda.synchronize()
    assert (joints == -7).all() and (agreement == -7).all() and (flag == -7).all() and (state == 0).all()      # nothing was launched
    call()
    call(smoothed_out=belief)                                   # in place is allowed
    # the C entry point refuses on its own what the wrapper checks first
    lib = _lib.load()
    ws = torch.empty(_lib.volume_smooth_scratch_bytes(rows, G, R), device=DEV, dtype=torch.uint8)
    P = _lib._ptr

    def raw(radius=R, floor=1e-3, frames=2, grid=G, voxels=N, scratch_bytes=ws.numel(), state=state):
        return lib.se_volume_smooth_f32(P(prob), P(belief), P(restarted), P(k["coord"]), P(k["taps_dev"]), P(state), None, P(joints),
                                        P(agreement), P(flag), P(ws), scratch_bytes, frames, rows, voxels, grid, radius, floor, None,
                                        _lib._stream())
    assert raw() == 0
    assert raw(radius=17) == raw(radius=G) == raw(floor=2.0) == raw(floor=float("nan")) == raw(frames=0) == raw(voxels=N + 4) \
        == raw(grid=129) == -1
    assert raw(scratch_bytes=ws.numel() - 1) == -1 and raw(state=None) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 5. public surface
def test_module_smoother_equals_the_library_call(net64, two_forwards):
    G, J = net64.volume_size, 15
    N = G ** 3
    s = net64.volume_smoother()
    assert isinstance(s, VolumeSmoother) and s.filter.radius == 10 and s.filter.floor == 1e-3 and s.filter.sigma == 0.10
    f = net64.volume_filter()
    live = [s.push(vols, joints=kp) for kp, vols in two_forwards]
    ref = [f.step(vols, joints=kp, return_beliefs=True) for kp, vols in two_forwards]
    torch.cuda.synchronize()
    for a, b in zip(live, ref):                                 # push returns what the filter's step returns, bit for bit
        assert tuple(a) == tuple(b)
        for key in a:
            assert torch.equal(a[key], b[key]) if key == "restarted" else same_bits(a[key].cpu().numpy(), b[key].cpu().numpy()), key
    assert s.max_bytes > 0 and s.frames_stored == 4 and s.bytes_stored == 2 * 4 * J * N * 4
    res = s.finish(return_beliefs=True)
    torch.cuda.synchronize()
    assert tuple(res["joints"].shape) == (4, J, 3) and tuple(res["agreement"].shape) == tuple(res["smoothed"].shape) == (4, J)
    assert res["smoothed"].dtype == torch.bool and res["smoothed"][:3].all() and not res["smoothed"][3].any()
    assert [tuple(b.shape) for b in res["beliefs"]] == [(2, J, G, G, G)] * 2 and tuple(res["shift"].shape) == (4, J)
    coord = net64.coord_volumes[0].reshape(N, 3).float().contiguous().to(DEV)
    vols = torch.cat([v for _, v in two_forwards]).reshape(4, J, N)
    taps = torch.from_numpy(gaussian_taps(0.10, 10, net64.cuboid_side / G)).to(DEV)
    belief = torch.cat([r["beliefs"] for r in ref]).reshape(4, J, N)
    restarted = torch.cat([r["restarted"] for r in ref]).to(torch.int32)
    lib = smooth(vols, belief, restarted, coord, taps, G, 10, 1e-3)
    assert same_bits(torch.cat(res["beliefs"]).reshape(4, J, N).cpu().numpy(), lib["gamma"])
    assert same_bits(res["joints"][:3].cpu().numpy(), lib["joints"][:3]) and same_bits(res["agreement"].cpu().numpy(), lib["agreement"])
    assert torch.equal(res["joints"][3], res["filtered_joints"][3])          # not smoothed: the filter's own joint
    assert same_bits(res["filtered_joints"].cpu().numpy(), torch.cat([r["joints"] for r in ref]).cpu().numpy())
    kp = torch.cat([k for k, _ in two_forwards])
    assert torch.equal(res["shift"], (res["joints"] - kp).norm(dim=-1))
    assert torch.equal(res["shift_filtered"], (res["joints"] - res["filtered_joints"]).norm(dim=-1))
    ag = lib["agreement"][:3] * N
    print(f"synthetic weights: agreement x N {ag.min():.3g} .. {ag.max():.3g}, shift from the filtered joints up to "
          f"{float(res['shift_filtered'].max()):.4f} m")
    assert np.isfinite(lib["joints"]).all() and (lib["agreement"][:3] > 0).all()
    # the smoothed beliefs are volumes: the per-frame tools take them unchanged
    b = res["beliefs"][0]
    stats = net64.joint_statistics(b, res["joints"][:2])
    modes = net64.joint_modes(b, k=4, radius=2)
    torch.cuda.synchronize()
    assert torch.isfinite(stats["entropy"]).all() and (modes["count"] >= 1).all()
    assert torch.equal(modes["index"][..., 0], stats["peak_index"])
    # max_bytes too small: refused before anything is allocated or stepped
    small = net64.volume_smoother(max_bytes=2 * 2 * J * N * 4 - 1)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="0 frames are stored"):
        small.push(two_forwards[0][1])
    assert torch.cuda.memory_allocated() == before and small.filter.frames_seen == 0 and small.frames_stored == 0


def test_three_streams_with_the_event_chain_equal_one_stream():
    rows, G, R, T, floor = 15, 16, 5, 5, 1e-3
    k = filtered(rows, G, R, floor, T)
    one = pushes(make_smoother(k, G, R, floor), k["prob"], (1,) * T, G)
    streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    three = pushes(make_smoother(k, G, R, floor), k["prob"], (1,) * T, G, streams=streams)     # no host synchronisation between the calls
    for key in ("beliefs", "joints", "agreement", "filtered_joints"):
        assert same_bits(three[key], one[key]), key
    assert np.array_equal(three["smoothed"], one["smoothed"])
    for a, b in zip(three["live"], one["live"]):
        assert same_bits(a["beliefs"].cpu().numpy(), b["beliefs"].cpu().numpy())
    # ... and finish() on a stream of its own
    s = make_smoother(k, G, R, floor)
    for t in range(T):
        s.push(k["prob"][t:t + 1].view(1, rows, G, G, G), stream=streams[t % 3])
    res = s.finish(stream=streams[2])
    torch.cuda.synchronize()
    assert same_bits(res["joints"].cpu().numpy(), one["joints"])


def test_finish_waits_for_the_copies_of_every_push():
    """The production shape, where a push's two copies (31.4 MB) take longer than the host needs to issue what follows: three pushes on
    three streams and finish() on a fourth with no host synchronisation in between must give the bits of one stream.  The filter's
    event chain orders the steps only; finish() has to wait for the event behind the copies of every push."""
    rows, G, R, T, floor = 15, 64, 10, 3, 1e-3
    k = filtered(rows, G, R, floor, T)
    one = pushes(make_smoother(k, G, R, floor), k["prob"], (1,) * T, G)
    streams = [torch.cuda.Stream(device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    s = make_smoother(k, G, R, floor)
    for t in range(T):
        s.push(k["prob"][t:t + 1].view(1, rows, G, G, G), stream=streams[t])
    assert len({id(p[5]) for p in s._pushes}) == T            # one event per push
    res = s.finish(return_beliefs=True, stream=streams[3])
    # a second track straight behind it reuses the workspace on another stream
    for t in range(T):
        s.push(k["prob"][t:t + 1].view(1, rows, G, G, G), stream=streams[(t + 1) % 3])
    again = s.finish(stream=streams[0])
    torch.cuda.synchronize()
    assert same_bits(torch.cat(res["beliefs"]).reshape(T, rows, -1).cpu().numpy(), one["beliefs"])
    assert same_bits(res["joints"].cpu().numpy(), one["joints"]) and same_bits(res["agreement"].cpu().numpy(), one["agreement"])
    # the second track continues the filter's state (frame 0 is no restart), so it is compared with the same through one stream
    ref = make_smoother(k, G, R, floor)
    for _ in range(2):
        for t in range(T):
            ref.push(k["prob"][t:t + 1].view(1, rows, G, G, G))
        want = ref.finish()
    torch.cuda.synchronize()
    assert same_bits(again["joints"].cpu().numpy(), want["joints"].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ 6. command line
def test_run_sequence_smooth_outputs(tmp_path, capsys):
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
    res = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl"), "--smooth_output", str(tmp_path / "s" / "smoothed.pkl"),
                                      "--smooth_info_output", str(tmp_path / "s" / "info.pkl"),
                                      "--filter_output", str(tmp_path / "s" / "filtered.pkl")])
    out = capsys.readouterr().out
    assert "smoothed volumes" in out.splitlines()[-1] and "filtered" in out.splitlines()[-1] and "filtered volumes" in out.splitlines()[-2]
    loaded = {}
    for name in ("smoothed", "info", "filtered"):
        with open(tmp_path / "s" / f"{name}.pkl", "rb") as f:
            loaded[name] = pickle.load(f)
    with open(tmp_path / "plain.pkl", "rb") as f:
        preds = pickle.load(f)
    smoothed, info, filt = loaded["smoothed"], loaded["info"], loaded["filtered"]
    assert type(smoothed) is type(preds) and len(smoothed) == len(preds) == len(info) == len(filt) == 3
    for a, b, fr, fj in zip(smoothed, preds, info, filt):
        assert type(a) is type(b) and a.dtype == b.dtype == np.float32 and a.shape == b.shape == (15, 3) and np.isfinite(a).all()
        assert tuple(fr) == ("joints", "smoothed", "agreement", "filtered_joints", "shift_filtered", "shift")
        assert np.array_equal(fr["joints"], a) and same_bits(fr["filtered_joints"], fj)
        assert np.allclose(fr["shift"], np.linalg.norm(a.astype(np.float64) - b, axis=1), rtol=1e-5, atol=1e-7)
    assert info[0]["smoothed"].all() and info[1]["smoothed"].all() and not info[2]["smoothed"].any()
    assert (info[0]["agreement"] > 0).all() and np.isnan(info[2]["agreement"]).all()
    assert same_bits(smoothed[2], filt[2])                      # the last frame's smoothed joints are the filtered ones
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((3, 15, 3)), f)
    ev = evaluate.main(["--pred_dir", str(tmp_path / "s" / "smoothed.pkl"), "--gt", str(tmp_path / "gt.pkl")])
    capsys.readouterr()
    assert ev["frames"] == 3 and np.isfinite(ev["mpjpe"])
    assert np.isfinite(res["smoothed_mpjpe"]) and np.isfinite(res["filtered_mpjpe"]) and len(res["smoothed"]) == 3 == len(res["smoother"])
    # driving VolumeSmoother by hand on the same volumes gives the same joints, bit for bit
    from sceneego_amd import load_config as load
    runner = run_sequence.SequenceRunner(load(str(cfg_path)), weights="synthetic")
    images, _, depths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    s = runner.net.volume_smoother(sigma=0.1, radius=None, floor=1e-3)
    for i in range(0, 3, 2):
        img = runner._images([JpegFile(p) for p in images[i:i + 2]])
        depth = runner._depths(depths[i:i + 2])
        with torch.no_grad():
            kp, _, vol, _ = runner.net(img, runner.net.grid_coord_proj_batch, runner.net.coord_volumes, depth_map_batch=depth)
        s.push(vol, joints=kp)
    by_hand = s.finish()["joints"].cpu().numpy()
    assert len(by_hand) == 3 and all(same_bits(a, b) for a, b in zip(by_hand, smoothed))
