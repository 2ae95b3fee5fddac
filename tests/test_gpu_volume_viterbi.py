"""GPU: the max-product pass (csrc/volume_viterbi.hip: se_volume_viterbi_f32, se_volume_viterbi_path_i32, se_volume_viterbi_refine_f32)
against its numpy float32 model (tests/volume_viterbi_model.py) BIT FOR BIT, its independence of how a sequence is cut into calls and
pushes, the direction of the offsets, NaN cells and frames, streams, storage, arguments, the public surface and the command line.

Inputs: those of tests/test_gpu_volume_filter.py (``sequence``: make_logits with seed 1000 G + 10 rows + R, softmaxed by
se_softargmax3d_f32 on the device); the model is fed the kernel's own inputs.  There is no tolerance anywhere: every product is one
float32 rounding in the model and in the kernel alike, and every other operation is a comparison or a selection.  The scaled scores of
these cases run down into the denormals and to exact zeros (printed), so gradual underflow is exercised.  The one condition on the
inputs is asserted on the model in the test itself: no frame's maximum is attained twice (the lowest index would still be defined, but a
seed whose path hangs on a tie should not hide).
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
from sceneego_amd.volume_viterbi import VolumeViterbi, segment_log_scores
from test_gpu_volume_filter import net64, same_bits, sequence, two_forwards  # noqa: F401  (the two fixtures)
from volume_filter_cases import SIDE
from volume_viterbi_model import JUMP, refine_model, viterbi_path, volume_viterbi_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

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
    (1, 128, 16, 1e-3, 2),       # the largest planes: 144 KB and 96 KB of LDS per workgroup
]


# ------------------------------------------------------------------------------------------------------------------ launches
def forward(prob, taps_dev, G, R, floor, cuts=None, states=False):
    """The _lib-level forward pass over ``prob`` [T, rows, N] in calls of ``cuts`` frames each, state / peak_state / best_state carried.
    Host arrays: back, peak, best, exponent, restarted, state (after the last call) and, with ``states``, state after every call."""
    T, rows, N = prob.shape
    cuts = (T,) if cuts is None else tuple(cuts)
    assert sum(cuts) == T
    state = torch.full((rows, N), float("nan"), device=DEV)
    peak_state = torch.full((rows,), 12345, device=DEV, dtype=torch.int32)
    best_state = torch.full((rows,), float("nan"), device=DEV)
    back = torch.full((T, rows, N), -7, device=DEV, dtype=torch.int32)
    peak = torch.empty((T, rows), device=DEV, dtype=torch.int32)
    best = torch.empty((T, rows), device=DEV)
    exponent = torch.empty((T, rows), device=DEV, dtype=torch.int32)
    restarted = torch.empty((T, rows), device=DEV, dtype=torch.int32)
    ones = torch.ones(rows, device=DEV, dtype=torch.int32)
    t, after = 0, []
    for n in cuts:
        _lib.volume_viterbi(prob[t:t + n].contiguous(), taps_dev, state, peak_state, best_state, back[t:t + n], peak[t:t + n],
                            best[t:t + n], exponent[t:t + n], restarted[t:t + n], n, rows, N, G, R, floor,
                            have_prior=None if t == 0 else ones)
        if states:
            after.append(state.cpu().numpy())
        t += n
    torch.cuda.synchronize()
    out = {"back": back.cpu().numpy(), "peak": peak.cpu().numpy(), "best": best.cpu().numpy(), "exponent": exponent.cpu().numpy(),
           "restarted": restarted.cpu().numpy(), "state": state.cpu().numpy(), "after": after,
           "dev": {"back": back, "peak": peak, "restarted": restarted}}
    assert np.array_equal(peak_state.cpu().numpy(), out["peak"][-1])
    assert same_bits(best_state.cpu().numpy(), out["best"][-1])
    return out


def walk(dev, cuts=None):
    """The _lib-level back-walk over the device arrays of ``forward`` in chunks of ``cuts`` frames, last chunk first: (index, jumped)."""
    back, peak, restarted = dev["back"], dev["peak"], dev["restarted"]
    T, rows, N = back.shape
    cuts = (T,) if cuts is None else tuple(cuts)
    starts = np.concatenate([[0], np.cumsum(cuts)]).tolist()
    cursor = torch.full((rows,), 777, device=DEV, dtype=torch.int32)      # not read by the first call
    index = torch.full((T, rows), -9, device=DEV, dtype=torch.int32)
    jumped = torch.full((T, rows), -9, device=DEV, dtype=torch.int32)
    for i in range(len(cuts) - 1, -1, -1):
        t0, t1 = starts[i], starts[i + 1]
        _lib.volume_viterbi_path(back[t0:t1], peak[t0:t1], restarted[t0:t1], cursor, index[t0:t1], jumped[t0:t1], t1 - t0, rows, N,
                                 have_next=int(t1 != T))
    torch.cuda.synchronize()
    return index, jumped.cpu().numpy()


def refine(prob, coord, index, G, r):
    T, rows, N = prob.shape
    joints = torch.full((T, rows, 3), -7.0, device=DEV)
    _lib.volume_viterbi_refine(prob.contiguous() if r > 0 else None, coord, index, joints, T, rows, N, G, r)
    torch.cuda.synchronize()
    return joints.cpu().numpy()


@functools.lru_cache(maxsize=None)
def modelled(rows, G, R, floor, T):
    """The shared sequence with the model run once on the kernel's own inputs (nothing below modifies it)."""
    k = dict(sequence(rows, G, R, T))
    k["m"] = volume_viterbi_model(k["p"], k["taps"], G, floor)
    k["m"]["index"], k["m"]["jumped"] = viterbi_path(k["m"]["back"], k["m"]["peak"], k["m"]["restarted"])
    return k


def check_forward(got, want, label):
    for key in ("back", "peak", "exponent"):
        assert np.array_equal(got[key], want[key]), f"{label}: {key}"
    assert np.array_equal(got["restarted"] != 0, want["restarted"]) and set(np.unique(got["restarted"])) <= {0, 1}, label
    assert same_bits(got["best"], want["best"]), f"{label}: best"
    assert same_bits(got["state"], want["state"][-1]), f"{label}: state"
    for t, s in enumerate(got["after"]):
        assert same_bits(s, want["state"][t]), f"{label}: state after frame {t}"


def make_path(k, G, R, floor, **kw):
    return VolumeViterbi(k["coord"], G, SIDE, sigma=R * (SIDE / G) / 3.0, radius=R, floor=floor, **kw)


def pushes(v, prob, cuts, G, streams=None, finish_stream=None, **kw):
    T, rows, N = prob.shape
    assert sum(cuts) == T
    live, t = [], 0
    for i, n in enumerate(cuts):
        extra = {} if streams is None else {"stream": streams[i % len(streams)]}
        live.append(v.push(prob[t:t + n].view(n, rows, G, G, G), **extra, **kw))
        t += n
    res = v.finish() if finish_stream is None else v.finish(stream=finish_stream)
    torch.cuda.synchronize()
    out = {key: res[key].cpu().numpy() for key in res}
    out["live"] = {key: torch.cat([x[key] for x in live]).cpu().numpy() for key in live[0]}
    return out


def same_result(a, b, keys=("joints", "coord", "moved")):
    for key in keys:
        assert same_bits(a[key], b[key]), key
    for key in ("index", "jumped", "segment_start"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["log_score"], b["log_score"], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("rows,G,R,floor,T", CASES)
def test_against_the_model_bit_for_bit(rows, G, R, floor, T):
    k = modelled(rows, G, R, floor, T)
    want = k["m"]
    label = f"rows {rows} G {G} R {R} floor {floor}"
    # the condition on the inputs, on the model
    assert not want["tied"].any(), f"{label}: a frame's maximum is attained twice"
    assert want["restarted"][0].all() and not want["restarted"][1:].any() and (want["peak"] >= 0).all()
    assert (want["best"] >= 1).all() and (want["best"] < 2).all()
    one = forward(k["prob"], k["taps_dev"], G, R, floor, cuts=(1,) * T, states=True)       # frame by frame: the state of every frame
    check_forward(one, want, label)
    whole = forward(k["prob"], k["taps_dev"], G, R, floor)
    check_forward(whole, want, label + ", one call")
    index, jumped = walk(whole["dev"])
    assert np.array_equal(index.cpu().numpy(), want["index"]) and np.array_equal(jumped != 0, want["jumped"]), label
    assert set(np.unique(jumped)) <= {0, 1}
    for r in ((0, 1) if G > 24 else (0, 1, 2, 3)):
        got = refine(k["prob"], k["coord"], index, G, r)
        assert same_bits(got, refine_model(k["p"], k["c"], want["index"], G, r)), f"{label}: joints, refine {r}"
    pos = want["state"][want["state"] > 0]
    print(f"{label}: scaled scores down to {pos.min():.3g}, {int((want['state'] == 0).sum())} exact zeros, exponents "
          f"{want['exponent'].min()}..{want['exponent'].max()}, {int(want['jump_bits'].sum())} back-pointers with the jump bit, "
          f"{int(want['jumped'].sum())} on the path")


def test_a_jump_bit_the_path_does_not_take():
    k = modelled(4, 10, 3, 1e-3, 5)
    assert k["m"]["jump_bits"].sum() > 0 and not k["m"]["jumped"].any()
    got = forward(k["prob"], k["taps_dev"], 10, 3, 1e-3)
    assert ((got["back"] >= 0) & ((got["back"] & JUMP) != 0)).sum() == k["m"]["jump_bits"].sum()


def teleport(G, rows=3):
    """Row r: a sharp lobe that moves one voxel, then teleports across the grid, then moves one voxel again (softmaxed on the host)."""
    from volume_filter_cases import softmax32
    ax = np.arange(G, dtype=np.float64)
    logits = np.zeros((4, rows, G ** 3), dtype=np.float32)
    for r in range(rows):
        for t, c in enumerate(((1, 1 + r, 1), (1, 1 + r, 2), (G - 2, G - 3, G - 2 - r), (G - 2, G - 3, G - 3 - r))):
            g = [np.exp(-(ax - c[a]) ** 2 / 2.0) for a in range(3)]
            logits[t, r] = (12.0 * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]).reshape(-1)
    rng = np.random.default_rng(3)
    return softmax32(logits + 0.01 * rng.standard_normal(logits.shape).astype(np.float32))


def test_a_teleporting_lobe_is_reached_by_a_jump():
    G, R, floor = 12, 1, 1e-2
    p = teleport(G)
    taps = gaussian_taps(R * (SIDE / G) / 3.0, R, SIDE / G)
    want = volume_viterbi_model(p, taps, G, floor)
    want["index"], want["jumped"] = viterbi_path(want["back"], want["peak"], want["restarted"])
    assert not want["tied"].any() and want["jumped"].any() and want["jumped"][2].all() and not want["restarted"][1:].any()
    prob = torch.from_numpy(p).to(DEV)
    got = forward(prob, torch.from_numpy(taps).to(DEV), G, R, floor, cuts=(2, 2), states=True)
    for key in ("back", "peak", "exponent"):
        assert np.array_equal(got[key], want[key]), key
    assert same_bits(got["best"], want["best"]) and same_bits(got["after"][0], want["state"][1]) and same_bits(got["state"], want["state"][3])
    for cuts in ((4,), (2, 2), (1, 3), (3, 1), (1, 1, 1, 1)):     # the jump crosses a chunk boundary of the walk in some of these
        index, jumped = walk(got["dev"], cuts)
        assert np.array_equal(index.cpu().numpy(), want["index"]) and np.array_equal(jumped != 0, want["jumped"]), cuts


# ------------------------------------------------------------------------------------------------------------------ 2. cuts
@pytest.mark.parametrize("rows,G,R", [(15, 16, 5), (4, 10, 3)])
def test_results_do_not_depend_on_how_the_frames_are_cut(rows, G, R):
    T, floor = 5, 1e-3
    k = modelled(rows, G, R, floor, T)
    lib = [forward(k["prob"], k["taps_dev"], G, R, floor, cuts=cuts) for cuts in ((5,), (2, 3), (3, 2), (1, 1, 1, 1, 1))]
    for other in lib[1:]:
        for key in ("back", "peak", "exponent", "restarted"):
            assert np.array_equal(lib[0][key], other[key]), key
        assert same_bits(lib[0]["best"], other["best"]) and same_bits(lib[0]["state"], other["state"])
    walks = [walk(lib[0]["dev"], cuts) for cuts in ((5,), (2, 3), (4, 1), (1, 1, 1, 1, 1))]
    for index, jumped in walks[1:]:
        assert torch.equal(index, walks[0][0]) and np.array_equal(jumped, walks[0][1])
    runs = [pushes(make_path(k, G, R, floor), k["prob"], cuts, G) for cuts in ((5,), (2, 3), (1, 1, 1, 1, 1), (5,))]
    for other in runs[1:]:
        same_result(runs[0], other)
        for key in ("peak_index", "exponent", "restarted"):
            assert np.array_equal(runs[0]["live"][key], other["live"][key]), key
        assert same_bits(runs[0]["live"]["best"], other["live"]["best"])
    # ... and the class is the _lib-level calls and the model
    a, want = runs[0], k["m"]
    assert tuple(a) == ("joints", "index", "coord", "jumped", "segment_start", "log_score", "moved", "live")
    assert np.array_equal(a["index"], want["index"]) and a["index"].dtype == np.int32 and a["jumped"].dtype == np.bool_
    assert np.array_equal(a["live"]["peak_index"], lib[0]["peak"]) and a["live"]["restarted"].dtype == np.bool_
    assert same_bits(a["joints"], refine_model(k["p"], k["c"], want["index"], G, 1)) and same_bits(a["coord"], k["c"][want["index"]])
    assert a["segment_start"][0].all() and not a["segment_start"][1:].any()
    ls = segment_log_scores(want["best"], want["exponent"], want["restarted"])
    assert a["log_score"].dtype == np.float64 and np.array_equal(a["log_score"], ls, equal_nan=True) and np.isfinite(ls[-1]).all()
    assert np.isnan(a["moved"][0]).all()
    step = np.linalg.norm(a["coord"][1:].astype(np.float64) - a["coord"][:-1], axis=-1)
    assert np.allclose(a["moved"][1:], step, rtol=1e-6, atol=1e-7)
    # refine = 0 stores no volumes and returns the voxel centres
    v0 = make_path(k, G, R, floor, refine=0)
    r0 = pushes(v0, k["prob"], (2, 3), G)
    assert same_bits(r0["joints"], a["coord"]) and np.array_equal(r0["index"], a["index"])


def test_storage_shift_and_reset():
    rows, G, R, T, floor = 4, 10, 3, 5, 1e-3
    k = modelled(rows, G, R, floor, T)
    N = G ** 3
    v = make_path(k, G, R, floor, max_bytes=2 * 3 * rows * N * 4)
    given = torch.zeros((2, rows, 3), device=DEV)
    r = v.push(k["prob"][:2].view(2, rows, G, G, G), joints=given)
    assert tuple(r) == ("peak_index", "best", "exponent", "restarted")
    assert v.frames_stored == 2 and v.bytes_stored == 2 * 2 * rows * N * 4 and v.frames_seen == 2
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="2 frames are stored"):
        v.push(k["prob"][2:4].view(2, rows, G, G, G))          # 4 frames would exceed max_bytes: nothing run, nothing stored
    assert torch.cuda.memory_allocated() == before and v.frames_stored == 2 and v.frames_seen == 2
    v.push(k["prob"][2:3].view(1, rows, G, G, G))
    res = v.finish()
    assert tuple(res) == ("joints", "index", "coord", "jumped", "segment_start", "log_score", "moved", "shift")
    assert tuple(res["shift"].shape) == (3, rows) and torch.equal(res["shift"][:2], res["joints"][:2].norm(dim=-1))
    assert torch.isnan(res["shift"][2]).all() and v.frames_stored == 0
    assert np.array_equal(res["index"].cpu().numpy(), viterbi_path(k["m"]["back"][:3], k["m"]["peak"][:3], k["m"]["restarted"][:3])[0])
    frames = op.volume_path_to_numpy(res)
    assert len(frames) == 3 and tuple(frames[0]) == tuple(res)
    assert frames[1]["joints"].shape == (rows, 3) and frames[1]["jumped"].dtype == np.bool_ and frames[1]["log_score"].shape == (rows,)
    with pytest.raises(ValueError):
        v.finish()
    # frames pushed after a finish() continue the recursion (no restart) and are walked as a piece of their own
    r = v.push(k["prob"][3:5].view(2, rows, G, G, G))
    assert not r["restarted"].any() and np.array_equal(r["peak_index"].cpu().numpy(), k["m"]["peak"][3:5])
    tail = v.finish()
    assert np.array_equal(tail["index"].cpu().numpy(), k["m"]["index"][3:5]) and not tail["segment_start"].any()
    v.reset()
    assert v.frames_seen == 0 and v.push(k["prob"][:1].view(1, rows, G, G, G))["restarted"].all()


# ------------------------------------------------------------------------------------------------------------------ 3. direction
def test_asymmetric_taps_pin_the_direction_of_the_offsets():
    """The kernel equals the model under taps that are not symmetric, and the model with the taps reversed (the offsets taken the other
    way round) gives other back-pointers and other scores on this input: the comparison is exact, so any difference tells them apart
    (a quarter of the back-pointers differ here; the rest are jumps or point at the lobe either way)."""
    rows, G, R, floor, T = 2, 8, 2, 1e-3, 4
    k = sequence(rows, G, R, T)
    w = np.array([0.05, 0.10, 0.20, 0.30, 0.35], dtype=np.float64)
    taps = (w / w.sum()).astype(np.float32)
    want = volume_viterbi_model(k["p"], taps, G, floor)
    wrong = volume_viterbi_model(k["p"], np.ascontiguousarray(taps[::-1]), G, floor)
    differ = (want["back"][1:] != wrong["back"][1:]).mean()
    print(f"asymmetric taps: {differ:.3f} of the back-pointers differ from those of the reversed taps")
    assert not want["tied"].any() and differ > 0 and not np.array_equal(want["state"][-1], wrong["state"][-1])
    got = forward(k["prob"], torch.from_numpy(taps).to(DEV), G, R, floor, cuts=(1,) * T, states=True)
    check_forward(got, want, "asymmetric taps")
    index, jumped = walk(got["dev"])
    want_index, want_jumped = viterbi_path(want["back"], want["peak"], want["restarted"])
    assert np.array_equal(index.cpu().numpy(), want_index) and np.array_equal(jumped != 0, want_jumped)


# ------------------------------------------------------------------------------------------------------------------ 4. NaN
def test_a_nan_cell_is_passed_over_and_a_nan_frame_cuts_the_track():
    rows, G, R, T, floor = 15, 16, 5, 5, 1e-3
    k = modelled(rows, G, R, floor, T)
    clean = forward(k["prob"], k["taps_dev"], G, R, floor)
    clean_index, clean_jumped = walk(clean["dev"])
    prob = k["prob"].clone()
    prob[1, 7, 1234] = float("nan")                              # one cell of row 7
    prob[2, 3] = float("nan")                                    # a whole frame of row 3
    p = prob.cpu().numpy()
    want = volume_viterbi_model(p, k["taps"], G, floor)
    want["index"], want["jumped"] = viterbi_path(want["back"], want["peak"], want["restarted"])
    assert want["restarted"][:, 7].tolist() == [True, False, False, False, False]
    assert want["restarted"][:, 3].tolist() == [True, False, True, True, False] and want["peak"][2, 3] == -1 and want["index"][2, 3] == -1
    assert not want["tied"].any()
    got = forward(prob, k["taps_dev"], G, R, floor, cuts=(2, 1, 2), states=True)
    for key in ("back", "peak", "exponent"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["restarted"] != 0, want["restarted"]) and same_bits(got["best"], want["best"])
    assert np.isnan(got["best"][2, 3]) and got["exponent"][2, 3] == 0 and (got["back"][2:4, 3] == -1).all()
    assert same_bits(got["after"][1][3], p[2, 3]) and np.isnan(got["after"][0][7, 1234])     # the copy of p; the NaN score of the one cell
    fin = np.isfinite(want["state"])
    for i, t in enumerate((1, 2, 4)):
        assert np.array_equal(np.isfinite(got["after"][i]), fin[t]) and same_bits(got["after"][i][fin[t]], want["state"][t][fin[t]])
    index, jumped = walk(got["dev"], (2, 1, 2))
    assert np.array_equal(index.cpu().numpy(), want["index"]) and np.array_equal(jumped != 0, want["jumped"])
    joints = refine(prob, k["coord"], index, G, 1)
    assert same_bits(joints, refine_model(p, k["c"], want["index"], G, 1))
    assert np.isnan(joints[2, 3]).all() and np.isfinite(np.delete(joints, 3, axis=1)).all() and np.isfinite(joints[[0, 1, 3, 4], 3]).all()
    # the window of a refinement holds the NaN cell: it is passed over
    at = torch.full((1, rows), 1234, device=DEV, dtype=torch.int32)
    near = refine(prob[1:2], k["coord"], at, G, 1)
    assert np.isfinite(near).all() and same_bits(near, refine_model(p[1:2], k["c"], at.cpu().numpy(), G, 1))
    # other rows: bit-equal to the clean run
    others = [r for r in range(rows) if r not in (3, 7)]
    for key in ("back", "peak", "exponent", "restarted"):
        assert np.array_equal(got[key][:, others], clean[key][:, others]), key
    assert same_bits(got["best"][:, others], clean["best"][:, others]) and same_bits(got["state"][others], clean["state"][others])
    assert np.array_equal(index.cpu().numpy()[:, others], clean_index.cpu().numpy()[:, others])
    # the class reports the cut: a segment start at the NaN frame and at the frame behind it, a score per segment
    res = pushes(make_path(k, G, R, floor), prob, (2, 3), G)
    assert res["segment_start"][:, 3].tolist() == [True, False, True, True, False] and np.isnan(res["coord"][2, 3]).all()
    assert np.isfinite(res["log_score"][[1, 4], 3]).all() and np.isnan(res["log_score"][[0, 2, 3], 3]).all()
    assert np.isnan(res["moved"][[2, 3], 3]).all() and np.isfinite(res["moved"][[1, 4], 3]).all()


# ------------------------------------------------------------------------------------------------------------------ 5. streams
def test_three_streams_with_the_event_chain_equal_one_stream():
    rows, G, R, T, floor = 15, 16, 5, 5, 1e-3
    k = modelled(rows, G, R, floor, T)
    one = pushes(make_path(k, G, R, floor), k["prob"], (1,) * T, G)
    streams = [torch.cuda.Stream(device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    three = pushes(make_path(k, G, R, floor), k["prob"], (1,) * T, G, streams=streams)     # no host synchronisation between the calls
    same_result(three, one)
    assert same_bits(three["live"]["best"], one["live"]["best"]) and np.array_equal(three["live"]["peak_index"], one["live"]["peak_index"])
    own = pushes(make_path(k, G, R, floor), k["prob"], (1,) * T, G, streams=streams, finish_stream=streams[2])
    same_result(own, one)


def test_finish_waits_for_the_copies_of_every_push():
    """The production shape, where a push's copy of the volumes (15.7 MB) takes longer than the host needs to issue what follows: three
    pushes on three streams and finish() on a fourth with no host synchronisation in between must give the bits of one stream."""
    rows, G, R, T, floor = 15, 64, 10, 3, 1e-3
    k = modelled(rows, G, R, floor, T)
    one = pushes(make_path(k, G, R, floor), k["prob"], (1,) * T, G)
    assert np.array_equal(one["index"], k["m"]["index"])
    streams = [torch.cuda.Stream(device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    v = make_path(k, G, R, floor)
    for t in range(T):
        v.push(k["prob"][t:t + 1].view(1, rows, G, G, G), stream=streams[t])
    assert len({id(p[7]) for p in v._pushes}) == T              # one event per push
    res = v.finish(stream=streams[3])
    # a second track straight behind it reuses the cursor on another stream
    v.reset()
    for t in range(T):
        v.push(k["prob"][t:t + 1].view(1, rows, G, G, G), stream=streams[(t + 1) % 3])
    again = v.finish(stream=streams[0])
    torch.cuda.synchronize()
    for r in (res, again):
        assert same_bits(r["joints"].cpu().numpy(), one["joints"]) and np.array_equal(r["index"].cpu().numpy(), one["index"])
        assert np.array_equal(r["log_score"].cpu().numpy(), one["log_score"], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ 6. arguments
def test_bad_arguments_raise_and_do_not_launch():
    rows, G, R, T, floor = 4, 10, 3, 5, 1e-3
    k = modelled(rows, G, R, floor, T)
    N = G ** 3
    prob = k["prob"][:2].contiguous()
    state = torch.zeros((rows, N), device=DEV)
    peak_state, best_state = torch.full((rows,), -7, device=DEV, dtype=torch.int32), torch.full((rows,), -7.0, device=DEV)
    back = torch.full((2, rows, N), -7, device=DEV, dtype=torch.int32)
    ints = [torch.full((2, rows), -7, device=DEV, dtype=torch.int32) for _ in range(3)]
    best = torch.full((2, rows), -7.0, device=DEV)

    def call(**kw):
        a = {"prob": prob, "taps": k["taps_dev"], "state": state, "peak_state": peak_state, "best_state": best_state, "back_out": back,
             "peak": ints[0], "best": best, "exponent": ints[1], "restarted": ints[2], "frames": 2, "rows": rows, "voxels": N, "grid": G,
             "radius": R, "floor": floor}
        a.update(kw)
        return _lib.volume_viterbi(**a)

    for kw in ({"radius": 17}, {"radius": -1}, {"radius": G}, {"floor": -0.1}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0},
               {"frames": 3}, {"rows": 0}, {"grid": G + 1}, {"voxels": N + 1}, {"grid": 1, "voxels": 1, "radius": 0},
               {"prob": prob.cpu()}, {"prob": prob.double()}, {"prob": prob[:, :, ::2]}, {"taps": k["taps_dev"][:-1]}, {"taps": k["taps"]},
               {"state": torch.zeros((rows, N - 1), device=DEV)}, {"state": prob[0]}, {"back_out": back[:1]},
               {"back_out": back.float()}, {"peak_state": peak_state.float()}, {"best_state": best_state[:-1]},
               {"peak": ints[0][:1]}, {"best": best.double()}, {"exponent": ints[1].long()}, {"restarted": ints[2] != 0},
               {"have_prior": torch.ones(rows, device=DEV)}, {"have_prior": torch.ones(rows + 1, device=DEV, dtype=torch.int32)},
               {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    index, jumped = ints[0].clone(), ints[1].clone()
    cursor = torch.full((rows,), -7, device=DEV, dtype=torch.int32)
    joints = torch.full((2, rows, 3), -7.0, device=DEV)
    for kw in ({"frames": 0}, {"frames": 3}, {"rows": 0}, {"voxels": 0}, {"voxels": N + 1}, {"have_next": 2}, {"back": back.float()},
               {"peak": ints[0][:1]}, {"cursor": cursor[:-1]}, {"index": index.float()}, {"jumped": jumped.cpu()}):
        a = {"back": back, "peak": ints[0], "restarted": ints[2], "cursor": cursor, "index": index, "jumped": jumped, "frames": 2,
             "rows": rows, "voxels": N, "have_next": 0}
        a.update(kw)
        with pytest.raises(_lib.HipExtensionError):
            _lib.volume_viterbi_path(**a)
    for kw in ({"refine": 4}, {"refine": -1}, {"refine": 1.5}, {"prob": None}, {"prob": prob[:1]}, {"coord": k["coord"][:-1]},
               {"index": index.long()}, {"joints": joints[:, :, :2]}, {"grid": G + 1}, {"frames": 0}):
        a = {"prob": prob, "coord": k["coord"], "index": index, "joints": joints, "frames": 2, "rows": rows, "voxels": N, "grid": G,
             "refine": 1}
        a.update(kw)
        with pytest.raises(_lib.HipExtensionError):
            _lib.volume_viterbi_refine(**a)
    torch.cuda.synchronize()
    for t in ints + [back, peak_state, index, jumped, cursor]:   # nothing was launched
        assert (t == -7).all()
    assert (best == -7).all() and (best_state == -7).all() and (joints == -7).all() and (state == 0).all()
    # the C entry points refuse on their own what the wrappers check first
    lib = _lib.load()
    ws = torch.empty(_lib.volume_viterbi_scratch_bytes(rows, G, R), device=DEV, dtype=torch.uint8)
    P = _lib._ptr

    def raw(radius=R, floor=1e-3, frames=2, grid=G, voxels=N, scratch_bytes=ws.numel(), state=state):
        return lib.se_volume_viterbi_f32(P(prob), P(k["taps_dev"]), P(state), P(peak_state), P(best_state), P(back), P(ints[0]), P(best),
                                         P(ints[1]), P(ints[2]), P(ws), scratch_bytes, frames, rows, voxels, grid, radius, floor, None,
                                         _lib._stream())

    assert raw(radius=17) == raw(radius=G) == raw(floor=2.0) == raw(floor=float("nan")) == raw(frames=0) == raw(voxels=N + 4) \
        == raw(grid=129) == raw(scratch_bytes=ws.numel() - 1) == raw(state=None) == -1

    def raw_path(frames=2, voxels=N, have_next=0, cursor=cursor):
        return lib.se_volume_viterbi_path_i32(P(back), P(ints[0]), P(ints[2]), P(cursor), P(index), P(jumped), frames, rows, voxels,
                                              have_next, _lib._stream())

    def raw_refine(refine=1, grid=G, voxels=N, joints=joints):
        return lib.se_volume_viterbi_refine_f32(P(prob), P(k["coord"]), P(index), P(joints), 2, rows, voxels, grid, refine, _lib._stream())

    assert raw_path(frames=0) == raw_path(voxels=0) == raw_path(have_next=2) == raw_path(cursor=None) == -1
    assert raw_refine(refine=4) == raw_refine(refine=-1) == raw_refine(grid=G + 1) == raw_refine(voxels=N + 1) == raw_refine(joints=None) == -1
    torch.cuda.synchronize()
    assert (back == -7).all() and (index == -7).all() and (joints == -7).all()
    assert raw() == 0 and raw_path() == 0 and raw_refine() == 0
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy(), k["m"]["back"][:2]) and np.array_equal(index.cpu().numpy(), viterbi_path(
        k["m"]["back"][:2], k["m"]["peak"][:2], k["m"]["restarted"][:2])[0])
    # an index out of range in the cursor or in a back-pointer is never followed
    bad_back = back.clone()
    bad_back[1] = N + 5
    cursor[:] = N
    _lib.volume_viterbi_path(bad_back, ints[0], ints[2], cursor, index, jumped, 2, rows, N, have_next=1)
    torch.cuda.synchronize()
    assert torch.equal(index, ints[0]) and (cursor == -1).all()


# ------------------------------------------------------------------------------------------------------------------ 7. public surface
def test_module_path_equals_the_library_calls(net64, two_forwards):
    G, J = net64.volume_size, 15
    N = G ** 3
    v = net64.volume_path()
    assert isinstance(v, VolumeViterbi) and v.filter.radius == 10 and v.filter.floor == 1e-3 and v.filter.sigma == 0.10 and v.refine == 1
    live = [v.push(vols, joints=kp) for kp, vols in two_forwards]
    assert v.max_bytes > 0 and v.frames_stored == 4 and v.bytes_stored == 2 * 4 * J * N * 4
    res = v.finish()
    torch.cuda.synchronize()
    assert tuple(res["joints"].shape) == tuple(res["coord"].shape) == (4, J, 3) and tuple(res["index"].shape) == (4, J)
    assert res["jumped"].dtype == torch.bool and res["segment_start"][0].all() and not res["segment_start"][1:].any()
    coord = net64.coord_volumes[0].reshape(N, 3).float().contiguous().to(DEV)
    vols = torch.cat([x for _, x in two_forwards]).reshape(4, J, N)
    taps = torch.from_numpy(gaussian_taps(0.10, 10, net64.cuboid_side / G)).to(DEV)
    lib = forward(vols, taps, G, 10, 1e-3, cuts=(2, 2))
    index, jumped = walk(lib["dev"], (2, 2))
    assert torch.equal(res["index"], index) and np.array_equal(res["jumped"].cpu().numpy(), jumped != 0)
    assert same_bits(res["joints"].cpu().numpy(), refine(vols, coord, index, G, 1))
    assert np.array_equal(torch.cat([x["peak_index"] for x in live]).cpu().numpy(), lib["peak"])
    assert same_bits(torch.cat([x["best"] for x in live]).cpu().numpy(), lib["best"])
    kp = torch.cat([x for x, _ in two_forwards])
    assert torch.equal(res["shift"], (res["joints"] - kp).norm(dim=-1))
    assert (res["index"] >= 0).all() and torch.isfinite(res["joints"]).all() and torch.isfinite(res["log_score"][-1]).all()
    # the path voxel of the last frame is its best voxel, and the joint lies within the refinement window of its voxel
    assert torch.equal(res["index"][-1], live[-1]["peak_index"][-1])
    h = net64.cuboid_side / G
    assert ((res["joints"] - res["coord"]).abs() <= 1.0001 * h).all()
    print(f"synthetic weights: path up to {float(res['shift'].max()):.4f} m from the soft-argmax joints, {int(res['jumped'].sum())} jumps")
    # max_bytes too small: refused before anything is allocated or run
    small = net64.volume_path(max_bytes=2 * 2 * J * N * 4 - 1)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="0 frames are stored"):
        small.push(two_forwards[0][1])
    assert torch.cuda.memory_allocated() == before and small.frames_seen == 0 and small.frames_stored == 0


# ------------------------------------------------------------------------------------------------------------------ 8. command line
def test_run_sequence_path_outputs(tmp_path, capsys):
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
    res = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl"), "--path_output", str(tmp_path / "p" / "path.pkl"),
                                      "--path_info_output", str(tmp_path / "p" / "info.pkl")])
    out = capsys.readouterr().out
    assert "most probable path" in out.splitlines()[-1] and "soft-argmax" in out.splitlines()[-1]
    loaded = {}
    for name in ("path", "info"):
        with open(tmp_path / "p" / f"{name}.pkl", "rb") as f:
            loaded[name] = pickle.load(f)
    with open(tmp_path / "plain.pkl", "rb") as f:
        preds = pickle.load(f)
    path, info = loaded["path"], loaded["info"]
    assert type(path) is type(preds) and len(path) == len(preds) == len(info) == 3
    for a, b, fr in zip(path, preds, info):
        assert type(a) is type(b) and a.dtype == b.dtype == np.float32 and a.shape == b.shape == (15, 3) and np.isfinite(a).all()
        assert tuple(fr) == ("joints", "index", "coord", "jumped", "segment_start", "log_score", "moved", "shift")
        assert np.array_equal(fr["joints"], a)
        assert np.allclose(fr["shift"], np.linalg.norm(a.astype(np.float64) - b, axis=1), rtol=1e-5, atol=1e-7)
    assert info[0]["segment_start"].all() and not info[1]["segment_start"].any() and np.isfinite(info[2]["log_score"]).all()
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((3, 15, 3)), f)
    ev = evaluate.main(["--pred_dir", str(tmp_path / "p" / "path.pkl"), "--gt", str(tmp_path / "gt.pkl")])
    capsys.readouterr()
    assert ev["frames"] == 3 and np.isfinite(ev["mpjpe"])
    assert np.isfinite(res["path_mpjpe"]) and len(res["path"]) == 3 == len(res["path_info"])
    # driving VolumeViterbi by hand on the same volumes gives the same joints, bit for bit
    from sceneego_amd import load_config as load
    runner = run_sequence.SequenceRunner(load(str(cfg_path)), weights="synthetic")
    images, _, depths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    v = runner.net.volume_path(sigma=0.1, radius=None, floor=1e-3)
    for i in range(0, 3, 2):
        img = runner._images([JpegFile(p) for p in images[i:i + 2]])
        depth = runner._depths(depths[i:i + 2])
        with torch.no_grad():
            kp, _, vol, _ = runner.net(img, runner.net.grid_coord_proj_batch, runner.net.coord_volumes, depth_map_batch=depth)
        v.push(vol, joints=kp)
    by_hand = v.finish()["joints"].cpu().numpy()
    assert len(by_hand) == 3 and all(same_bits(a, b) for a, b in zip(by_hand, path))
