"""GPU: the smoother, the transition statistics, the Viterbi pass, the most probable pose, the runner-up poses and the edge statistics
over the part of their documented domain (include/sceneego_hip.h) that their own test files never enter: odd grids, G = 2 and 3, R = 16
below 128^3, the second column tile, J = 32 and a tree of depth 31, R = 24, bases that are only 4-byte aligned (the first executions of
vs_finish_kernel<false> and, at a small grid, of ts_finish_kernel<false>), and for all of them the memory contract: every output and the
exactly sized scratch lie between guard bands, every input between NaN bands (tests/volume_domain_cases.py: guarded, nan_banded), and the
bands are checked after each launch.  Every launch here is at _lib level.

INPUTS.  Those of tests/sequence_domain_cases.py, softmaxed ON THE HOST (volume_filter_cases.softmax32) and copied: the arrays that
tests/test_sequence_domain_host.py has already put through the models on the CPU.  The forward pass behind the smoother and the
statistics is se_volume_filter_f32 on the device; its float32 beliefs and flags go to the kernel and to the model alike.

TOLERANCES.  None is new and none is measured.  The Viterbi pass, its walk and refinement, the pose, the runner-up poses and the
stand-alone maxima are compared BIT FOR BIT.  The others go through the operator's own bound function, imported from its test file;
the chain lengths those bounds rest on were derived for particular grids and are derived again here for the grids of these cases
(W the power of two >= G, RP = 256 / W thread rows):
  smoother    test_gpu_volume_smoother.check_against_model: gamma, r within 2 k e1 want + 2^-90, agreement 2 k e1, joints max(2 k e1,
              (L + 2) u) sum gamma |c|, e1 = (6 R + 20 + L) u, k the backward steps behind the frame.  L = _lib.SMOOTH_CHAIN = 80 was
              derived for G = 128: a thread of vs_update_kernel owns column k and the slab rows ir, ir + RP, ...: ceil(G / RP) terms, then
              6 + 2 (workgroup), lane l of the finish pass adds records l and l + 64 (2) and the lanes fold by a butterfly (6).
              G = 127: W = 128, RP = 2, 64 terms: 64 + 6 + 2 + 2 + 6 = 80.  G = 17: W = 32, RP = 8, 3 terms; G = 2, 3, 5, 9: W = 2..16,
              RP >= 16 > G, 1 term; one record per lane below 65: at most 3 + 6 + 2 + 1 + 6 = 18 <= 80.  (G = 65: 33 + 6 + 2 + 2 + 6 = 49.)
              The scalar finish pass divides each element by the same s and S as the vector pass: no term is added.
  statistics  test_gpu_motion_fit.check_case: (e_s + 2 k e1) want + 2^-60, e_s = (6 R + 8 + L) u, L = _lib.STATS_CHAIN = 80: s, S, A0,
              A2, Bsum are sums of ts_update_kernel over the same threads, records and folds as the smoother's (above); Rsum is the sum
              of ts_blur_kj_kernel over the rows jr, jr + RP, ... of an i-plane, ceil(G / RP) terms again, one record per plane, the
              same two folds: 80 at G = 127 (where the k-blurred planes are formed by halves of 64 and 63 columns: a column's values do not
              depend on the split, and Rsum is taken before it), at most 18 at G <= 17.
  edge stats  test_gpu_skeleton_fit.compare_stats: B_fit = belief_bound(parents, R) + (T(R) + M + 2) u.  belief_bound rests on L =
              _lib.SKELETON_SUM_CHAIN = 142, derived for 128^3: CH = min(64, ceil(N / 256)) chunks of ceil(N / CH) values, a thread adds
              ceil(chunk / 256) of them, then 6 + 2 + 6: 126 + 14 at 127^3 (chunk 32006), 17 + 14 at 65^3 (chunk 4292), 1 + 14 at 2^3..9^3
              (CH = 1..3, chunks of at most 256).  M = _lib.MOMENT_CHAIN(G) = 4 + 6 + 2 + ceil(records / 64) + 6 with G ceil(G / 16)
              ceil(G / 64) records per row is a function of G and is taken from _lib at the case's own grid: 19 at G = 3, 5, 9 (one lane
              holds every record), 29 at 65 (650 records), 31 at 80, 50 at 127 (2032 records) and at 128.
  moments     test_gpu_skeleton_fit.check_moments: (T(R) + M + 2) u want, against the FFT form of the model from 64^3 up.
  maxima      bit for bit at all of volume_domain_cases.correlate_voxels(G) under thin shells and at every voxel at 127^3 and 9^3; under
              the full-length shells of (80, 24) and (128, 20) at 12,288 voxels sampled from it plus the tile seams
              (sequence_domain_cases.full_voxels: the direct model over 19,000 taps would take 9 s and 80 s a row for all of it).
A launch through the Python classes uses buffers the class allocates and cannot be guarded; they are out of scope here."""
import functools

import numpy as np
import pytest
import torch

import sequence_domain_cases as S
import test_gpu_motion_fit as TM
import test_gpu_skeleton_alternatives as TA
import test_gpu_skeleton_fit as TF
import test_gpu_skeleton_pose as TP
import test_gpu_skeleton_prior as TK
import test_gpu_volume_smoother as TS
import test_gpu_volume_viterbi as TV
import volume_domain_cases as D
from motion_fit_model import transition_stats_model
from sceneego_amd import _lib
from skeleton_alternatives_model import skeleton_alternatives_model
from skeleton_pose_model import shell_max, shell_max_at, skeleton_pose_model
from test_gpu_volume_domain import DEV, F32, I32, U8, Guards, all_same, dev, same_bits
from volume_smoother_model import volume_smoother_model
from volume_viterbi_model import refine_model

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NAN = float("nan")


def banded(a, offset=0, shape=None):
    """An input between NaN bands; ``shape``: the view handed to the wrapper (default: flat)."""
    v = D.nan_banded(a, offset, DEV)
    return v if shape is None else v.view(shape)


def host(t, shape=None):
    a = t.cpu().numpy()
    return a if shape is None else a.reshape(shape)


def same_values(got, want):
    """Bit-equal dicts or tuples of arrays; NaN cells only have to be NaN on both sides."""
    pairs = list(zip(got, want)) if isinstance(got, tuple) else [(got[key], want[key]) for key in got]
    return all(TA.same_values(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in pairs)


# ================================================================================================================== 1. sequences
@functools.lru_cache(maxsize=None)
def sequence_dev(rows, G, R, floor, T):
    """filter_inputs, plain device copies of them and the forward pass se_volume_filter_f32 taken once (nothing modifies them)."""
    k = dict(S.filter_inputs(rows, G, R, T))
    k.update(prob=dev(k["p"]), coord=dev(k["c"]), taps_dev=dev(k["taps"]))
    k["belief"], k["restarted"] = TS.forward(k["prob"], k["coord"], k["taps_dev"], G, R, floor)
    k["b"], k["rs"] = k["belief"].cpu().numpy(), k["restarted"].cpu().numpy()
    return k


def chunks_of(T, cuts):
    cuts = (T,) if cuts is None else tuple(cuts)
    assert sum(cuts) == T
    starts = np.concatenate([[0], np.cumsum(cuts)]).tolist()
    return [(starts[i], starts[i + 1]) for i in range(len(cuts) - 1, -1, -1)]          # issued last chunk first


def smooth_guarded(prob, belief, restarted, coord, taps_dev, G, R, floor, cuts=None, out="new", offsets=None):
    """test_gpu_volume_smoother.smooth with every output and the exactly sized scratch between guard bands and every input between NaN
    bands; ``offsets`` {prob, belief, state, smoothed_out, scratch: bytes} moves the named buffers off their alignment."""
    off = offsets or {}
    T, rows, N = prob.shape
    g = Guards(f"volume_smooth rows {rows} G {G} R {R} out {out} offsets {off}")
    pd = banded(prob, off.get("prob", 0), (T, rows, N))
    if out == "inplace":
        bel = g.out(T * rows * N, F32, off.get("belief", 0)).view(T, rows, N)
        bel.copy_(belief)
    else:
        bel = banded(belief, off.get("belief", 0), (T, rows, N))
    rs, cd, td = banded(restarted, 0, (T, rows)), banded(coord), banded(taps_dev)
    gamma = bel if out == "inplace" else g.out(T * rows * N, F32, off.get("smoothed_out", 0)).view(T, rows, N) if out == "new" else None
    state = g.out(rows * N, F32, off.get("state", 0))
    state.fill_(NAN)
    joints, agreement = g.out(T * rows * 3, F32).view(T, rows, 3), g.out(T * rows, F32).view(T, rows)
    smoothed = g.out(T * rows, I32).view(T, rows)
    scratch = g.out(_lib.volume_smooth_scratch_bytes(rows, G, R), U8, off.get("scratch", 0))
    for name, t in (("prob", pd), ("belief", bel), ("state", state), ("smoothed_out", None if out == "inplace" else gamma), ("scratch", scratch)):
        assert t is None or t.data_ptr() % 16 == off.get(name, 0) % 16
    r = {}
    for t0, t1 in chunks_of(T, cuts):
        link = None if t1 == T else banded((rs[t1] == 0).to(torch.int32))
        _lib.volume_smooth(pd[t0:t1], bel[t0:t1], rs[t0:t1], cd, td, state, None if gamma is None else gamma[t0:t1], joints[t0:t1],
                           agreement[t0:t1], smoothed[t0:t1], t1 - t0, rows, N, G, R, floor, have_link=link, scratch=scratch)
        g.check()
        r[t0] = host(state, (rows, N))
    return {"gamma": None if gamma is None else host(gamma), "joints": host(joints), "agreement": host(agreement),
            "smoothed": host(smoothed), "state": host(state, (rows, N)), "r": r}


def stats_guarded(prob, belief, restarted, taps_dev, G, R, floor, cuts=None, offsets=None):
    """test_gpu_motion_fit.stats_pass, guarded as smooth_guarded; ``offsets`` {prob, belief, state, scratch: bytes}."""
    off = offsets or {}
    T, rows, N = prob.shape
    g = Guards(f"volume_transition_stats rows {rows} G {G} R {R} offsets {off}")
    pd, bel = banded(prob, off.get("prob", 0), (T, rows, N)), banded(belief, off.get("belief", 0), (T, rows, N))
    rs, td = banded(restarted, 0, (T, rows)), banded(taps_dev)
    state = g.out(rows * N, F32, off.get("state", 0))
    state.fill_(NAN)
    stats, linked = g.out(T * rows * 6, F32).view(T, rows, 6), g.out(T * rows, I32).view(T, rows)
    scratch = g.out(_lib.volume_transition_stats_scratch_bytes(rows, G, R), U8, off.get("scratch", 0))
    r = {}
    for t0, t1 in chunks_of(T, cuts):
        link = None if t1 == T else banded((rs[t1] == 0).to(torch.int32))
        _lib.volume_transition_stats(pd[t0:t1], bel[t0:t1], rs[t0:t1], td, state, stats[t0:t1], linked[t0:t1], t1 - t0, rows, N, G, R,
                                     floor, have_link=link, scratch=scratch)
        g.check()
        r[t0] = host(state, (rows, N))
    return {"stats": host(stats), "linked": host(linked), "state": host(state, (rows, N)), "r": r}


def same_run(a, b, keys):
    return all(a[key] is b[key] is None or same_bits(a[key], b[key]) for key in keys)


SMOOTH_KEYS = ("gamma", "joints", "agreement", "smoothed", "state")


# ------------------------------------------------------------------------------------------------------------------ the smoother
@pytest.mark.parametrize("rows,G,R,floor,T", S.SEQUENCE_CASES)
def test_smoother_against_the_model(rows, G, R, floor, T):
    """check_against_model cuts the sequence frame by frame and takes it whole, bit-equal, and holds both to the model; then
    smoothed_out in place over belief and None, and the launch into plain tensors."""
    k = sequence_dev(rows, G, R, floor, T)
    TS.check_against_model(k, G, R, floor, k["taps"], k["taps_dev"], f"smoother rows {rows} G {G} R {R} floor {floor}", smooth=smooth_guarded)
    args = (k["prob"], k["belief"], k["restarted"], k["coord"], k["taps_dev"], G, R, floor)
    new = smooth_guarded(*args)
    inplace, none = smooth_guarded(*args, cuts=(1, T - 1), out="inplace"), smooth_guarded(*args, out=None)
    assert same_run(inplace, new, SMOOTH_KEYS) and none["gamma"] is None and same_run(none, new, SMOOTH_KEYS[1:])
    assert same_bits(k["belief"].cpu().numpy(), k["b"])
    assert same_run(TS.smooth(*args), new, SMOOTH_KEYS), "the guarded launch and the launch into plain tensors differ"


def test_smoother_alignment_does_not_change_a_bit():
    """An even grid with whole quads, so that vs_finish_kernel<true> runs when every base is 16-byte aligned and vs_finish_kernel<false>
    when prob, belief, state, smoothed_out or scratch starts 4 bytes into its buffer: both divide each element by the same s and S."""
    rows, G, R, floor, T = S.SEQUENCE_ALIGN_CASE
    k = sequence_dev(rows, G, R, floor, T)
    TS.check_against_model(k, G, R, floor, k["taps"], k["taps_dev"], "smoother, every base aligned", smooth=smooth_guarded)
    args = (k["prob"], k["belief"], k["restarted"], k["coord"], k["taps_dev"], G, R, floor)
    base = smooth_guarded(*args)
    names = ("prob", "belief", "state", "smoothed_out", "scratch")
    for moved in [(n,) for n in names] + [names]:
        offsets = {n: 4 for n in moved}
        got = smooth_guarded(*args, offsets=offsets)
        assert same_run(got, base, SMOOTH_KEYS), f"offset {moved}: the results differ from the aligned launch"
        TS.check_against_model(k, G, R, floor, k["taps"], k["taps_dev"], f"smoother, {'+'.join(moved)} offset by 4 bytes",
                               smooth=functools.partial(smooth_guarded, offsets=offsets))
    for moved in (("belief",), ("belief", "scratch")):                       # in place: belief is the output
        got = smooth_guarded(*args, out="inplace", offsets={n: 4 for n in moved})
        assert same_run(got, base, SMOOTH_KEYS), f"in place, offset {moved}"
    assert same_run(smooth_guarded(*args, out=None, offsets={"state": 4}), base, SMOOTH_KEYS[1:])


def test_smoother_nan_frame_cuts_the_chain_on_the_scalar_path():
    rows, G, R, floor, T = S.SMOOTHER_NAN_CASE
    k = sequence_dev(rows, G, R, floor, T)
    clean = smooth_guarded(k["prob"], k["belief"], k["restarted"], k["coord"], k["taps_dev"], G, R, floor)
    prob = k["prob"].clone()
    prob[2, 1] = NAN                                                         # the filter restarts row 1 at frames 2 and 3
    belief, restarted = TS.forward(prob, k["coord"], k["taps_dev"], G, R, floor)
    p, b, rs = prob.cpu().numpy(), belief.cpu().numpy(), restarted.cpu().numpy()
    assert rs[:, 1].tolist() == [1, 0, 1, 1]
    want = volume_smoother_model(p, b, rs, k["c"], k["taps"], G, floor)
    assert want["smoothed"][:, 1].tolist() == [True, False, False, False]
    got = smooth_guarded(prob, belief, restarted, k["coord"], k["taps_dev"], G, R, floor, cuts=(3, 1))
    assert np.array_equal(got["smoothed"] != 0, want["smoothed"])
    for t in (1, 2, 3):                                                      # not linked: copies, bit for bit (frame 2: all NaN)
        assert same_bits(got["gamma"][t, 1], b[t, 1]) and np.isnan(got["agreement"][t, 1])
    assert np.isnan(got["gamma"][2, 1]).all() and np.isnan(got["joints"][2, 1]).all() and np.isfinite(got["state"]).all()
    for t in (0, 1, 3):
        assert np.isfinite(got["gamma"][t, 1]).all() and np.isfinite(got["joints"][t, 1]).all()
    err = np.abs(got["gamma"][0, 1].astype(np.float64) - want["gamma"][0, 1])        # one backward step behind frame 0
    assert (err <= 2 * TS.e1(R) * want["gamma"][0, 1] + 2.0 ** -90).all()
    head = smooth_guarded(prob[:2], belief[:2], restarted[:2], k["coord"], k["taps_dev"], G, R, floor)
    assert same_bits(got["gamma"][:2, 1], head["gamma"][:, 1]) and same_bits(got["state"][1], head["state"][1])
    for key in ("gamma", "joints", "agreement"):
        assert same_bits(got[key][:, [0, 2]], clean[key][:, [0, 2]]), key
    assert same_bits(got["state"][[0, 2]], clean["state"][[0, 2]])


# ------------------------------------------------------------------------------------------------------------------ the statistics
@pytest.mark.parametrize("rows,G,R,floor,T", S.SEQUENCE_CASES)
def test_transition_stats_against_the_model_and_the_smoother(rows, G, R, floor, T):
    k = sequence_dev(rows, G, R, floor, T)
    TM.check_case(k, rows, G, R, floor, T, stats_pass=stats_guarded, smooth=smooth_guarded)
    args = (k["prob"], k["belief"], k["restarted"], k["taps_dev"], G, R, floor)
    assert same_run(TM.stats_pass(*args), stats_guarded(*args), ("stats", "linked", "state")), "guarded and plain launches differ"


def test_transition_stats_alignment_does_not_change_a_bit():
    """ts_finish_kernel<false> at a shape where ts_finish_kernel<true> gives the answer to compare with: prob, state or scratch 4 bytes
    off takes the scalar pass.  The finish pass does not touch belief, so an offset belief alone stays on the vector pass; it is
    there for the 4-byte promise of the header (the update pass reads it)."""
    rows, G, R, floor, T = S.SEQUENCE_ALIGN_CASE
    k = sequence_dev(rows, G, R, floor, T)
    args = (k["prob"], k["belief"], k["restarted"], k["taps_dev"], G, R, floor)
    base = stats_guarded(*args)
    want = transition_stats_model(k["p"], k["b"], k["rs"], k["taps"], G, floor)
    names = ("prob", "belief", "state", "scratch")
    for moved in [(n,) for n in names] + [names]:
        got = stats_guarded(*args, offsets={n: 4 for n in moved})
        assert same_run(got, base, ("stats", "linked", "state")), f"offset {moved}: the results differ from the aligned launch"
        worst = TM.check_stats(got["stats"], want, R, f"statistics, {'+'.join(moved)} offset by 4 bytes")
        print(f"statistics, {'+'.join(moved)} offset by 4 bytes: bound {TM.stat_bound(want['linked'], R).max() / U:.0f} u; worst (units of "
              f"2^-24) " + ", ".join(f"{n} {v:.1f}" for n, v in worst.items()))
    sm = smooth_guarded(k["prob"], k["belief"], k["restarted"], k["coord"], k["taps_dev"], G, R, floor, out=None, offsets={"state": 4})
    assert same_bits(base["state"], sm["state"]) and same_bits(base["stats"][..., 0], sm["agreement"])


def test_transition_stats_chunked_against_whole_at_an_odd_grid():
    rows, G, R, floor, T = S.STATS_CUT_CASE
    k = sequence_dev(rows, G, R, floor, T)
    args = (k["prob"], k["belief"], k["restarted"], k["taps_dev"], G, R, floor)
    runs = [stats_guarded(*args, cuts=cuts) for cuts in ((4,), (1, 3), (2, 2), (1, 1, 1, 1))]
    for other in runs[1:]:
        assert same_run(other, runs[0], ("stats", "linked", "state"))
    assert same_bits(runs[2]["r"][2], runs[3]["r"][2])


# ------------------------------------------------------------------------------------------------------------------ Viterbi
def viterbi_guarded(p, taps, G, R, floor, cuts=None, states=False, offsets=None):
    """test_gpu_volume_viterbi.forward on the host array ``p`` [T, rows, N], guarded; ``offsets`` {prob, state, back_out, scratch: bytes}."""
    off = offsets or {}
    T, rows, N = p.shape
    cuts = (T,) if cuts is None else tuple(cuts)
    assert sum(cuts) == T
    g = Guards(f"volume_viterbi rows {rows} G {G} R {R} cuts {cuts} offsets {off}")
    pd, td = banded(p, off.get("prob", 0), (T, rows, N)), banded(taps)
    state = g.out(rows * N, F32, off.get("state", 0))
    state.fill_(NAN)
    peak_state, best_state = g.out(rows, I32), g.out(rows, F32)
    back = g.out(T * rows * N, I32, off.get("back_out", 0)).view(T, rows, N)
    peak, exponent, restarted = (g.out(T * rows, I32).view(T, rows) for _ in range(3))
    best = g.out(T * rows, F32).view(T, rows)
    scratch = g.out(_lib.volume_viterbi_scratch_bytes(rows, G, R), U8, off.get("scratch", 0))
    ones = torch.ones(rows, device=DEV, dtype=torch.int32)
    t, after = 0, []
    for n in cuts:
        _lib.volume_viterbi(pd[t:t + n], td, state, peak_state, best_state, back[t:t + n], peak[t:t + n], best[t:t + n], exponent[t:t + n],
                            restarted[t:t + n], n, rows, N, G, R, floor, have_prior=None if t == 0 else ones, scratch=scratch)
        g.check()
        if states:
            after.append(host(state, (rows, N)))
        t += n
    out = {"back": host(back), "peak": host(peak), "best": host(best), "exponent": host(exponent), "restarted": host(restarted),
           "state": host(state, (rows, N)), "after": after, "dev": {"back": back, "peak": peak, "restarted": restarted}}
    assert np.array_equal(host(peak_state), out["peak"][-1]) and TA.same_values(host(best_state), out["best"][-1])
    return out


def walk_guarded(d, cuts=None):
    """test_gpu_volume_viterbi.walk, guarded: (index on the device, index, jumped on the host)."""
    back, peak, restarted = d["back"], d["peak"], d["restarted"]
    T, rows, N = back.shape
    g = Guards(f"volume_viterbi_path rows {rows} voxels {N} cuts {cuts}")
    cursor, index, jumped = g.out(rows, I32), g.out(T * rows, I32).view(T, rows), g.out(T * rows, I32).view(T, rows)
    for t0, t1 in chunks_of(T, cuts):
        _lib.volume_viterbi_path(back[t0:t1], peak[t0:t1], restarted[t0:t1], cursor, index[t0:t1], jumped[t0:t1], t1 - t0, rows, N,
                                 have_next=int(t1 != T))
        g.check()
    return index, host(index), host(jumped)


def refine_guarded(p, c, index, G, r):
    T, rows, N = p.shape
    g = Guards(f"volume_viterbi_refine rows {rows} G {G} refine {r}")
    joints = g.out(T * rows * 3, F32)
    _lib.volume_viterbi_refine(banded(p) if r > 0 else None, banded(c), index.reshape(-1), joints, T, rows, N, G, r)
    g.check()
    return host(joints, (T, rows, 3))


def check_walk(got, want, label, cuts=None):
    """The guarded back-walk over the device arrays of ``viterbi_guarded`` against the model's path; returns the index on the device."""
    index_dev, index, jumped = walk_guarded(got["dev"], cuts)
    assert np.array_equal(index, want["index"]) and np.array_equal(jumped != 0, want["jumped"]), label
    assert set(np.unique(jumped)) <= {0, 1}
    return index_dev


@pytest.mark.parametrize("rows,G,R,floor,T", S.SEQUENCE_CASES)
def test_viterbi_against_the_model_bit_for_bit(rows, G, R, floor, T):
    k = S.filter_inputs(rows, G, R, T)
    want = S.viterbi_want(rows, G, R, floor, T)
    S.viterbi_condition(want)
    label = f"viterbi rows {rows} G {G} R {R} floor {floor}"
    one = viterbi_guarded(k["p"], k["taps"], G, R, floor, cuts=(1,) * T, states=True)      # frame by frame: the state of every frame
    TV.check_forward(one, want, label)
    whole = viterbi_guarded(k["p"], k["taps"], G, R, floor)
    TV.check_forward(whole, want, label + ", one call")
    index = check_walk(whole, want, label)
    for r in (0, 1, 2, 3):
        assert same_bits(refine_guarded(k["p"], k["c"], index, G, r), refine_model(k["p"], k["c"], want["index"], G, r)), f"{label}: refine {r}"
    plain = TV.forward(dev(k["p"]), dev(k["taps"]), G, R, floor)
    assert all(np.array_equal(plain[key], whole[key]) for key in ("back", "peak", "exponent", "restarted"))
    assert same_bits(plain["best"], whole["best"]) and same_bits(plain["state"], whole["state"]), "guarded and plain launches differ"
    pos = want["state"][want["state"] > 0]
    print(f"{label}: every output equal to the model (0 u); scaled scores down to {pos.min():.3g}, {int((want['state'] == 0).sum())} exact "
          f"zeros, exponents {want['exponent'].min()}..{want['exponent'].max()}, {int(want['jump_bits'].sum())} back-pointers with the jump bit")


@pytest.mark.parametrize("rows,G,R,floor,T", S.SEQUENCE_CUT_CASES)
def test_viterbi_cuts_at_odd_grids(rows, G, R, floor, T):
    k = S.filter_inputs(rows, G, R, T)
    want = S.viterbi_want(rows, G, R, floor, T)
    runs = [viterbi_guarded(k["p"], k["taps"], G, R, floor, cuts=cuts) for cuts in ((T,), (1,) * T, (1, T - 1), (T - 1, 1))]
    for other in runs[1:]:
        assert all(np.array_equal(runs[0][key], other[key]) for key in ("back", "peak", "exponent", "restarted"))
        assert same_bits(runs[0]["best"], other["best"]) and same_bits(runs[0]["state"], other["state"])
    for cuts in ((T,), (1,) * T, (2, T - 2)):
        check_walk(runs[0], want, f"walk cut {cuts}", cuts)
    # ... and no base has to be more than 4-byte aligned
    for moved in ("prob", "state", "back_out", "scratch"):
        got = viterbi_guarded(k["p"], k["taps"], G, R, floor, offsets={moved: 4})
        assert np.array_equal(got["back"], runs[0]["back"]) and same_bits(got["state"], runs[0]["state"]) and same_bits(got["best"], runs[0]["best"])


def test_viterbi_takes_a_jump_at_an_odd_grid():
    G, R, floor = S.VITERBI_JUMP_CASE
    k = S.viterbi_jump_inputs()
    want = k["m"]
    assert want["jumped"][2].all() and not want["tied"].any()
    got = viterbi_guarded(k["p"], k["taps"], G, R, floor, cuts=(2, 2), states=True)
    for key in ("back", "peak", "exponent"):
        assert np.array_equal(got[key], want[key]), key
    assert same_bits(got["best"], want["best"]) and same_bits(got["after"][0], want["state"][1]) and same_bits(got["state"], want["state"][3])
    for cuts in ((4,), (2, 2), (1, 3), (3, 1), (1, 1, 1, 1)):                # the jump crosses a chunk boundary of the walk in some of these
        check_walk(got, want, f"jump, walk cut {cuts}", cuts)


def test_viterbi_nan_cell_and_nan_frame_at_an_odd_grid():
    rows, G, R, floor, T = S.VITERBI_NAN_CASE
    k = S.viterbi_nan_inputs()
    c = S.filter_inputs(rows, G, R, T)["c"]
    p, want = k["p"], k["m"]
    got = viterbi_guarded(p, k["taps"], G, R, floor, cuts=(2, 1, 1), states=True)
    for key in ("back", "peak", "exponent"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["restarted"] != 0, want["restarted"]) and TA.same_values(got["best"], want["best"])
    assert np.isnan(got["best"][2, 3]) and got["exponent"][2, 3] == 0 and (got["back"][2:4, 3] == -1).all()
    assert same_bits(got["after"][1][3], p[2, 3]) and np.isnan(got["after"][0][1, 60])      # the copy of p; the NaN score of the one cell
    for i, t in enumerate((1, 2, 3)):
        assert TA.same_values(got["after"][i], want["state"][t]), t
    index = check_walk(got, want, "NaN cell and frame", (2, 1, 1))
    joints = refine_guarded(p, c, index, G, 1)
    assert TA.same_values(joints, refine_model(p, c, want["index"], G, 1))
    assert np.isnan(joints[2, 3]).all() and np.isfinite(np.delete(joints, 3, axis=1)).all()
    clean = S.viterbi_want(rows, G, R, floor, T)
    assert np.array_equal(got["back"][:, [0, 2]], clean["back"][:, [0, 2]])


# ================================================================================================================== 2. skeletons
@functools.lru_cache(maxsize=None)
def tree_dev(frames, tree, G, R):
    k = dict(S.skeleton_inputs(frames, tree, G, R))
    k.update(prob=dev(k["p"]), coord=dev(k["c"]), taps_dev=dev(k["taps"]))
    return k


POSE_OUT = (("index", I32, 1), ("jumped", I32, 1), ("exponent", I32, 1), ("best_root", F32, 0), ("solved", I32, 0))


def pose_guarded(k, G, R, floor, offsets=None, frames=None, p=None):
    """One guarded _lib-level call over the frames ``frames`` (a slice; default all) of ``p`` (default the case's volumes): host arrays
    as test_gpu_skeleton_pose.launch returns them.  ``offsets`` {prob, scratch, <output>: bytes}."""
    off = offsets or {}
    p = k["p"] if p is None else p
    p = p if frames is None else p[frames]
    F, J, N = p.shape
    g = Guards(f"skeleton_pose frames {F} J {J} G {G} R {R} offsets {off}")
    outs = {name: g.out(F * J if per_joint else F, dtype, off.get(name, 0)) for name, dtype, per_joint in POSE_OUT}
    scratch = g.out(_lib.skeleton_pose_scratch_bytes(F, J, G, R), U8, off.get("scratch", 0))
    _lib.skeleton_pose(banded(p, off.get("prob", 0)), banded(k["taps"]), k["parents"], **outs, frames=F, voxels=N, grid=G, radius=R,
                       floor=floor, scratch=scratch)
    g.check()
    return tuple(host(outs[name], (F, J) if per_joint else (F,)) for name, _, per_joint in POSE_OUT)


def alternatives_guarded(k, G, R, floor, separation, offsets=None, frames=None, p=None, volumes=True):
    """The same for se_skeleton_alternatives_f32: a dict as test_gpu_skeleton_alternatives.launch returns it."""
    off = offsets or {}
    p = k["p"] if p is None else p
    p = p if frames is None else p[frames]
    F, J, N = p.shape
    g = Guards(f"skeleton_alternatives frames {F} J {J} G {G} R {R} separation {separation} offsets {off}")
    shape = {"solved": (F,), "complete": (F,), "best_root": (F,), "alt_pose": (F, J, J), "alt_jumped": (F, J, J)}
    outs = {}
    for key in TA.INT_KEYS + TA.FLOAT_KEYS:
        outs[key] = g.out(int(np.prod(shape.get(key, (F, J)))), I32 if key in TA.INT_KEYS else F32, off.get(key, 0))
    outs["max_marginals"] = g.out(F * J * N, F32, off.get("max_marginals", 0)) if volumes else None
    shape["max_marginals"] = (F, J, N)
    scratch = g.out(_lib.skeleton_alternatives_scratch_bytes(F, J, G, R), U8, off.get("scratch", 0))
    _lib.skeleton_alternatives(banded(p, off.get("prob", 0)), banded(k["taps"]), k["parents"], separation, frames=F, voxels=N, grid=G,
                               radius=R, floor=floor, scratch=scratch, **outs)
    g.check()
    return {key: host(v, shape.get(key, (F, J))) for key, v in outs.items() if v is not None}


def edge_stats_guarded(k, blocks, G, R, floor, offsets=None, frames=None):
    """The same for se_skeleton_edge_stats_f32: (stats, norms, valid) as test_gpu_skeleton_fit.edge_stats returns them."""
    off = offsets or {}
    p = k["p"] if frames is None else k["p"][frames]
    F, J, N = p.shape
    g = Guards(f"skeleton_edge_stats frames {F} J {J} G {G} R {R} offsets {off}")
    stats, norms, valid = g.out(F * J * 4, F32, off.get("stats", 0)), g.out(F * J * 3, F32, off.get("norms", 0)), g.out(F, I32, off.get("valid", 0))
    scratch = g.out(_lib.skeleton_edge_stats_scratch_bytes(F, J, G, R), U8, off.get("scratch", 0))
    _lib.skeleton_edge_stats(banded(p, off.get("prob", 0)), banded(blocks[0]), banded(blocks[1]), banded(blocks[2]), k["parents"], stats,
                             norms, valid, F, N, G, R, floor, scratch=scratch)
    g.check()
    return host(stats, (F, J, 4)), host(norms, (F, J, 3)), host(valid)


# ------------------------------------------------------------------------------------------------------------------ the pose
@pytest.mark.parametrize("frames,tree,G,R,floor", S.TREE_CASES)
def test_pose_against_the_model_bit_for_bit(frames, tree, G, R, floor):
    k = tree_dev(frames, tree, G, R)
    want = S.pose_want(frames, tree, G, R, floor)
    assert want["solved"].all()
    got = pose_guarded(k, G, R, floor)
    TP.equals_model(got, want)
    assert all_same(got, TP.launch(k["prob"], k["taps_dev"], k["parents"], G, R, floor)), "guarded and plain launches differ"
    if G > 64:
        # The pose lies in the first column tile (k = 45..47 at 127^3), so no output depends on a message of the second one.  Mirrored
        # along k it lies there, and the model mirrors exactly (tests/test_sequence_domain_host.py): the same values, the mirrored voxels.
        mirror = pose_guarded(k, G, R, floor, p=S.mirrored_k(k["p"], G))
        assert np.array_equal(mirror[0], S.mirrored_index(want["index"], G)) and all(same_bits(a, b) for a, b in zip(mirror[1:], got[1:]))
    print(f"pose frames {frames} {tree} G {G} R {R} floor {floor}: every output equal to the model (0 u); jumps {int(got[1].sum())}, log "
          f"score {want['log_score'].round(3).tolist()}")


def test_pose_batching_at_an_odd_grid():
    """Five frames in one call walk a group of four and a group of one: 5 = 1 + 4 = 5 singles, bit for bit."""
    frames, tree, G, R, floor = S.TREE_BATCH_CASE
    k = tree_dev(frames, tree, G, R)
    five = pose_guarded(k, G, R, floor)
    TP.equals_model(five, S.pose_want(frames, tree, G, R, floor))
    parts = [pose_guarded(k, G, R, floor, frames=slice(0, 1)), pose_guarded(k, G, R, floor, frames=slice(1, 5))]
    singles = [pose_guarded(k, G, R, floor, frames=slice(f, f + 1)) for f in range(frames)]
    for x in range(5):
        assert same_bits(np.concatenate([q[x] for q in parts]), five[x]) and same_bits(np.concatenate([q[x] for q in singles]), five[x]), x


def test_pose_fallback_and_nan_cell_at_an_odd_grid():
    frames, tree, G, R, floor = S.TREE_FALLBACK_CASE
    k = tree_dev(frames, tree, G, R)
    p = S.fallback_inputs()
    want = skeleton_pose_model(p, k["taps"], k["parents"], G, floor)
    assert want["solved"].tolist() == [False, True]
    got = pose_guarded(k, G, R, floor, p=p)
    TP.equals_model(got, want)
    clean = pose_guarded(k, G, R, floor)
    assert all(same_bits(a[1:], b[1:]) for a, b in zip(got, clean))          # the NaN cell lies off the pose: nothing changes
    alt_want = skeleton_alternatives_model(p, k["taps"], k["parents"], G, floor, 1)
    assert alt_want["complete"].tolist() == [False, True]
    TA.equals_model(alternatives_guarded(k, G, R, floor, 1, p=p), alt_want)


# ------------------------------------------------------------------------------------------------------------------ the alternatives
@pytest.mark.parametrize("frames,tree,G,R,floor", S.ALTERNATIVES_CASES)
def test_alternatives_against_the_model_bit_for_bit(frames, tree, G, R, floor):
    k = tree_dev(frames, tree, G, R)
    pose = pose_guarded(k, G, R, floor)
    for sep in S.separations(G):
        want = S.alternatives_want(frames, tree, G, R, floor, sep)
        assert want["solved"].all() and want["complete"].all()
        got = alternatives_guarded(k, G, R, floor, sep)
        TA.equals_model(got, want)
        for key, ref in zip(("index", "jumped", "exponent", "best_root", "solved"), pose):       # the upward outputs: the pose call's
            assert same_bits(got[key], ref), key
        if sep == G - 1:
            assert (got["alt_index"] == -1).all() and (got["alt_pose"] == -1).all() and (got["alt_value"] == 0).all()
        print(f"alternatives frames {frames} {tree} G {G} R {R} floor {floor} separation {sep}: every output equal to the model (0 u); "
              f"{int((got['alt_index'] >= 0).sum())} of {got['alt_index'].size} alternatives, {int(got['alt_jumped'].sum())} jumps")
    none = alternatives_guarded(k, G, R, floor, 1, volumes=False)
    assert same_values(none, {key: S.alternatives_want(frames, tree, G, R, floor, 1)[key].astype(none[key].dtype) for key in none})


# ------------------------------------------------------------------------------------------------------------------ the edge statistics
@pytest.mark.parametrize("frames,tree,G,R,floor", S.EDGE_CASES)
def test_edge_stats_against_the_model_and_the_coupling(frames, tree, G, R, floor):
    k = tree_dev(frames, tree, G, R)
    blocks = S.edge_blocks(frames, tree, G, R)
    want = S.edge_want(frames, tree, G, R, floor)
    S.edge_condition(want, blocks, G, floor)
    got = edge_stats_guarded(k, blocks, G, R, floor)
    TF.compare_stats(got, want, k["parents"], G, R, floor, f"edge stats frames {frames} {tree} G {G} R {R} floor {floor}")
    _, _, evidence, coupled = TK.launch(k["prob"], k["coord"], k["taps_dev"], k["parents"], G, R, floor, beliefs=False)
    assert same_bits(got[1][:, :, 2], evidence) and np.array_equal(got[2], coupled)
    assert all_same(got, TF.edge_stats(k["prob"], blocks, k["parents"], G, R, floor)), "guarded and plain launches differ"
    if frames == 5:                                                          # a group of four and one more, against every frame alone
        singles = [edge_stats_guarded(k, blocks, G, R, floor, frames=slice(f, f + 1)) for f in range(frames)]
        for x in range(3):
            assert same_bits(np.concatenate([q[x] for q in singles]), got[x]), x


# ------------------------------------------------------------------------------------------------------------------ alignment
def test_tree_alignment_does_not_change_a_bit():
    """prob, every output and the scratch of the three tree walks 4 bytes off their alignment, one at a time and all together."""
    frames, tree, G, R, floor = S.TREE_ALIGN_CASE
    k = tree_dev(frames, tree, G, R)
    blocks = S.edge_blocks(frames, tree, G, R)
    runs = (("pose", [n for n, _, _ in POSE_OUT], lambda o: pose_guarded(k, G, R, floor, offsets=o)),
            ("alternatives", list(TA.KEYS), lambda o: alternatives_guarded(k, G, R, floor, 1, offsets=o)),
            ("edge stats", ["stats", "norms", "valid"], lambda o: edge_stats_guarded(k, blocks, G, R, floor, offsets=o)))
    for what, outputs, run in runs:
        base = run(None)
        names = ["prob", "scratch"] + outputs
        for moved in [(n,) for n in names] + [tuple(names)]:
            assert same_values(run({n: 4 for n in moved}), base), f"{what}, offset {moved}: the results differ from the aligned launch"
    TP.equals_model(pose_guarded(k, G, R, floor), S.pose_want(frames, tree, G, R, floor))


# ================================================================================================================== 3. stand-alone
def maxcorr_guarded(a, taps, tap_row, G, R, scale, query):
    """se_shell_maxcorr_f32 over the rows of ``a`` and se_shell_argmax_i32 at the voxels ``query``, guarded: (out [rows, N], out_tap,
    out_value [rows, queries])."""
    rows, N = a.shape
    g = Guards(f"shell_maxcorr / shell_argmax rows {rows} G {G} R {R}")
    ad, td, rd = banded(a), banded(taps, 0, taps.shape), banded(np.asarray(tap_row, dtype=np.int32))
    out = g.out(rows * N, F32)
    scratch = g.out(_lib.shell_correlate_scratch_bytes(taps.shape[0], R), U8)
    _lib.shell_maxcorr(ad, td, rd, out, rows, G, R, scale_mul=float(scale), scratch=scratch)
    g.check()
    q = banded(np.asarray(query, dtype=np.int32))
    out_tap, out_value = g.out(rows * len(query), I32), g.out(rows * len(query), F32)
    _lib.shell_argmax(ad, td, rd, q, out_tap, out_value, rows, G, R)
    g.check()
    return host(out, (rows, N)), host(out_tap, (rows, len(query))), host(out_value, (rows, len(query)))


def moments_guarded(e, a, blocks, tap_row, G, R):
    rows = e.shape[0]
    g = Guards(f"shell_moments rows {rows} G {G} R {R}")
    out = g.out(rows * 3, F32)
    scratch = g.out(_lib.shell_moments_scratch_bytes(rows, blocks[0].shape[0], G, R), U8)
    _lib.shell_moments(banded(e), banded(a), banded(blocks[0], 0, blocks[0].shape), banded(blocks[1]), banded(blocks[2]),
                       banded(np.asarray(tap_row, dtype=np.int32)), out, rows, G, R, scratch=scratch)
    g.check()
    return host(out, (rows, 3))


def check_sampled_maxima(k, G, R, voxels, what):
    a, taps, rows = k["a"][1:], k["taps"], [2, 1]                            # the two children under each other's shells
    scale = np.float32(0.999)
    out, out_tap, out_value = maxcorr_guarded(a, taps, rows, G, R, scale, voxels)
    assert np.isfinite(out).all()
    for r, tr in enumerate(rows):
        e3, arg = shell_max_at(a[r], taps[tr], G, R, voxels)
        assert same_bits(out_value[r], e3) and same_bits(out[r, voxels], scale * e3) and np.array_equal(out_tap[r], arg), (what, r)
        print(f"{what} row {r}: {int(np.count_nonzero(taps[tr]))} taps, {len(voxels)} voxels ({int((voxels % G >= 64).sum())} with k >= 64): "
              f"maxima and arguments equal to the model (0 u); {int((e3 == 0).sum())} zeros")


@pytest.mark.parametrize("G,R", S.SHELL_FULL)
def test_shell_maxima_and_moments_under_full_length_shells(G, R):
    """R = 24 at 80^3 and R = 20 at 128^3, the shapes a whole tree cannot afford on the host: maxima and arguments at sampled voxels of
    the last plane, of the second column tile and of the rest; the moments against the FFT form of the model."""
    k = S.shell_inputs(G, R)
    check_sampled_maxima(k, G, R, S.full_voxels(G), f"shell maxima G {G} R {R}")
    got = moments_guarded(k["e"], k["m"], k["blocks"], k["tap_row"], G, R)
    TF.check_moments(got, k["e"], k["m"], k["blocks"], list(k["tap_row"]), G, R, f"shell moments G {G} R {R}", method="fft")


def test_shell_maxima_and_moments_under_thin_shells_in_the_deepest_tile():
    G, R, bones = S.SHELL_DEEP
    k = S.shell_inputs(G, R, bones)
    check_sampled_maxima(k, G, R, D.correlate_voxels(G), f"thin shells G {G} R {R}")
    got = moments_guarded(k["e"], k["m"], k["blocks"], k["tap_row"], G, R)
    TF.check_moments(got, k["e"], k["m"], k["blocks"], list(k["tap_row"]), G, R, f"thin-shell moments G {G} R {R}", method="fft")


def test_shell_maxima_at_every_voxel_of_the_largest_odd_grid():
    G, R = S.SHELL_ODD
    k = S.shell_inputs(G, R, (2.4, 1.6), tau_voxels=0.25)                    # thin shells: the whole-volume model takes 12 ms a tap
    a, taps = k["a"][1:2], k["taps"]
    voxels = D.correlate_voxels(G)
    out, out_tap, out_value = maxcorr_guarded(a, taps, [1], G, R, 1.0, voxels)
    e3, arg = shell_max(a[0], taps[1], G, R)
    assert same_bits(out[0], e3) and same_bits(out_value[0], e3[voxels]) and np.array_equal(out_tap[0], arg[voxels])
    print(f"shell maxima G {G} R {R}: {int(np.count_nonzero(taps[1]))} taps, every voxel equal to the model (0 u)")
    got = moments_guarded(k["e"], k["m"], k["blocks"], k["tap_row"], G, R)
    TF.check_moments(got, k["e"], k["m"], k["blocks"], list(k["tap_row"]), G, R, f"shell moments G {G} R {R}", method="fft")


def test_shell_maxima_at_every_voxel_of_a_small_odd_grid():
    """The five rows of test_gpu_skeleton_pose.shell_rows at 9^3 with R = 8 = G - 1: random, uniform, subnormals and exact zeros, NaN
    cells, a tap row out of range."""
    G, R = S.SHELL_SMALL
    N = G ** 3
    taps = S.small_shell_taps()
    a = TP.shell_rows(G, 100 * G + R)
    rows = [1, 2, 1, 2, 7]
    scale = np.float32(0.999)
    out, out_tap, out_value = maxcorr_guarded(a, taps, rows, G, R, scale, np.arange(N))
    assert np.isnan(out[4]).all() and np.isnan(out_value[4]).all() and (out_tap[4] == -1).all()
    for r in range(4):
        e3, arg = shell_max(a[r], taps[rows[r]], G, R)
        assert same_bits(out_value[r], e3) and same_bits(out[r], scale * e3) and np.array_equal(out_tap[r], arg), r
    e3, arg = shell_max(a[2], taps[rows[2]], G, R)
    assert (arg[e3 == 0] == -1).all() and ((e3 > 0) & (e3 < 2.0 ** -126)).any() and not np.isnan(out[3]).any()
    print(f"shell maxima G {G} R {R}: five rows, every voxel equal to the model (0 u)")
    h = S.SIDE / G
    blocks = TF.three_blocks((R - 1.51, min(1.6, R - 1.6)), 0.5, G, R)
    assert np.array_equal(blocks[0].view(np.int32), taps.view(np.int32)) and h > 0
    rng = np.random.default_rng(100 * G + R)
    e, m = (rng.uniform(0.05, 1.0, size=(3, N)).astype(np.float32) for _ in range(2))
    TF.check_moments(moments_guarded(e, m, blocks, [1, 2, 1], G, R), e, m, blocks, [1, 2, 1], G, R, f"shell moments G {G} R {R}")
