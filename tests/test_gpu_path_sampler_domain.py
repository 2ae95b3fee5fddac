"""GPU: the runner-up trajectories, the trajectory samples and the pose samples over the part of their documented domain
(include/sceneego_hip.h) that their own test files never enter: odd grids, G = 2 and 3, R = 16 below 128^3, R = 20 and 24, J = 32 on a
chain of depth 31 and on a tree with four children per joint, more than 65535 frames in one call, bases that are only 4-byte aligned
(8 bytes for the float64 scratch of the two samplers), and for all of them the memory contract: every output and the exactly sized
scratch lie between guard bands, every input between NaN bands (tests/volume_domain_cases.py: guarded, nan_banded), and the bands are
checked after each launch.  Every launch here is at _lib level.

INPUTS.  Those of tests/path_sampler_domain_cases.py, softmaxed ON THE HOST and copied: the arrays that
tests/test_path_sampler_domain_host.py has already put through the models on the CPU.  The forward pass behind the trajectory sampler
is se_volume_filter_f32 on the device (test_gpu_volume_domain.filter_guarded: guarded as well); the upward products behind the pose
sampler are se_skeleton_upward_f32's.  The models get the float32 arrays and flags the kernels got.

WHAT EACH CASE IS THERE FOR (W the power of two >= G, RP = 256 / W thread rows).
  runner-up trajectories (csrc/volume_viterbi.hip)
    vb_update_kernel   a new kernel, not vv_update_kernel reused.  G = 2, 3, 5, 9: RP >= G, so the three further rows of every thread
                       are clamped to G - 1 and discarded.  With succ written over scores the clamped row is another thread's voxel
                       whose score may already be a pointer: the value must go unused (test_pointers_written_over_the_scores...).
                       G = 127 (W = 128, RP = 2): the last turn of a thread is ragged.  G = 17, R = 16: the zero padding is as deep as
                       the plane.  The window test max(|i-xi|, |j-xj|, |k-xk|) > separation and the hand-over of mm(x*) through
                       rec[..][8] of workgroup xj at odd G: every case, and separation 0, G - 1, G + 5 at G = 9 and 3.
    vb_fold_kernel     the death path (r = p, pointers -1, max-marginals NaN, written by `chunks` workgroups) over 729 voxels, no
                       multiple of 256 (test_nan_cell_nan_frame_and_a_backward_death...).
    vv_scratch_bytes   rounds to 16 after two int8 planes of an odd voxel count: the scratch is exactly sized between guard bands.
    vb_branch_kernel   both directions across chunk cuts at G = 9 and 17, and over jump bits (the teleporting lobe at G = 9).
  trajectory samples (csrc/volume_sample.hip, csrc/categorical_sums.h)
    se_draw_sums_kernel  LDS rows of G + 1 floats at odd G; 65537 frames take turns in grid.z (frames 0 and 1 a second one).
    vsm_walk_kernel    windows clipped on both sides at G = 2, 3, 17 (R = G - 1); steps, jumps and fresh draws at odd grids (the
                       three cases at floor 0.3); 65537 dependent frames inside one launch.
    scratch            8-byte aligned, not 16; belief 4-byte aligned.
  pose samples (csrc/skeleton_sample.hip)
    sks_walk_kernel    R = 24 at 80^3: windows of up to 49^2 rows, the full r[SKS_WIN * SKS_WIN].  R = 20 at 128^3: 41^2 rows, no
                       ni * nj loop of an unclipped window finishes in one turn of 256 threads.  chain32: pose[] in LDS across 31
                       dependent joints.  heap4_32: four children per joint.  frame = y + 65535 z: 65537 frames.
    sk_upward_walk     the upward mode of the coupling's walk at the coupling's own domain cases.

TOLERANCES.  None is new and none is measured.  Everything on the two sequence operators and on the draws is BIT FOR BIT.  The one
bound is that of se_skeleton_upward_f32 against the float64 recursion, derived in tests/test_gpu_skeleton_sampler.py and taken from
there: |got - want| <= B want + delta_j, sums (B + L u) want + N delta_j, valid exact, B = belief_bound(parents, R) = 1.01 (2 (J - 1)
+ 1) (T(R) + L + 8 + kids) u.  T(R) = _lib.SHELL_CHAIN(R) depends on R alone.  L = _lib.SKELETON_SUM_CHAIN = 142 was derived for 128^3
and covers these grids by the argument of tests/test_gpu_volume_domain.py: CH = min(64, ceil(N / 256)) chunks of ceil(N / CH) values, a
thread adds ceil(chunk / 256) of them: 126 at 127^3 (chunk 32006), 17 at 65^3, at most 1 below 9^3; then 6 + 2 + 6.  All <= 142.
At (80, 24) and (128, 20) the direct float64 model is too slow on the host; there the sums must equal se_skeleton_couple_f32's evidence
of the root and se_skeleton_edge_stats_f32's normalisers bit for bit, as test_upward_sums_are_the_couplings_own_bit_for_bit has it.
The three J = 32 trees go through both: delta_j compounds by 1 / s_c per level of the tree, so on the chain of depth 31 the absolute
term of the bound holds nothing near the root (the test prints it, and the relative errors beside it), and the
bit-for-bit tie to the coupling, which tests/test_gpu_volume_domain.py holds to float64, is what constrains those sums.

NOT GUARDED.  Launches through VolumeViterbi, VolumeSmoother.sample and SkeletonPrior.sample use buffers the class allocates; they are
out of scope here (the operators' own files run them)."""
import functools

import numpy as np
import pytest
import torch

import path_sampler_domain_cases as C
import sequence_domain_cases as S
import test_gpu_skeleton_sampler as TQ
import test_gpu_volume_domain as TD
import test_gpu_volume_path_alternatives as TA
from sceneego_amd import _lib
from skeleton_sampler_model import FRESH, JUMP, STEP, skeleton_sample_model
from test_gpu_sequence_domain import banded, chunks_of, edge_stats_guarded, host, viterbi_guarded
from test_gpu_volume_domain import DEV, F32, I32, U8, Guards, same_bits
from test_gpu_volume_sampler import equal
from volume_sampler_model import volume_sampler_model
from volume_viterbi_model import JUMP as JUMP_BIT

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NAN = float("nan")


def ints(a, shape=None):
    return banded(np.ascontiguousarray(a, dtype=np.int32), 0, shape)


# ================================================================================================================== 1. runner-up trajectories
def keep_guarded(p, taps, G, R, floor, cuts=None, offsets=None):
    """test_gpu_volume_path_alternatives.forward_keep on the host array ``p`` [T, rows, N], guarded; ``offsets`` {prob, back_out, scores,
    scratch: bytes}."""
    off = offsets or {}
    T, rows, N = p.shape
    cuts = (T,) if cuts is None else tuple(cuts)
    assert sum(cuts) == T
    g = Guards(f"volume_viterbi_keep rows {rows} G {G} R {R} cuts {cuts} offsets {off}")
    pd, td = banded(p, off.get("prob", 0), (T, rows, N)), banded(taps)
    state = g.out(rows * N, F32)
    state.fill_(NAN)
    peak_state, best_state = g.out(rows, I32), g.out(rows, F32)
    back = g.out(T * rows * N, I32, off.get("back_out", 0)).view(T, rows, N)
    scores = g.out(T * rows * N, F32, off.get("scores", 0)).view(T, rows, N)
    peak, exponent, restarted = (g.out(T * rows, I32).view(T, rows) for _ in range(3))
    best = g.out(T * rows, F32).view(T, rows)
    scratch = g.out(_lib.volume_viterbi_scratch_bytes(rows, G, R), U8, off.get("scratch", 0))
    for name, t in (("prob", pd), ("back_out", back), ("scores", scores), ("scratch", scratch)):
        assert t.data_ptr() % 16 == off.get(name, 0) % 16
    ones = ints(np.ones(rows))
    t = 0
    for n in cuts:
        _lib.volume_viterbi_keep(pd[t:t + n], td, state, peak_state, best_state, back[t:t + n], peak[t:t + n], best[t:t + n],
                                 exponent[t:t + n], restarted[t:t + n], scores[t:t + n], n, rows, N, G, R, floor,
                                 have_prior=None if t == 0 else ones, scratch=scratch)
        g.check()
        t += n
    return {"back": host(back), "peak": host(peak), "best": host(best), "exponent": host(exponent), "restarted": host(restarted),
            "state": host(state, (rows, N)), "scores": host(scores), "dev": {"back": back, "restarted": restarted}}


def back_guarded(p, keep, index, taps, G, R, floor, sep=C.SEP, cuts=None, alias=False, want_mm=True, offsets=None):
    """test_gpu_volume_path_alternatives.backward over the host arrays of ``keep_guarded``, guarded, the carry poisoned before the first
    call; ``alias``: the successor pointers are written over (a guarded copy of) the scores.  ``offsets`` {prob, scores, r_state, succ,
    max_marginals, scratch: bytes}; with ``alias`` succ is the memory of scores and takes its offset."""
    off = offsets or {}
    T, rows, N = p.shape
    g = Guards(f"volume_viterbi_back rows {rows} G {G} R {R} separation {sep} cuts {cuts} alias {alias} offsets {off}")
    pd, td = banded(p, off.get("prob", 0), (T, rows, N)), banded(taps)
    ex, rs, idx = ints(keep["exponent"], (T, rows)), ints(keep["restarted"], (T, rows)), ints(index, (T, rows))
    if alias:
        scores = g.out(T * rows * N, F32, off.get("scores", 0)).view(T, rows, N)
        scores.copy_(torch.from_numpy(keep["scores"]))
        succ = scores.view(I32)
        assert succ.data_ptr() == scores.data_ptr()
    else:
        scores = banded(keep["scores"], off.get("scores", 0), (T, rows, N))
        succ = g.out(T * rows * N, I32, off.get("succ", 0)).view(T, rows, N)
    mm = g.out(T * rows * N, F32, off.get("max_marginals", 0)).view(T, rows, N) if want_mm else None
    carry = {"r": g.out(rows * N, F32, off.get("r_state", 0)), "link": g.out(rows, I32), "best": g.out(rows, F32),
             "complete": g.out(rows, I32)}
    carry["r"].fill_(NAN), carry["link"].fill_(5), carry["best"].fill_(NAN), carry["complete"].fill_(9)
    out = {name: g.out(T * rows, dtype).view(T, rows) for name, dtype in _lib.BACK_OUTPUTS}
    scratch = g.out(_lib.volume_viterbi_back_scratch_bytes(rows, G, R), U8, off.get("scratch", 0))
    for name, t in (("prob", pd), ("scores", scores), ("r_state", carry["r"]), ("scratch", scratch)):
        assert t.data_ptr() % 16 == off.get(name, 0) % 16
    for t0, t1 in chunks_of(T, cuts):
        _lib.volume_viterbi_back(pd[t0:t1], scores[t0:t1], ex[t0:t1], rs[t0:t1], idx[t0:t1], td, carry, {k: v[t0:t1] for k, v in out.items()},
                                 t1 - t0, rows, N, G, R, floor, sep, int(t1 != T), succ=succ[t0:t1],
                                 max_marginals=None if mm is None else mm[t0:t1], scratch=scratch)
        g.check()
    got = {k: host(v) for k, v in out.items()}
    got["succ"], got["succ_dev"], got["mm"] = host(succ), succ, None if mm is None else host(mm)
    got["carry"] = {"r": host(carry["r"], (rows, N)), "link": host(carry["link"]), "best": host(carry["best"]),
                    "complete": host(carry["complete"])}
    return got


def branch_guarded(dev, succ, anchor, cuts=None):
    """test_gpu_volume_path_alternatives.branch, guarded: down, last chunk first, then up, first chunk first."""
    back, restarted = dev["back"], dev["restarted"]
    T, rows, N = back.shape
    g = Guards(f"volume_viterbi_branch rows {rows} voxels {N} cuts {cuts}")
    an = ints(anchor, (T, rows))
    cursor, index, jumped = g.out(rows, I32), g.out(T * rows, I32).view(T, rows), g.out(T * rows, I32).view(T, rows)
    cursor.fill_(777), index.fill_(-9), jumped.fill_(-9)
    down = chunks_of(T, cuts)
    for direction, chunks in ((-1, down), (1, down[::-1])):
        for n, (t0, t1) in enumerate(chunks):
            _lib.volume_viterbi_branch(back[t0:t1], succ[t0:t1], restarted[t0:t1], an[t0:t1], cursor, index[t0:t1], jumped[t0:t1], t1 - t0,
                                       rows, N, direction, int(n > 0))
            g.check()
    return host(index), host(jumped)


def check_branch(keep, got, want, label, cuts=None):
    index, jumped = branch_guarded(keep["dev"], got["succ_dev"], want["anchor"], cuts)
    assert np.array_equal(index, want["runner_up_index"]) and np.array_equal(jumped != 0, want["runner_up_jumped"]), label
    assert set(np.unique(jumped)) <= {0, 1}


@pytest.mark.parametrize("rows,G,R,floor,T", C.SEQUENCE_CASES)
def test_runner_up_against_the_model_bit_for_bit(rows, G, R, floor, T):
    k, label = C.filter_inputs(rows, G, R, T), f"runner-up rows {rows} G {G} R {R} floor {floor}"
    f, want = C.alternatives_want(rows, G, R, floor, T)
    C.alternatives_condition(f, want)
    # (a) the kept-scores entry: every output of the old entry bit for bit, and the scores
    old = viterbi_guarded(k["p"], k["taps"], G, R, floor)
    keep = keep_guarded(k["p"], k["taps"], G, R, floor)
    for key in ("back", "peak", "exponent", "restarted"):
        assert np.array_equal(keep[key], old[key]), f"{label}: {key}"
    assert same_bits(keep["best"], old["best"]) and same_bits(keep["state"], old["state"])
    assert same_bits(np.ldexp(keep["scores"], -keep["exponent"][:, :, None]), f["state"]), f"{label}: scores"
    # (b) the backward pass, the successor pointers and the raw max-marginals in buffers of their own, and the carried state
    got = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor)
    TA.check_backward(got, want, label)
    assert set(np.unique(got["complete"])) <= {0, 1}
    # (c) the branch walk from the model's anchors
    check_branch(keep, got, want, label)
    print(f"{label}: every output equal to the model (0 u); {int((want['alt_index'] < 0).sum())} frames without an alternative, "
          f"{int(((want['succ'] >= 0) & ((want['succ'] & JUMP_BIT) != 0)).sum())} successor pointers with the jump bit")


@pytest.mark.parametrize("G", C.ALTERNATIVES_SEPARATION_GRIDS)
def test_separation_zero_and_a_window_that_leaves_nothing_at_an_odd_grid(G):
    rows, _, R, floor, T = C.case_of(G)
    k = C.filter_inputs(rows, G, R, T)
    keep = keep_guarded(k["p"], k["taps"], G, R, floor)
    for sep in (0, G - 1, G + 5):
        f, want = C.alternatives_want(rows, G, R, floor, T, sep)
        assert not want["tied"].any()
        got = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor, sep=sep)
        TA.check_backward(got, want, f"G {G} separation {sep}")
        if sep == 0:
            assert (got["alt_index"] >= 0).all() and (got["alt_index"] != f["index"]).all()
        else:
            assert (got["alt_index"] == -1).all() and np.isnan(got["alt_value"]).all() and (want["anchor"] == -1).all()
            assert np.isfinite(got["path_value"]).all()
        check_branch(keep, got, want, f"G {G} separation {sep}")


@pytest.mark.parametrize("G", C.ALTERNATIVES_ALIAS_GRIDS)
def test_pointers_written_over_the_scores_at_the_clamped_row_shapes(G):
    """succ is the memory of scores: a thread of vb_update_kernel reads the score of a clamped row - another thread's voxel, perhaps a
    pointer already - and must not use it.  Identical to the run into a buffer of its own, and to the model."""
    rows, _, R, floor, T = C.case_of(G)
    k = C.filter_inputs(rows, G, R, T)
    f, want = C.alternatives_want(rows, G, R, floor, T)
    keep = keep_guarded(k["p"], k["taps"], G, R, floor)
    own = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor)
    over = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor, alias=True)
    TA.check_backward(over, want, f"G {G}, pointers over the scores")
    assert np.array_equal(over["succ"], own["succ"]) and same_bits(over["mm"], own["mm"])
    for key in TA.FLOATS + TA.INTS:
        assert same_bits(over[key], own[key]), key
    assert same_bits(over["carry"]["r"], own["carry"]["r"])
    none = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor, alias=True, want_mm=False)
    TA.check_backward(none, want, f"G {G}, pointers over the scores, no max-marginals")
    check_branch(keep, over, want, f"G {G}, pointers over the scores")


@pytest.mark.parametrize("G", C.ALTERNATIVES_CUT_GRIDS)
def test_chunk_cuts_at_odd_grids_give_the_bits_of_one_call(G):
    rows, _, R, floor, T = C.case_of(G)
    k = C.filter_inputs(rows, G, R, T)
    f, want = C.alternatives_want(rows, G, R, floor, T)
    whole = keep_guarded(k["p"], k["taps"], G, R, floor)
    for cuts in ((1, T - 1), (T - 1, 1), (1,) * T):
        keep = keep_guarded(k["p"], k["taps"], G, R, floor, cuts=cuts)
        for key in ("back", "peak", "exponent", "restarted"):
            assert np.array_equal(keep[key], whole[key]), (cuts, key)
        assert same_bits(keep["scores"], whole["scores"]) and same_bits(keep["state"], whole["state"]) and same_bits(keep["best"], whole["best"])
        for alias in (False, True):
            got = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor, cuts=cuts, alias=alias, want_mm=not alias)
            TA.check_backward(got, want, f"G {G} cuts {cuts} alias {alias}")
        check_branch(keep, got, want, f"G {G} walk cut {cuts}", cuts)


def test_nan_cell_nan_frame_and_a_backward_death_at_an_odd_grid():
    rows, G, R, floor, T = C.ALTERNATIVES_NAN_CASE
    n = C.alternatives_nan_inputs()
    p, f, want = n["p"], n["f"], n["b"]
    keep = keep_guarded(p, n["taps"], G, R, floor, cuts=(2, 1, 1))
    assert np.array_equal(keep["back"], f["back"]) and np.array_equal(keep["restarted"] != 0, f["restarted"])
    got = back_guarded(p, keep, f["index"], n["taps"], G, R, floor, cuts=(2, 1, 1))
    TA.check_backward(got, want, "NaN", volumes=False)
    assert np.array_equal(got["succ"], want["succ"])
    fin = np.isfinite(want["mm"])
    assert np.array_equal(np.isfinite(got["mm"]), fin) and same_bits(got["mm"][fin], want["mm"][fin])
    assert np.isnan(got["mm"][1, 0, 400]) and np.isnan(got["mm"][2, 1]).all() and (got["succ"][1:, 1] == -1).all()
    assert np.isnan(got["path_value"][2, 1]) and got["alt_index"][2, 1] == got["mm_peak"][2, 1] == -1
    check_branch(keep, got, want, "NaN", (2, 1, 1))
    _, clean = C.alternatives_want(rows, G, R, floor, T)
    for key in TA.FLOATS:                                                    # row 2 holds no NaN: the clean run's
        assert same_bits(got[key][:, 2], clean[key][:, 2]), key
    assert np.array_equal(got["succ"][:, 2], clean["succ"][:, 2])
    # the death: vb_fold_kernel's fill loop over 729 voxels, by `chunks` workgroups
    d = C.alternatives_death_inputs()
    G, R, floor = d["G"], d["R"], d["floor"]
    keep = keep_guarded(d["p"], d["taps"], G, R, floor)
    assert np.array_equal(keep["back"], d["f"]["back"]) and np.array_equal(keep["restarted"] != 0, d["f"]["restarted"])
    for cuts, alias in (((4,), False), ((2, 2), True), ((1, 1, 1, 1), False)):
        got = back_guarded(d["p"], keep, d["f"]["index"], d["taps"], G, R, floor, sep=0, cuts=cuts, alias=alias)
        TA.check_backward(got, d["b"], f"death {cuts}")
    assert np.isnan(got["mm"][1, 0]).all() and (got["succ"][1, 0] == -1).all() and np.isnan(got["path_value"][1, 0])
    assert same_bits(got["carry"]["r"], d["b"]["carry"]["r"]) and got["complete"].T.tolist() == [[0, 0, 1, 1], [1] * 4]


def test_a_teleporting_lobe_sets_jump_bits_at_an_odd_grid():
    G, R, floor = S.VITERBI_JUMP_CASE
    k, want = C.alternatives_jump_want()
    f = k["m"]
    jump_bits = ((want["succ"] >= 0) & ((want["succ"] & JUMP_BIT) != 0)).sum()
    assert not f["tied"].any() and not want["tied"].any() and jump_bits > 0 and want["runner_up_jumped"].any() and f["jumped"][2].all()
    keep = keep_guarded(k["p"], k["taps"], G, R, floor, cuts=(2, 2))
    got = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor, cuts=(2, 2))
    TA.check_backward(got, want, "teleport")
    assert int(((got["succ"] >= 0) & ((got["succ"] & JUMP_BIT) != 0)).sum()) == jump_bits
    for cuts in ((4,), (2, 2), (1, 3), (3, 1), (1, 1, 1, 1)):                # the jump crosses a chunk boundary of the walk in some of these
        check_branch(keep, got, want, f"teleport, walk cut {cuts}", cuts)


@pytest.mark.parametrize("rows,G,R,floor,T", [C.SEQUENCE_ALIGN_CASE, C.case_of(9)])
def test_runner_up_alignment_does_not_change_a_bit(rows, G, R, floor, T):
    """prob, scores, r_state, succ, max_marginals, back_out and the scratch of both calls 4 bytes off their alignment, one at a time and
    all together."""
    k = C.filter_inputs(rows, G, R, T)
    f, want = C.alternatives_want(rows, G, R, floor, T)
    base_keep = keep_guarded(k["p"], k["taps"], G, R, floor)
    names = ("prob", "scores", "r_state", "succ", "max_marginals", "back_out", "scratch")
    for moved in [(n,) for n in names] + [names]:
        offsets = {n: 4 for n in moved}
        keep = keep_guarded(k["p"], k["taps"], G, R, floor, offsets=offsets)
        for key in ("back", "peak", "exponent", "restarted"):
            assert np.array_equal(keep[key], base_keep[key]), (moved, key)
        assert same_bits(keep["scores"], base_keep["scores"]) and same_bits(keep["state"], base_keep["state"]), moved
        got = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor, offsets=offsets)
        TA.check_backward(got, want, f"offset {moved}")
        over = back_guarded(k["p"], keep, f["index"], k["taps"], G, R, floor, alias=True, offsets=offsets)
        TA.check_backward(over, want, f"offset {moved}, pointers over the scores")
        check_branch(keep, got, want, f"offset {moved}")


# ================================================================================================================== 2. trajectory samples
@functools.lru_cache(maxsize=None)
def forward_dev(rows, G, R, floor, T):
    """filter_inputs and the forward pass se_volume_filter_f32 through one guarded call, taken once: the float32 beliefs ``b`` and the
    flags ``rs`` on the host (nothing modifies them)."""
    k = dict(TD.filter_dev(rows, G, R, T))
    out = TD.filter_guarded(k, G, R, floor)
    k["b"], k["rs"] = out[0], out[3]
    return k


def sample_guarded(b, rs, taps, G, R, floor, samples, cuts=None, seed=0, first_sample=0, offsets=None):
    """test_gpu_volume_sampler.sample on the host arrays ``b`` [T, rows, N] and ``rs`` [T, rows], guarded: calls of ``cuts`` frames each
    (in frame order; issued last chunk first, ``next`` and ``have_link`` carried), each with its exactly sized scratch.  ``offsets``
    {belief: bytes (a multiple of 4), scratch: bytes (a multiple of 8)}.  A launch that does not return 0 raises in _lib; the bands
    are checked, behind a synchronize, after each."""
    off = offsets or {}
    T, rows, N = b.shape
    g = Guards(f"volume_sample rows {rows} G {G} R {R} samples {samples} cuts {cuts} offsets {off}")
    bd, rd, td = banded(b, off.get("belief", 0), (T, rows, N)), ints(rs, (T, rows)), banded(taps)
    nxt = g.out(samples * rows, I32)
    nxt.fill_(-7)
    index, kind = np.full((samples, T, rows), -7, dtype=np.int32), np.full((samples, T, rows), -7, dtype=np.int32)
    for t0, t1 in chunks_of(T, cuts):
        n = t1 - t0
        idx, knd = g.out(samples * n * rows, I32), g.out(samples * n * rows, I32)
        scratch = g.out(_lib.volume_sample_scratch_bytes(n, rows, G), U8, off.get("scratch", 0))
        assert scratch.data_ptr() % 16 == off.get("scratch", 0) % 16 and bd.data_ptr() % 16 == off.get("belief", 0) % 16
        link = None if t1 == T else ints(np.asarray(rs[t1]) == 0)
        _lib.volume_sample(bd[t0:t1], rd[t0:t1], td, nxt, idx, knd, n, rows, N, G, R, floor, samples, first_sample=first_sample,
                           first_frame=t0, seed=seed, have_link=link, scratch=scratch)
        torch.cuda.synchronize()
        g.check()
        index[:, t0:t1], kind[:, t0:t1] = host(idx, (samples, n, rows)), host(knd, (samples, n, rows))
    return {"index": index, "kind": kind, "next": host(nxt, (samples, rows))}


@pytest.mark.parametrize("rows,G,R,floor,T", C.SAMPLER_CASES)
def test_trajectory_samples_against_the_model_bit_for_bit(rows, G, R, floor, T):
    k = forward_dev(rows, G, R, floor, T)
    n = C.samples_for(floor)
    assert k["rs"][0].all() and not k["rs"][1:].any()
    want = volume_sampler_model(k["b"], k["rs"], k["taps"], G, floor, n, seed=C.SAMPLER_SEED)
    kinds = C.sampler_condition(want, floor)
    got = sample_guarded(k["b"], k["rs"], k["taps"], G, R, floor, n, seed=C.SAMPLER_SEED)
    equal(got, want, f"rows {rows} G {G} R {R} floor {floor}")
    assert (got["index"] >= 0).all() and (got["index"] < G ** 3).all() and np.array_equal(got["next"], got["index"][:, 0])
    if floor == C.JUMP_FLOOR:
        assert set(np.unique(got["kind"]).tolist()) == {STEP, JUMP, FRESH}
    print(f"rows {rows} G {G} R {R} floor {floor}: {n * T * rows} draws equal; kinds of the linked frames {sorted(kinds)}")


def test_trajectory_samples_do_not_depend_on_cuts_and_splits_at_an_odd_grid():
    rows, G, R, floor, T = C.SAMPLER_CUT_CASE
    k = forward_dev(rows, G, R, floor, T)
    args = (k["b"], k["rs"], k["taps"], G, R, floor)
    whole = sample_guarded(*args, 16, seed=9)
    equal(whole, volume_sampler_model(k["b"], k["rs"], k["taps"], G, floor, 16, seed=9), "whole")
    for cuts in ((1, 3), (3, 1), (2, 2), (1, 2, 1), (1, 1, 1, 1)):
        equal(sample_guarded(*args, 16, cuts=cuts, seed=9), whole, f"cuts {cuts}")
    lo, hi = sample_guarded(*args, 8, seed=9), sample_guarded(*args, 8, seed=9, first_sample=8, cuts=(2, 2))
    for key in ("index", "kind", "next"):
        assert np.array_equal(np.concatenate([lo[key], hi[key]]), whole[key]), key


@pytest.mark.parametrize("rows,G,R,floor,T", [C.SEQUENCE_ALIGN_CASE, C.SAMPLER_CUT_CASE])
def test_trajectory_samples_alignment_does_not_change_a_bit(rows, G, R, floor, T):
    """belief 4 bytes off its alignment; scratch 8 bytes off 16: what the header promises the float64 sums."""
    k = forward_dev(rows, G, R, floor, T)
    args = (k["b"], k["rs"], k["taps"], G, R, floor, 8)
    base = sample_guarded(*args, seed=4)
    equal(base, volume_sampler_model(k["b"], k["rs"], k["taps"], G, floor, 8, seed=4), "aligned")
    for offsets in ({"belief": 4}, {"scratch": 8}, {"belief": 4, "scratch": 8}):
        equal(sample_guarded(*args, seed=4, offsets=offsets), base, f"offsets {offsets}")
        equal(sample_guarded(*args, seed=4, offsets=offsets, cuts=(1, T - 1)), base, f"offsets {offsets}, cut")


def test_a_nan_frame_unlinks_its_neighbour_at_an_odd_grid():
    rows, G, R, floor, T = C.SAMPLER_NAN_CASE
    k = forward_dev(rows, G, R, floor, T)
    clean = sample_guarded(k["b"], k["rs"], k["taps"], G, R, floor, 8, seed=2)
    p = k["p"].copy()
    p[2, 1] = np.nan
    out = TD.filter_guarded(k, G, R, floor, prob=p)
    b, rs = out[0], out[3]
    assert rs[:, 1].tolist() == [1, 0, 1, 1]
    got = sample_guarded(b, rs, k["taps"], G, R, floor, 8, cuts=(3, 1), seed=2)
    equal(got, volume_sampler_model(b, rs, k["taps"], G, floor, 8, seed=2), "NaN frame")
    assert (got["index"][:, 2, 1] == -1).all() and (got["kind"][:, [1, 2, 3], 1] == FRESH).all()
    assert (got["kind"][:, 0, 1] != FRESH).all() and (got["index"][:, [0, 1, 3], 1] >= 0).all()
    others = [0, 2, 3]
    assert np.array_equal(got["index"][:, :, others], clean["index"][:, :, others])
    assert np.array_equal(got["kind"][:, :, others], clean["kind"][:, :, others])


def test_a_track_of_65537_frames():
    """More frames than grid.z of se_draw_sums_kernel holds: frames 0 and 1 take a second turn of a workgroup.  One call against the
    same track in two calls of 32768 + 32769 frames (each sums launch within grid.z), and its last eight frames against the model."""
    k = C.long_track_inputs()
    args = (k["b"], k["rs"], k["taps"], k["G"], k["R"], k["floor"], k["samples"])
    one = sample_guarded(*args, seed=k["seed"])                             # raises unless the launch returned 0 and the device is clean
    assert (one["index"] >= 0).all() and (one["index"] < 8).all() and set(np.unique(one["kind"]).tolist()) == {STEP, JUMP, FRESH}
    assert (one["kind"][:, -1] == FRESH).all() and (one["kind"][:, :-1] != FRESH).all()
    two = sample_guarded(*args, seed=k["seed"], cuts=(C.LONG_SPLIT, C.LONG_FRAMES - C.LONG_SPLIT))
    equal(one, two, "65537 frames in one call and in two")
    tail = C.long_track_tail()
    t0 = C.LONG_FRAMES - C.LONG_TAIL
    assert np.array_equal(one["index"][:, t0:], tail["index"]) and np.array_equal(one["kind"][:, t0:], tail["kind"])


# ================================================================================================================== 3. pose samples
def upward_guarded(k, G, R, floor, frames=None, offsets=None):
    """One guarded se_skeleton_upward_f32 call over the frames ``frames`` (a slice; default all): host arrays (upward [F, J, N], sums
    [F, J], valid [F]).  ``offsets`` {prob, upward, scratch: bytes}."""
    off = offsets or {}
    p = k["p"] if frames is None else k["p"][frames]
    F, J, N = p.shape
    g = Guards(f"skeleton_upward frames {F} J {J} G {G} R {R} offsets {off}")
    A, sums, valid = g.out(F * J * N, F32, off.get("upward", 0)), g.out(F * J, F32), g.out(F, I32)
    scratch = g.out(_lib.skeleton_upward_scratch_bytes(F, J, G, R), U8, off.get("scratch", 0))
    _lib.skeleton_upward(banded(p, off.get("prob", 0)), banded(k["taps"]), k["parents"], A, sums, valid, F, N, G, R, floor, scratch=scratch)
    g.check()
    return host(A, (F, J, N)), host(sums, (F, J)), host(valid)


def pose_sample_guarded(A, valid, taps, parents, G, R, floor, samples, first_sample=0, first_frame=0, seed=0, offsets=None):
    """One guarded se_skeleton_sample_f32 call on the host array ``A`` [F, J, N] between NaN bands: host arrays (index, kind) [samples,
    F, J].  ``offsets`` {upward: bytes (a multiple of 4), scratch: bytes (a multiple of 8)}."""
    off = offsets or {}
    F, J, N = A.shape
    g = Guards(f"skeleton_sample frames {F} J {J} G {G} R {R} samples {samples} offsets {off}")
    Ad = banded(A, off.get("upward", 0), (F, J, N))
    index, kind = g.out(samples * F * J, I32), g.out(samples * F * J, I32)
    scratch = g.out(_lib.skeleton_sample_scratch_bytes(F, J, G), U8, off.get("scratch", 0))
    assert scratch.data_ptr() % 16 == off.get("scratch", 0) % 16 and Ad.data_ptr() % 16 == off.get("upward", 0) % 16
    _lib.skeleton_sample(Ad, None if valid is None else ints(valid), banded(taps), parents, index, kind, F, N, G, R, floor, samples,
                         first_sample=first_sample, first_frame=first_frame, seed=seed, scratch=scratch)
    torch.cuda.synchronize()
    g.check()
    return host(index, (samples, F, J)), host(kind, (samples, F, J))


def check_pose(got, want, what):
    wrong = int((got[0] != want["index"]).sum()), int((got[1] != want["kind"]).sum())
    assert wrong == (0, 0), f"{what}: {wrong[0]} voxels and {wrong[1]} kinds of {got[0].size} differ from the model"


@functools.lru_cache(maxsize=None)
def upward_run(frames, tree, G, R, floor):
    """The device's own upward products of a case through one guarded call, read back once (nothing modifies them)."""
    return upward_guarded(TD.skeleton_dev(frames, tree, G, R), G, R, floor)


@pytest.mark.parametrize("frames,tree,G,R,floor", C.UPWARD_MODEL_CASES)
def test_upward_against_the_model(frames, tree, G, R, floor):
    """The bound of tests/test_gpu_skeleton_sampler.py: test_upward_against_the_model (the docstring above says why L covers these grids)."""
    k = TD.skeleton_dev(frames, tree, G, R)
    N = G ** 3
    wA, ws, wv = C.upward_want(frames, tree, G, R, floor)
    small = C.upward_condition(ws, wv)
    A, sums, valid = upward_run(frames, tree, G, R, floor)
    assert valid.tolist() == [1] * frames
    B = TQ.belief_bound(k["parents"], R)
    assert B < 0.01
    delta = TQ.underflow_term(k["parents"], ws, R)
    err = np.abs(A.astype(np.float64) - wA)
    tol = B * wA + delta[:, :, None]
    serr = np.abs(sums.astype(np.float64) - ws)
    print(f"upward frames {frames} {tree} G {G} R {R} floor {floor}: bound {B / U:.0f} u; worst upward "
          f"{float((err / (wA + 2.0 ** -100)).max()) / U:.2f} u, sums {float((serr / ws).max()) / U:.2f} u; smallest sum {small:.3g}; largest "
          f"underflow term {delta.max():.3g}")
    assert (err <= tol).all(), f"an upward product is off by {float((err - tol).max()):.3e} beyond the bound"
    assert (serr <= (B + TQ.L * U) * ws + N * delta).all(), f"a sum is off by {float((serr / ws).max()):.3e} relative"


@pytest.mark.parametrize("frames,tree,G,R,floor", C.UPWARD_LIBRARY_CASES)
def test_upward_sums_are_the_couplings_own_at_the_largest_radii_and_the_deepest_trees(frames, tree, G, R, floor):
    k = TD.skeleton_dev(frames, tree, G, R)
    _, sums, valid = upward_run(frames, tree, G, R, floor)
    _, _, evidence, coupled = TD.skeleton_guarded(k, G, R, floor)
    _, norms, ok = edge_stats_guarded(k, (k["taps"],) * 3, G, R, floor)
    assert same_bits(sums[:, 1:], np.ascontiguousarray(norms[:, 1:, 0])) and same_bits(sums[:, 0], np.ascontiguousarray(evidence[:, 0]))
    assert coupled.all() and ok.all() and valid.tolist() == [1] * frames and (sums >= 1e-12).all()


@pytest.mark.parametrize("frames,tree,G,R,floor", C.SKELETON_DRAW_CASES)
def test_pose_samples_against_the_model_bit_for_bit(frames, tree, G, R, floor):
    k = TD.skeleton_dev(frames, tree, G, R)
    A, _, valid = upward_run(frames, tree, G, R, floor)
    seed = C.pose_seed(tree, G, R)
    want = skeleton_sample_model(A, valid, k["taps"], k["parents"], G, R, floor, C.POSE_SAMPLES, seed=seed)
    kinds = C.pose_condition(want, G)
    got = pose_sample_guarded(A, valid, k["taps"], k["parents"], G, R, floor, C.POSE_SAMPLES, seed=seed)
    check_pose(got, want, f"frames {frames} {tree} G {G} R {R} floor {floor}")
    assert (got[0] >= 0).all() and (got[0] < G ** 3).all()
    print(f"pose samples frames {frames} {tree} G {G} R {R} floor {floor}: {got[0].size} draws equal; kinds below the root {sorted(kinds)}")


def test_steps_and_jumps_both_occur_at_the_jump_floor():
    kinds = []
    for frames, tree, G, R, floor in C.SKELETON_JUMP_CASES:
        k = TD.skeleton_dev(frames, tree, G, R)
        A, _, valid = upward_run(frames, tree, G, R, floor)
        want = skeleton_sample_model(A, valid, k["taps"], k["parents"], G, R, floor, C.POSE_SAMPLES, seed=C.pose_seed(tree, G, R))
        kinds.append(want["kind"][:, :, 1:].reshape(-1))
    kinds = np.concatenate(kinds)
    assert (kinds == STEP).any() and (kinds == JUMP).any() and not (kinds == FRESH).any()


def test_pose_batching_at_an_odd_grid():
    """Five frames in one call, as 1 + 4 and as 2 + 3 with first_frame: the upward pass walks a group of four and one more."""
    frames, tree, G, R, floor = C.SKELETON_BATCH_CASE
    k = TD.skeleton_dev(frames, tree, G, R)
    five = upward_guarded(k, G, R, floor)
    assert five[2].tolist() == [1] * 5
    args = (k["taps"], k["parents"], G, R, floor, C.POSE_SAMPLES)
    drawn = pose_sample_guarded(five[0], five[2], *args, seed=7)
    check_pose(drawn, skeleton_sample_model(five[0], five[2], k["taps"], k["parents"], G, R, floor, C.POSE_SAMPLES, seed=7), "five frames")
    for cut in (1, 2):
        parts = [upward_guarded(k, G, R, floor, frames=slice(0, cut)), upward_guarded(k, G, R, floor, frames=slice(cut, 5))]
        for x in range(3):
            assert same_bits(np.concatenate([q[x] for q in parts]), five[x]), (cut, x)
        head = pose_sample_guarded(parts[0][0], parts[0][2], *args, seed=7)
        tail = pose_sample_guarded(parts[1][0], parts[1][2], *args, seed=7, first_frame=cut)
        assert all(np.array_equal(np.concatenate([a, b], axis=1), c) for a, b, c in zip(head, tail, drawn)), cut
    lo, hi = pose_sample_guarded(five[0], five[2], *args[:-1], 3, seed=7), pose_sample_guarded(five[0], five[2], *args[:-1], 5, seed=7, first_sample=3)
    assert all(np.array_equal(np.concatenate([a, b]), c) for a, b, c in zip(lo, hi, drawn))


def test_pose_samples_alignment_does_not_change_a_bit():
    """upward 4 bytes off its alignment - as an output of the upward call and as the input of the draws - and the float64 scratch of
    the draws 8 bytes off 16; prob and the scratch of the upward call 4 bytes off."""
    frames, tree, G, R, floor = C.SKELETON_ALIGN_CASE
    k = TD.skeleton_dev(frames, tree, G, R)
    base = upward_guarded(k, G, R, floor)
    names = ("prob", "upward", "scratch")
    for moved in [(n,) for n in names] + [names]:
        got = upward_guarded(k, G, R, floor, offsets={n: 4 for n in moved})
        assert all(same_bits(a, b) for a, b in zip(got, base)), f"upward, offset {moved}"
    args = (base[0], base[2], k["taps"], k["parents"], G, R, floor, C.POSE_SAMPLES)
    drawn = pose_sample_guarded(*args, seed=4)
    check_pose(drawn, skeleton_sample_model(*args, seed=4), "aligned")
    for offsets in ({"upward": 4}, {"scratch": 8}, {"upward": 4, "scratch": 8}):
        got = pose_sample_guarded(*args, seed=4, offsets=offsets)
        assert np.array_equal(got[0], drawn[0]) and np.array_equal(got[1], drawn[1]), offsets


def test_an_invalid_frame_between_two_valid_ones_reads_nothing():
    """valid = 0 in the middle frame, whose upward products are NaN throughout, between NaN bands: nothing of it may reach a result."""
    frames, tree, G, R, floor = C.SKELETON_HOLE_CASE
    k = TD.skeleton_dev(frames, tree, G, R)
    A = upward_guarded(k, G, R, floor, frames=slice(0, 3))[0].copy()
    args = (k["taps"], k["parents"], G, R, floor, C.POSE_SAMPLES)
    clean = pose_sample_guarded(A, None, *args, seed=5)
    A[1] = np.nan
    valid = np.array([1, 0, 1], dtype=np.int32)
    got = pose_sample_guarded(A, valid, *args, seed=5)
    check_pose(got, skeleton_sample_model(A, valid, k["taps"], k["parents"], G, R, floor, C.POSE_SAMPLES, seed=5), "an invalid frame")
    assert (got[0][:, 1] == -1).all() and (got[1][:, 1] == FRESH).all() and (got[0][:, [0, 2]] >= 0).all()
    assert np.array_equal(got[0][:, [0, 2]], clean[0][:, [0, 2]]) and np.array_equal(got[1][:, [0, 2]], clean[1][:, [0, 2]])


def test_poses_of_65537_frames():
    """frame = y + 65535 z in sks_walk_kernel, and the turns of se_draw_sums_kernel in grid.z: one call against two calls of 32768 +
    32769 frames, and the last eight frames against the model."""
    k = C.long_pose_inputs()
    args = (k["taps"], k["parents"], k["G"], k["R"], k["floor"], k["samples"])
    one = pose_sample_guarded(k["A"], None, *args, seed=k["seed"])          # raises unless the launch returned 0 and the device is clean
    assert (one[0] >= 0).all() and (one[0] < 8).all() and (one[1][:, :, 0] == FRESH).all() and (one[1][:, :, 1:] != FRESH).all()
    assert set(np.unique(one[1]).tolist()) == {STEP, JUMP, FRESH}
    head = pose_sample_guarded(k["A"][:C.LONG_SPLIT], None, *args, seed=k["seed"])
    rest = pose_sample_guarded(k["A"][C.LONG_SPLIT:], None, *args, seed=k["seed"], first_frame=C.LONG_SPLIT)
    assert all(np.array_equal(np.concatenate([a, b], axis=1), c) for a, b, c in zip(head, rest, one))
    tail = C.long_pose_tail()
    t0 = C.LONG_FRAMES - C.LONG_TAIL
    assert np.array_equal(one[0][:, t0:], tail["index"]) and np.array_equal(one[1][:, t0:], tail["kind"])
