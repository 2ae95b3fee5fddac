"""CPU: the numpy model of the backward max-product pass and of the branch walk (tests/volume_viterbi_alternatives_model.py) gives the
max-marginals it claims to (against the brute force over every trajectory, and a dense check), pins the direction of the reversed
taps, keeps segments apart, reports a backward death, stays within a counted number of float32 roundings of float64, and shows the
runner-up on the ghost case of the README.  The Python surface refuses bad calls before anything touches a device."""
import math

import numpy as np
import pytest

from sceneego_amd import _lib
from sceneego_amd.volume_viterbi import (ALTERNATIVE_KEYS, VolumeViterbi, path_margins, runner_up_anchors, segment_broadcast,
                                          segment_log_scores)
from test_volume_viterbi_host import _ghost
from volume_filter_cases import SIDE, coord_grid, make_logits, softmax32, taps_for
from volume_viterbi_alternatives_model import (backward_model, branch_walk, brute_force_max_marginals, margins, reversed_taps,
                                               runner_up_anchors as model_anchors)
from volume_viterbi_model import JUMP, viterbi_path, volume_viterbi_model

ASYM = {1: np.array([0.2, 0.3, 0.5], dtype=np.float32), 2: np.array([0.05, 0.10, 0.20, 0.30, 0.35], dtype=np.float32)}


def run(p, w, G, floor, separation, dtype=np.float32, reverse=True):
    """Forward model, path, backward model, margins, anchors and the runner-up's branch walk."""
    f = volume_viterbi_model(p, w, G, floor, dtype=dtype)
    f["index"], f["jumped"] = viterbi_path(f["back"], f["peak"], f["restarted"])
    b = backward_model(p, f, f["index"], w, G, floor, separation, dtype=dtype, reverse=reverse)
    b["margin"] = margins(b["path_value"], b["alt_value"], b["alt_index"], f["index"])
    b["anchor"], b["runner_up_margin"] = model_anchors(b["margin"], b["alt_index"], f["restarted"])
    b["runner_up_index"], b["runner_up_jumped"] = branch_walk(f["back"], b["succ"], f["restarted"], b["anchor"])
    return f, b


def brute_cases():
    for R in (1, 2):
        for sym in (True, False):
            for floor in (0.0, 1e-3, 0.3):
                yield R, sym, floor


# ------------------------------------------------------------------------------------------------------------------ the claim
@pytest.mark.parametrize("R,sym,floor", list(brute_cases()))
def test_max_marginals_equal_the_brute_force_over_every_trajectory(R, sym, floor):
    """G = 3, T = 4, float64: every mm_t(x) equals the maximum over all 27^4 trajectories that are at x in frame t, to 1e-12 relative
    (each frame normalised by its maximum: the model's scores carry the powers of two of the rescaling)."""
    G, T = 3, 4
    p = softmax32(make_logits(T, 1, G, R, seed=9100 + 10 * R + int(sym)))
    w = taps_for(G, R) if sym else ASYM[R]
    want, _, _ = brute_force_max_marginals(p[:, 0], w, G, floor)
    _, b = run(p, w, G, floor, 0, dtype=np.float64)
    got = b["mm"][:, 0] / b["mm"][:, 0].max(axis=1, keepdims=True)
    want = want / want.max(axis=1, keepdims=True)
    err = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print(f"R {R} {'symmetric' if sym else 'asymmetric'} floor {floor}: max relative difference {err.max():.2e}, "
          f"{int((want == 0).sum())} exact zeros")
    assert (got[want == 0] == 0).all() and err.max() <= 1e-12
    assert b["complete"].all() and not b["death"].any() and b["linked"][:-1].all() and not b["linked"][-1].any()


@pytest.mark.parametrize("R", [1, 2])
def test_unreversed_asymmetric_taps_do_not_agree(R):
    """The direction: with asymmetric taps the backward pass must take them reversed.  Taken as they are, the max-marginals differ
    from the brute force by far more than rounding."""
    G, T, floor = 3, 4, 1e-3
    p = softmax32(make_logits(T, 1, G, R, seed=9100 + 10 * R))
    want, _, _ = brute_force_max_marginals(p[:, 0], ASYM[R], G, floor)
    want = want / want.max(axis=1, keepdims=True)
    _, wrong = run(p, ASYM[R], G, floor, 0, dtype=np.float64, reverse=False)
    got = wrong["mm"][:, 0] / wrong["mm"][:, 0].max(axis=1, keepdims=True)
    worst = (np.abs(got - want) / want).max()
    print(f"R {R}: un-reversed taps are off by up to {worst:.3g} relative")
    assert worst > 1e-3
    assert np.array_equal(reversed_taps(reversed_taps(ASYM[R])), ASYM[R])


@pytest.mark.parametrize("R,sym,floor", list(brute_cases()))
@pytest.mark.parametrize("separation", [0, 1])
def test_alternative_trajectories_and_the_runner_up_are_the_brute_force_ones(R, sym, floor, separation):
    """G = 3, T = 4, float64: for every frame the best trajectory that is further than ``separation`` from the path voxel in that
    frame - its voxel, its margin and its whole course through the back- and successor pointers - and the segment's runner-up are
    those of the enumeration.  The inputs are such that the enumeration decides each of these choices by more than 1e-9 (asserted:
    no case is skipped)."""
    G, T, N = 3, 4, 27
    p = softmax32(make_logits(T, 1, G, R, seed=9100 + 10 * R + int(sym)))
    w = taps_for(G, R) if sym else ASYM[R]
    mm, arg, score = brute_force_max_marginals(p[:, 0], w, G, floor)
    f, b = run(p, w, G, floor, separation, dtype=np.float64)
    best = np.unravel_index(int(score.argmax()), score.shape)
    top = np.sort(score.reshape(-1))[-2:]
    assert (top[1] - top[0]) / top[1] > 1e-9 and f["index"][:, 0].tolist() == list(best)
    idx = np.arange(N)
    ci, cj, ck = idx // 9, (idx // 3) % 3, idx % 3
    want_margin = np.full(T, np.inf)
    for t in range(T):
        x = best[t]
        far = np.maximum(np.maximum(np.abs(ci - ci[x]), np.abs(cj - cj[x])), np.abs(ck - ck[x])) > separation
        cand = np.where(far, mm[t], 0.0)
        if not (cand > 0).any():
            assert b["alt_index"][t, 0] == -1 and b["margin"][t, 0] == np.inf
            continue
        alt = int(cand.argmax())
        two = np.sort(cand)[-2:]
        assert (two[1] - two[0]) / two[1] > 1e-9, "the alternative voxel is a close call"
        through = np.sort(np.moveaxis(score, t, 0)[alt].reshape(-1))[-2:]
        assert (through[1] - through[0]) / through[1] > 1e-9, "the trajectory through it is a close call"
        assert b["alt_index"][t, 0] == alt
        want_margin[t] = math.log(mm[t, x]) - math.log(mm[t, alt])
        assert abs(b["margin"][t, 0] - want_margin[t]) <= 1e-12 * max(1.0, want_margin[t])
        anchor = np.full((T, 1), -1, dtype=np.int32)
        anchor[t, 0] = alt
        walked, _ = branch_walk(f["back"], b["succ"], f["restarted"], anchor)
        assert walked[:, 0].tolist() == arg[t, alt].tolist(), (t, alt)
    if np.isfinite(want_margin).any():
        # One trajectory is the alternative of every frame in which it keeps clear of the path, with the same margin in each but for
        # rounding: among those frames the anchor may fall on any.  Every other frame must be more than 1e-9 behind.
        t = int(want_margin.argmin())
        near = [u for u in range(T) if want_margin[u] - want_margin[t] <= 1e-9]
        assert all(arg[u, b["alt_index"][u, 0]].tolist() == arg[t, b["alt_index"][t, 0]].tolist() for u in near), "a close call"
        got = np.flatnonzero(b["anchor"][:, 0] >= 0).tolist()
        assert len(got) == 1 and got[0] in near and b["anchor"][got[0], 0] == b["alt_index"][got[0], 0]
        assert b["runner_up_index"][:, 0].tolist() == arg[t, b["alt_index"][t, 0]].tolist()
        assert np.allclose(b["runner_up_margin"][:, 0], want_margin[t], rtol=1e-12, atol=1e-12)
    else:
        assert (b["anchor"] == -1).all() and (b["runner_up_index"] == -1).all() and np.isnan(b["runner_up_margin"]).all()


def test_the_maximum_of_every_frames_max_marginals_is_the_paths_score():
    """G = 4, float64, the seeds of the dense check of the forward model: max_x mm_t(x), with the powers of two of both rescalings put
    back, is the path's score in EVERY frame to 1e-12, and the path voxel attains it."""
    G, T = 4, 6
    for seed in range(24):
        R, floor = (1, 2, 3)[seed % 3], (1e-3, 1e-2, 0.1, 0.0)[seed % 4]
        p = softmax32(make_logits(T, 1, G, R, seed=7000 + seed))
        f, b = run(p, taps_for(G, R), G, floor, 1, dtype=np.float64)
        want = segment_log_scores(f["best"], f["exponent"], f["restarted"])[-1, 0]
        for t in range(T):
            power = f["exponent"][:t + 1, 0].sum() + b["r_exponent"][t + 1:, 0].sum()
            got = math.log(b["mm_best"][t, 0]) + math.log(2.0) * power
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (seed, t, got, want)
        assert np.array_equal(b["mm_peak"], f["index"]) and np.array_equal(b["path_value"], b["mm_best"]), seed
        assert (b["margin"][np.isfinite(b["margin"])] >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ segments
def test_a_nan_frame_gives_two_segments_that_equal_separate_runs_bit_for_bit():
    rows, G, R, T, floor, sep = 2, 8, 2, 5, 1e-3, 1
    p = softmax32(make_logits(T, rows, G, R, seed=5))
    p[2, 1] = np.nan
    w = taps_for(G, R)
    f, b = run(p, w, G, floor, sep)
    assert f["restarted"][:, 1].tolist() == [True, False, True, True, False] and f["index"][2, 1] == -1
    assert b["linked"][:, 1].tolist() == [True, False, False, True, False] and b["linked"][:, 0].tolist() == [True] * 4 + [False]
    assert b["complete"].all() and not b["death"].any()
    assert np.isnan(b["path_value"][2, 1]) and np.isnan(b["alt_value"][2, 1]) and np.isnan(b["mm_best"][2, 1])
    assert b["alt_index"][2, 1] == b["mm_peak"][2, 1] == -1 and np.isnan(b["margin"][2, 1]) and (b["succ"][[1, 2, 4], 1] == -1).all()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)            # noqa: E731
    for t0, t1 in ((0, 2), (3, 5)):
        fa, ba = run(p[t0:t1, 1:2], w, G, floor, sep)
        for key in ("mm", "r", "path_value", "alt_value", "mm_best", "r_best"):
            assert np.array_equal(bits(b[key][t0:t1, 1:2]), bits(ba[key])), key
        for key in ("succ", "alt_index", "mm_peak", "r_exponent", "runner_up_index", "anchor"):
            assert np.array_equal(b[key][t0:t1, 1:2], ba[key]), key
        assert np.array_equal(b["runner_up_margin"][t0:t1, 1:2], ba["runner_up_margin"])
    assert b["runner_up_index"][2, 1] == -1 and np.isnan(b["runner_up_margin"][2, 1])
    # the chunks of a track, last chunk first with the carry, give the bits of one call
    for cuts in ((2, 3), (1, 1, 1, 1, 1), (4, 1)):
        starts = np.concatenate([[0], np.cumsum(cuts)]).tolist()
        carry, parts = None, {}
        for i in range(len(cuts) - 1, -1, -1):
            t0, t1 = starts[i], starts[i + 1]
            sub = {key: f[key][t0:t1] for key in ("state", "restarted")}
            parts[i] = backward_model(p[t0:t1], sub, f["index"][t0:t1], w, G, floor, sep, carry=carry)
            carry = parts[i]["carry"]
        for key in ("mm", "r", "succ", "path_value", "alt_value", "alt_index", "complete", "r_exponent"):
            whole = np.concatenate([parts[i][key] for i in range(len(cuts))])
            assert np.array_equal(whole, b[key], equal_nan=True), (cuts, key)


def test_a_backward_death_is_reported_by_complete():
    """Frame 1 holds one cell, the smallest denormal; the forward pass rescales it and goes on, the backward product with a tap of
    0.25 rounds it to zero: the backward chain restarts there, frames 1 and 0 are not complete, frames 2 and 3 are."""
    G, R, floor, T = 4, 1, 0.0, 4
    N = G ** 3
    w = np.array([0.25, 1.0, 0.25], dtype=np.float32)
    at = lambda i, j, k: (i * G + j) * G + k                           # noqa: E731
    p = np.zeros((T, 1, N), dtype=np.float32)
    p[0, 0, at(1, 1, 1)] = 1.0
    p[1, 0, at(1, 1, 1)] = np.float32(1e-45)                           # the smallest denormal
    p[2, 0, at(1, 1, 2)] = 1.0                                         # one step along k: tap 0.25
    p[3, 0, at(1, 1, 2)] = 0.5
    f, b = run(p, w, G, floor, 0)
    assert f["restarted"][:, 0].tolist() == [True, False, False, False] and f["index"][:, 0].tolist() == [at(1, 1, 1)] * 2 + [at(1, 1, 2)] * 2
    assert b["death"][:, 0].tolist() == [False, True, False, False] and b["complete"][:, 0].tolist() == [0, 0, 1, 1]
    assert b["linked"][:, 0].tolist() == [True, True, True, False]
    assert np.array_equal(b["r"][1], np.ldexp(p[1], 149)) and (b["succ"][1] == -1).all() and np.isnan(b["mm"][1]).all()
    assert np.isnan(b["path_value"][1, 0]) and b["mm_peak"][1, 0] == -1 and np.isnan(b["margin"][1, 0])
    assert b["path_value"][0, 0] > 0 and b["succ"][0, 0, at(1, 1, 1)] == at(1, 1, 1)       # frame 0 is linked to the restarted r
    f64, b64 = run(p, w, G, floor, 0, dtype=np.float64)
    assert b64["complete"].all() and not b64["death"].any()                               # no underflow in float64


# ------------------------------------------------------------------------------------------------------------------ float32 against float64
def trajectory_log_score(p, w, G, floor, path):
    """float64: ln of the product of p_t(x_t) and of the transition scores max(keep W(x_t - x_{t+1}), uniform) along ``path``."""
    N = G ** 3
    R = len(w) // 2
    fl = float(np.float32(floor))
    keep, uniform = 1.0 - fl, fl / N
    w = np.asarray(w, dtype=np.float64)
    total = 0.0
    for t, x in enumerate(path):
        total += math.log(float(p[t, x]))
        if t + 1 < len(path):
            z = path[t + 1]
            d = [x // (G * G) - z // (G * G), (x // G) % G - (z // G) % G, x % G - z % G]      # the predecessor x = z + d
            W = ((w[d[2] + R] * w[d[1] + R]) * w[d[0] + R]) if max(abs(v) for v in d) <= R else 0.0
            total += math.log(max(keep * W, uniform))
    return total


@pytest.mark.parametrize("rows,G,R,T,seed", [(3, 16, 5, 6, 21), (1, 64, 10, 3, 22)])
def test_float32_scores_of_the_runner_up_stay_within_the_counted_roundings_of_float64(rows, G, R, T, seed):
    """``alt_log_score`` = the segment's log score - ln path_value + ln alt_value, all three float32 products along one trajectory
    each.  Per frame such a product takes 5 roundings (three taps, keep, p; a jump takes 2), and mm = s m one more: each of the
    three terms is within (5 T + 1) roundings of 2^-24 of its float64 value, so c = 15 and the bound is (15 T + 3) 2^-24 (first
    order; 1 % slack for the second) - provided nothing underflowed on the way, which the float64 scores of the trajectories
    (above 2^-100 per frame) show.  Compared: the runner-up trajectory's float64 score, recomputed along the trajectory."""
    floor = 1e-3
    p = softmax32(make_logits(T, rows, G, R, seed=seed))
    w = taps_for(G, R)
    f, b = run(p, w, G, floor, 2)
    assert not b["tied"].any() and not f["tied"].any() and b["complete"].all()
    log_score = segment_broadcast(segment_log_scores(f["best"], f["exponent"], f["restarted"]), f["restarted"])
    bound = 1.01 * (15 * T + 3) * 2.0 ** -24
    worst, compared = 0.0, 0
    for r in range(rows):
        if not (b["anchor"][:, r] >= 0).any():           # every cell outside the window is an exact zero: nothing to compare
            assert (b["alt_index"][:, r] == -1).all() and (b["runner_up_index"][:, r] == -1).all()
            continue
        compared += 1
        t = int(np.flatnonzero(b["anchor"][:, r] >= 0)[0])
        got = log_score[t, r] - b["margin"][t, r]
        path = b["runner_up_index"][:, r].tolist()
        assert min(path) >= 0 and path[t] == b["alt_index"][t, r]
        want = trajectory_log_score(p[:, r], w, G, floor, path)
        assert want > T * math.log(2.0 ** -100)
        own = trajectory_log_score(p[:, r], w, G, floor, f["index"][:, r].tolist())
        worst = max(worst, abs(got - want), abs(log_score[t, r] - own))
    print(f"G {G} R {R} T {T}: |alt_log_score - float64 along the runner-up| and the path's own at most {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound and compared >= min(rows, 2)


# ------------------------------------------------------------------------------------------------------------------ the ghost table
def test_the_ghost_table():
    """The README's table: 16^3, R = 5, the true lobe and its ghost 7 voxels away over 8 frames.  Which lobe the path and the
    runner-up follow is gated, not the digits."""
    G, R, floor, sep = 16, 5, 1e-3, 2
    w = taps_for(G, R)
    rows = (("true lobe at 1.02 x", {"true_factor": {t: 1.02 for t in range(8)}}, "true"),
            ("ghost 1.05 x, true 1.3 x in frame 3", {"ghost_factor": 1.05, "true_factor": {3: 1.3}}, "ghost"),
            ("ghost at 1.02 x", {"ghost_factor": 1.02}, "ghost"))
    print("case                                path on   runner-up on   anchor frame   margin")
    for label, kw, leader in rows:
        p, true, ghost, voxel = _ghost(8, **kw)
        f, b = run(p, w, G, floor, sep)
        lobes = {"true": true, "ghost": ghost}
        other = "ghost" if leader == "true" else "true"
        path = voxel[f["index"][:, 0]].astype(np.float64)
        runner = voxel[b["runner_up_index"][:, 0]].astype(np.float64)
        t = int(np.flatnonzero(b["anchor"][:, 0] >= 0)[0])
        m = b["runner_up_margin"][0, 0]
        print(f"{label:35s} {leader:9s} {other:14s} {t:12d}   {m:.3f}  (runner-up {np.linalg.norm(runner - lobes[other], axis=1).max():.2f} "
              f"voxels from the {other} lobe at most; per-frame margins {np.array2string(b['margin'][:, 0], precision=2)})")
        assert (np.linalg.norm(path - lobes[leader], axis=1) < 1.0).all()          # the path: the leading lobe in all 8 frames
        assert (np.linalg.norm(runner - lobes[other], axis=1) < 1.0).all()         # the runner-up: the other lobe in all 8 frames
        assert b["complete"].all() and m > 0 and not b["runner_up_jumped"].any()
    # a lead too strong for the other lobe to be the runner-up: a detour of the same track three voxels wide in one frame costs less
    p, true, ghost, voxel = _ghost(8, true_factor={t: 1.3 for t in range(8)})
    f, b = run(p, w, G, floor, sep)
    runner = voxel[b["runner_up_index"][:, 0]].astype(np.float64)
    away = np.linalg.norm(runner - true, axis=1)
    print(f"true lobe at 1.3 x: runner-up margin {b['runner_up_margin'][0, 0]:.3f}, {away.max():.2f} voxels from the true lobe at most")
    assert (np.linalg.norm(runner - ghost, axis=1) > 6.0).all() and away.max() > sep and (away < 1.0).sum() >= 6


# ------------------------------------------------------------------------------------------------------------------ host helpers, surface
def test_the_packages_margins_and_anchors_are_the_models():
    rows, G, R, T, floor = 3, 8, 3, 6, 1e-3
    p = softmax32(make_logits(T, rows, G, R, seed=11))
    p[3, 1] = 0.0
    f, b = run(p, taps_for(G, R), G, floor, 1)
    assert f["restarted"][:, 1].tolist() == [True, False, False, True, True, False]
    got = path_margins(b["path_value"], b["alt_value"], b["alt_index"], f["index"])
    assert got.dtype == np.float64 and np.array_equal(got, b["margin"], equal_nan=True)
    anchor, broadcast = runner_up_anchors(got, b["alt_index"], f["restarted"])
    assert np.array_equal(anchor, b["anchor"]) and np.array_equal(broadcast, b["runner_up_margin"], equal_nan=True)
    assert ((anchor >= 0).sum(axis=0) == [1, 2, 1]).all()
    # equal margins: the lowest frame
    m = np.array([[0.5], [0.25], [0.25], [np.inf]])
    a, bc = runner_up_anchors(m, np.array([[3], [4], [5], [-1]]), np.array([[1], [0], [0], [0]]))
    assert a[:, 0].tolist() == [-1, 4, -1, -1] and (bc == 0.25).all()
    ls = np.array([[np.nan], [1.5], [np.nan], [2.5]])
    assert segment_broadcast(ls, np.array([[1], [0], [1], [0]]))[:, 0].tolist() == [1.5, 1.5, 2.5, 2.5]


def test_alternatives_needs_the_kept_scores_and_a_sound_separation():
    c = coord_grid(8)
    v = VolumeViterbi(c, 8, SIDE, sigma=0.2, max_bytes=1 << 20)
    assert v.keep_scores is False
    with pytest.raises(ValueError, match="alternatives=True"):
        v.alternatives()
    v = VolumeViterbi(c, 8, SIDE, sigma=0.2, max_bytes=1 << 20, alternatives=True)
    assert v.keep_scores is True and v.bytes_stored == 0
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="separation"):
            v.alternatives(separation=bad)
    with pytest.raises(ValueError, match="nothing is stored"):
        v.alternatives()
    assert len(ALTERNATIVE_KEYS) == 13


def test_binding_lists_the_new_entry_points():
    assert _lib.ABI_VERSION >= 39
    for name, n in (("se_volume_viterbi_keep_f32", 21), ("se_volume_viterbi_back_f32", 31), ("se_volume_viterbi_back_scratch_bytes", 3),
                    ("se_volume_viterbi_branch_i32", 13)):
        assert len(_lib.SIGNATURES[name][1]) == n, name
    assert JUMP == _lib.VITERBI_JUMP and [name for name, _ in _lib.BACK_OUTPUTS] == [
        "mm_best", "mm_peak", "path_value", "alt_value", "alt_index", "complete", "r_best", "r_exponent"]


def test_the_command_line_takes_the_alternatives_flags():
    import evaluate
    import run_sequence
    base = ["--root_dir", "r", "--seq_name", "s"]
    assert run_sequence.parse_args(base + ["--path_output", "p.pkl"]).path.get("separation") is None
    a = run_sequence.parse_args(base + ["--path_alternatives_output", "a.pkl"])
    assert a.path["separation"] == 2 and a.path["refine"] == 1 and a.path_output is None
    assert run_sequence.parse_args(base + ["--path_alternatives_output", "a.pkl", "--path_separation", "0"]).path["separation"] == 0
    for bad in (["--path_separation", "2"], ["--path_output", "p.pkl", "--path_separation", "2"],
                ["--path_alternatives_output", "a.pkl", "--path_separation", "-1"]):
        with pytest.raises(SystemExit):
            run_sequence.parse_args(base + bad)
    e = evaluate.build_parser().parse_args(["--pred_dir", "path.pkl", "--path_alternatives", "alt.pkl"])
    assert e.path_alternatives == "alt.pkl" and e.alternatives is None and e.gt is None


def test_best_of_two_per_joint():
    import evaluate
    rng = np.random.default_rng(0)
    gt = rng.standard_normal((4, 15, 3))
    pred = gt + 0.1
    runner = gt + 0.2
    runner[1, 3] = gt[1, 3]                            # the runner-up is right where the path is not
    runner[2] = np.nan                                 # a frame without a runner-up
    margin = np.full((4, 15), 5.0)
    margin[1, 3], margin[3, 0] = 0.1, np.inf
    frames = [{"runner_up_joints": runner[t], "margin": margin[t]} for t in range(4)]
    r = evaluate.best_of_two_path(frames, pred, gt)
    e = np.sqrt(0.03)
    assert abs(r["best_of_two_mpjpe"] - e * 59 / 60) < 1e-12 and abs(r["runner_up_closer_share"] - 1 / 60) < 1e-12
    assert r["joint_frames_with_margin"] == 59 and abs(r["below_ln2_share"] - 1 / 60) < 1e-12
