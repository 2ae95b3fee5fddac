"""CPU: the numpy model of the trajectory sampler (tests/volume_sampler_model.py) draws from the law it claims to: the generator is
Philox4x32-10, the conditional of a frame given the next equals the one of the dense transition matrix, the sample frequencies agree
with the smoothed marginals and with the pairwise posterior, the results do not depend on how the work is cut, a NaN stays in its
frame, and the Python surface refuses bad arguments before anything touches a device."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from sceneego_amd import _lib
from sceneego_amd.volume_smoother import VolumeSmoother
from volume_filter_cases import SIDE, coord_grid, make_logits, softmax32, taps_for
from volume_filter_model import blur3, volume_filter_model
from volume_sampler_model import (FRESH, JUMP, STEP, M0, M1, W0, W1, conditional_law, constants, draw, last_positive, philox4x32_10,
                                  sample_in_chunks, search, uniform53, volume_sampler_model)
from volume_smoother_model import volume_smoother_model

G, R, ROWS, T, S = 4, 2, 2, 4, 4096
N = G ** 3
FLOORS = (0.0, 1e-2, 0.3)
ASYM = np.array([0.05, 0.10, 0.20, 0.30, 0.35])


def asymmetric_taps():
    return (ASYM / ASYM.sum()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(floor, asym=False, frames=T):
    """Two rows (the second two-lobed) over ``frames`` frames at G = 4: the volumes, the filter model's beliefs rounded to float32 (what
    the sampler takes) and its restart flags.  Shared; nothing below modifies it.  The logits are the filter tests' own, unscaled."""
    p = softmax32(make_logits(frames, ROWS, G, R, seed=23))
    c = coord_grid(G)
    w = asymmetric_taps() if asym else taps_for(G, R)
    b, _, _, rs = volume_filter_model(p, c, w, G, floor)
    assert rs[0].all() and not rs[1:].any()
    return {"p": p, "c": c, "w": w, "b": b.astype(np.float32), "rs": rs}


def dense_transition(w, floor, grid=G):
    """D[x, y] = keep W(x -> y) + uniform, W from blur3 itself: column m of K is blur3 of the unit vector at m, so K[y, x] is the weight
    with which b(x) enters q(y).  keep and uniform are the definition's: formed in float32 as the filter's kernels form them.
    ``grid``: another grid than this file's (tests/test_path_sampler_domain_host.py takes it at 3^3)."""
    n = grid ** 3
    K = np.stack([blur3(np.eye(n)[m][None], w, grid)[0] for m in range(n)], axis=1)
    keep, uniform = constants(floor, n)
    return keep * K.T + uniform


def conditional_law_error(b, w, floor, grid=G):
    """Worst |conditional_law - b(x) D[x, y] normalised| as a share of the peak, over every y, for one belief ``b`` [grid^3] float32."""
    D = dense_transition(w, floor, grid)
    worst = 0.0
    for y in range(grid ** 3):
        want = b.astype(np.float64) * D[:, y]
        want /= want.sum()
        worst = max(worst, float(np.abs(conditional_law(b, y, w, grid, floor) - want).max() / want.max()))
    return worst


def bound(prob):
    return 5.0 * np.sqrt(prob * (1.0 - prob) / S) + 1.0 / S


# ------------------------------------------------------------------------------------------------------------------ the generator
def test_philox_known_answers():
    """The known-answer vectors of Philox4x32-10 as Random123 publishes them (kat_vectors: counter and key all zero, all ones, and the
    digits of pi), quoted from memory.  What settled them: this model was written from the round function of the SC'11 paper alone and
    gives all three, 384 bits that nothing was bent to; the multipliers and Weyl constants are, besides, those of rocRAND's
    rocrand_philox4x32_10.h where that header is installed (compared below when it is)."""
    f = 0xFFFFFFFF
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
                           ((f, f, f, f), (f, f), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
                           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
                            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))):
        got = philox4x32_10(np.array(ctr), np.array(key))
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]
    # vectorised over counters: the same words
    ctr = np.array([[0, 0, 0, 0], [f, f, f, f]])
    key = np.array([[0, 0], [f, f]])
    got = philox4x32_10(ctr, key)
    assert int(got[0, 0]) == 0x6627E8D5 and int(got[1, 3]) == 0x6D5451FD
    header = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include", "rocrand", "rocrand_philox4x32_10.h")
    if os.path.isfile(header):
        text = open(header).read()
        found = {int(x, 16) for x in re.findall(r"0x[0-9A-Fa-f]{8}", text)}
        assert {M0, M1, W0, W1} <= found
    # the kernel's header carries the same four constants
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "sceneego_amd", "csrc", "categorical_draw.h")).read()
    assert {M0, M1, W0, W1} <= {int(x, 16) for x in re.findall(r"0x[0-9A-Fa-f]{8}", text)}


def test_uniforms_lie_in_the_unit_interval_and_are_exact():
    assert uniform53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 and uniform53(0, 0) == 0.0 and uniform53(0, 0x7FF) == 0.0
    assert uniform53(0x80000000, 0) == 0.5 and uniform53(0, 0x800) == 2.0 ** -53


def test_the_vectorised_search_is_the_scalar_draw():
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 33, 128):
        v = rng.random((64, n)) * (rng.random((64, n)) > 0.4)          # exact zeros among the values
        v[0] = 0.0                                                     # no mass: no draw
        v[1, :] = np.nan
        u = rng.random(64)
        u[2], u[3] = 0.0, 1.0 - 2.0 ** -53
        with np.errstate(invalid="ignore"):
            got = search(np.cumsum(v, axis=1), last_positive(v), u)
        want = np.array([draw(v[s], u[s]) for s in range(64)])
        assert np.array_equal(got, want)
        assert got[0] == -1 and got[1] == -1
        ok = got >= 0
        assert (v[ok, got[ok]] > 0).all()                              # a value of 0 is never drawn
    # the rounding edge: a total so small that u total rounds up to the total; the last positive value is the draw
    tiny = np.array([0.0, 5e-324, 0.0])
    assert draw(tiny, 1.0 - 2.0 ** -53) == 1 and search(np.cumsum(tiny)[None], last_positive(tiny)[None], np.array([1.0 - 2.0 ** -53]))[0] == 1


# ------------------------------------------------------------------------------------------------------------------ the law
@pytest.mark.parametrize("floor", FLOORS)
def test_the_conditional_law_equals_the_dense_transition_matrix(floor):
    """No sampling noise: for every frame, row and y the N probabilities the model's own masses imply against b_t(x) D[x, y] normalised."""
    worst = 0.0
    for asym in (False, True):
        k = case(floor, asym)
        D = dense_transition(k["w"], floor)
        for t in range(T):
            for row in range(ROWS):
                b = k["b"][t, row].astype(np.float64)
                for y in range(N):
                    want = b * D[:, y]
                    want /= want.sum()
                    got = conditional_law(k["b"][t, row], y, k["w"], G, floor)
                    worst = max(worst, float(np.abs(got - want).max() / want.max()))
    print(f"floor {floor}: conditional law against the dense matrix, worst {worst:.3e} of the peak")
    assert worst <= 1e-12


@pytest.mark.parametrize("floor", FLOORS)
def test_a_reversed_tap_model_is_visibly_wrong_with_asymmetric_taps(floor):
    k = case(floor, True)
    D = dense_transition(k["w"], floor)
    rev = np.ascontiguousarray(k["w"][::-1])
    least = np.inf
    for t in range(T):
        for row in range(ROWS):
            b = k["b"][t, row].astype(np.float64)
            off = 0.0
            for y in range(N):
                want = b * D[:, y]
                want /= want.sum()
                off = max(off, float(np.abs(conditional_law(k["b"][t, row], y, rev, G, floor) - want).max() / want.max()))
            least = min(least, off)
    assert least > 1e-3, least


# ------------------------------------------------------------------------------------------------------------------ the statistics
@functools.lru_cache(maxsize=None)
def drawn(floor, asym=False):
    k = case(floor, asym)
    return volume_sampler_model(k["b"], k["rs"], k["w"], G, floor, S, seed=0)


@pytest.mark.parametrize("floor,asym", [(f, False) for f in FLOORS] + [(1e-2, True)])
def test_sample_frequencies_match_the_smoothed_marginals_and_the_pairwise_posterior(floor, asym):
    """S = 4096, seed 0: |f - prob| <= 5 sqrt(prob (1 - prob) / S) + 1 / S for every frame, row and state against the smoothed marginal,
    and for every pair of states of the two last frames against the dense pairwise posterior.  A condition on the sampler, not a knob.

    What the bound is worth.  It is a five-sigma bound where the expected count S prob is large; in a cell that expects between 0.01
    and 1 counts the count is Poisson and passes the bound with a probability of up to 1.5e-4, not 6e-7 (expected 0.26, observed 4 is
    such an event).  The exact binomial probability that a CORRECT sampler fails the test, summed over the cells of a case from the
    reference laws alone (the smoother model's marginals, the dense pair posterior), is 6e-3 for the marginals and 1e-2 for the pairs
    of these inputs; with the same logits scaled by 0.3 (flatter volumes, more cells in the Poisson band) it is 2e-2 and 8e-2 to 0.15,
    with logits scaled by 3 it is 4e-4 and 1e-3, but the beliefs are then nearly one-hot and the test sees few cells.  The inputs are
    the filter tests' own logits, unscaled.  The law itself is tested without noise above."""
    k = case(floor, asym)
    got = drawn(floor, asym)
    assert (got["index"] >= 0).all() and (got["kind"][:, T - 1] == FRESH).all() and (got["kind"][:, :T - 1] != FRESH).all()
    gamma = volume_smoother_model(k["p"], k["b"], k["rs"], k["c"], k["w"], G, floor)["gamma"]
    worst = 0.0
    for t in range(T):
        for row in range(ROWS):
            f = np.bincount(got["index"][:, t, row], minlength=N) / S
            excess = np.abs(f - gamma[t, row]) - bound(gamma[t, row])
            worst = max(worst, float(excess.max()))
    assert worst <= 0.0, f"a marginal frequency is {worst:.3e} beyond five sigma"
    D = dense_transition(k["w"], floor)
    for row in range(ROWS):
        b1, b0 = k["b"][T - 1, row].astype(np.float64), k["b"][T - 2, row].astype(np.float64)
        cond = b0[:, None] * D                                     # [x, y]
        pair = cond / cond.sum(axis=0, keepdims=True) * (b1 / b1.sum())[None, :]
        f = np.bincount(got["index"][:, T - 2, row].astype(np.int64) * N + got["index"][:, T - 1, row], minlength=N * N) / S
        excess = np.abs(f - pair.reshape(-1)) - bound(pair.reshape(-1))
        assert excess.max() <= 0.0, f"a pair frequency of row {row} is {excess.max():.3e} beyond five sigma"
    if floor == 0.0:
        assert not (got["kind"] == JUMP).any()
    if floor == 0.3:
        assert (got["kind"] == JUMP).any() and (got["kind"] == STEP).any()


# ------------------------------------------------------------------------------------------------------------------ invariance
def test_results_do_not_depend_on_how_frames_and_samples_are_cut():
    floor = 1e-2
    k = case(floor)
    whole = volume_sampler_model(k["b"], k["rs"], k["w"], G, floor, 16, seed=7)
    for cuts in ((1, 3), (2, 2), (3, 1), (1, 1, 1, 1)):
        cut = sample_in_chunks(k["b"], k["rs"], k["w"], G, floor, 16, cuts, seed=7)
        for key in ("index", "kind", "next"):
            assert np.array_equal(cut[key], whole[key]), (cuts, key)
    lo = volume_sampler_model(k["b"], k["rs"], k["w"], G, floor, 8, seed=7)
    hi = volume_sampler_model(k["b"], k["rs"], k["w"], G, floor, 8, seed=7, first_sample=8)
    for key, axis in (("index", 0), ("kind", 0), ("next", 0)):
        assert np.array_equal(np.concatenate([lo[key], hi[key]], axis=axis), whole[key]), key
    other = volume_sampler_model(k["b"], k["rs"], k["w"], G, floor, 16, seed=8)
    assert not np.array_equal(other["index"], whole["index"])
    assert np.array_equal(whole["next"], whole["index"][:, 0]) and whole["index"].dtype == np.int32


# ------------------------------------------------------------------------------------------------------------------ NaN, extremes
def test_a_nan_frame_in_the_middle():
    floor, frames = 1e-2, 5
    k = case(floor, frames=frames)
    clean_b, clean_rs = k["b"], k["rs"]
    p = k["p"].copy()
    p[2, 0, 17] = np.nan
    b, _, _, rs = volume_filter_model(p, k["c"], k["w"], G, floor)
    b = b.astype(np.float32)
    assert rs[:, 0].tolist() == [True, False, True, True, False] and rs[:, 1].tolist() == [True] + [False] * 4
    got = volume_sampler_model(b, rs, k["w"], G, floor, 64, seed=3)
    # the NaN frame is invalid; the frame after it restarted, so the frame before the restart (1) is a fresh draw, and so is the last
    assert (got["index"][:, 2, 0] == -1).all() and (got["kind"][:, 2, 0] == FRESH).all()
    assert (got["kind"][:, 1, 0] == FRESH).all() and (got["kind"][:, 4, 0] == FRESH).all()
    assert (got["kind"][:, 0, 0] != FRESH).all() and (got["kind"][:, 3, 0] != FRESH).all()
    assert (got["index"][:, [0, 1, 3, 4], 0] >= 0).all()
    # the chain on both sides is intact: each side equals the same frames sampled as a track of their own (global frame indices kept)
    tail = volume_sampler_model(b[3:], rs[3:], k["w"], G, floor, 64, seed=3, first_frame=3)
    head = volume_sampler_model(b[:2], rs[:2], k["w"], G, floor, 64, seed=3)
    assert np.array_equal(got["index"][:, 3:, 0], tail["index"][:, :, 0]) and np.array_equal(got["kind"][:, 3:, 0], tail["kind"][:, :, 0])
    assert np.array_equal(got["index"][:, :2, 0], head["index"][:, :, 0]) and np.array_equal(got["kind"][:, :2, 0], head["kind"][:, :, 0])
    # the other row is that of the clean sequence
    clean = volume_sampler_model(clean_b, clean_rs, k["w"], G, floor, 64, seed=3)
    assert np.array_equal(got["index"][:, :, 1], clean["index"][:, :, 1]) and np.array_equal(got["kind"][:, :, 1], clean["kind"][:, :, 1])


def test_floor_extremes_and_exact_zeros():
    k = case(1e-2)
    one = volume_sampler_model(k["b"], k["rs"], k["w"], G, 1.0, 256, seed=1)
    assert (one["kind"][:, :T - 1] == JUMP).all() and (one["kind"][:, T - 1] == FRESH).all() and (one["index"] >= 0).all()
    zero = volume_sampler_model(k["b"], k["rs"], k["w"], G, 0.0, 256, seed=1)
    assert (zero["kind"][:, :T - 1] == STEP).all()
    # a belief with exact zeros never yields a zero cell, by a step, a jump or a fresh draw
    rng = np.random.default_rng(9)
    sparse = k["b"] * (rng.random(k["b"].shape) > 0.6)
    assert (sparse == 0).mean() > 0.5
    got = volume_sampler_model(sparse, k["rs"], k["w"], G, 0.3, 512, seed=2)
    assert {STEP, JUMP, FRESH} <= set(np.unique(got["kind"]).tolist())
    for t in range(T):
        for row in range(ROWS):
            x = got["index"][:, t, row]
            assert (x >= 0).all() and (sparse[t, row, x] > 0).all()
    # a frame of zeros has no mass: invalid, and the frame before it is a fresh draw
    dead = k["b"].copy()
    dead[2, 1] = 0.0
    got = volume_sampler_model(dead, k["rs"], k["w"], G, 1e-2, 32, seed=2)
    assert (got["index"][:, 2, 1] == -1).all() and (got["kind"][:, 1, 1] == FRESH).all() and (got["index"][:, [0, 1, 3], 1] >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ the surface
def test_binding_and_scratch_size():
    assert "se_volume_sample_f32" in _lib.SIGNATURES and "se_volume_sample_scratch_bytes" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["se_volume_sample_f32"][1]) == 21
    assert (_lib.SAMPLE_STEP, _lib.SAMPLE_JUMP, _lib.SAMPLE_FRESH) == (STEP, JUMP, FRESH)
    lib = _lib.load()
    assert lib.se_volume_sample_scratch_bytes(3, 15, 64) == 3 * 15 * (64 * 64 + 64) * 8
    assert lib.se_volume_sample_scratch_bytes(0, 15, 64) == 0 and lib.se_volume_sample_scratch_bytes(1, 0, 64) == 0
    assert lib.se_volume_sample_scratch_bytes(1, 1, 129) == 0 and lib.se_volume_sample_scratch_bytes(1, 1, 1) == 0
    assert lib.se_volume_sample_scratch_bytes(1, 65535, 128) == 65535 * (128 * 128 + 128) * 8
    assert lib.se_volume_sample_scratch_bytes(2 ** 31 - 1, 1, 128) == (2 ** 31 - 1) * (128 * 128 + 128) * 8
    assert lib.se_volume_sample_scratch_bytes(2 ** 31 - 1, 65535, 128) == 0          # 1.9e19 bytes: no size a long long holds
    z = torch.zeros((1, 1, 8))
    i = torch.zeros((1, 1, 1), dtype=torch.int32)
    with pytest.raises(_lib.HipExtensionError):
        _lib.volume_sample(z, torch.zeros((1, 1), dtype=torch.int32), torch.ones(1), torch.zeros((1, 1), dtype=torch.int32), i, i.clone(),
                           1, 1, 8, 2, 0, 1e-3, 1)
    for kw in ({"samples": 0}, {"first_sample": -1}, {"first_frame": 2 ** 32}, {"seed": -1}, {"seed": 2 ** 64}):
        a = {"samples": 1, "first_sample": 0, "first_frame": 0, "seed": 0}
        a.update(kw)
        with pytest.raises(_lib.HipExtensionError, match="expected"):
            _lib.volume_sample(z, torch.zeros((1, 1), dtype=torch.int32), torch.ones(1), torch.zeros((1, 1), dtype=torch.int32), i,
                               i.clone(), 1, 1, 8, 2, 0, 1e-3, **a)


def test_sample_refuses_bad_arguments_without_a_device():
    s = VolumeSmoother(coord_grid(G), G, SIDE, sigma=0.1, radius=R)
    for kw in ({"samples": 0}, {"samples": -3}, {"samples": 1.5}, {"samples": True}, {"seed": -1}, {"seed": 2 ** 64}, {"seed": 0.5}):
        with pytest.raises(ValueError, match="sample:"):
            s.sample(**kw)
    with pytest.raises(ValueError, match="nothing is stored"):
        s.sample()
    s.reset()
    with pytest.raises(ValueError, match="nothing is stored"):
        s.sample(samples=4, seed=1)
