"""CPU: the cases of tests/volume_domain_cases.py are what they claim to be.  Every filter and skeleton case is built and run through
its float64 model here, so that a seed whose frames would restart, or whose frames would fall back, fails on a machine without a GPU
and not on the device; the case lists reach the paths they are there for; and the Python layer accepts the odd and the large grids.
Nothing here touches a device."""
import numpy as np
import pytest
import torch

import volume_domain_cases as D
from sceneego_amd import _lib
from sceneego_amd.skeleton_prior import SkeletonPrior
from sceneego_amd.volume_filter import VolumeFilter, default_radius
from test_gpu_skeleton_prior import belief_bound
from test_gpu_volume_filter import e1

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ the filter
@pytest.mark.parametrize("rows,G,R,floor,T", D.FILTER_CASES + [D.FILTER_ALIGN_CASE])
def test_filter_case_meets_the_models_condition(rows, G, R, floor, T):
    k = D.filter_inputs(rows, G, R, T)
    N = G ** 3
    assert k["p"].dtype == np.float32 and k["p"].shape == (T, rows, N) and k["taps"].shape == (2 * R + 1,)
    assert np.isfinite(k["p"]).all() and (np.abs(k["p"].astype(np.float64).sum(axis=-1) - 1.0) < 1e-5).all()
    low = D.filter_condition(D.filter_want(rows, G, R, floor, T), N)
    bound = 2 * (T - 1) * e1(R)
    print(f"rows {rows} G {G} R {R} floor {floor}: evidence x N >= {low:.3g}; belief bound of the last frame {bound / U:.0f} u")
    assert bound < 0.01
    assert 0 <= R <= min(_lib.FILTER_MAX_RADIUS, G - 1) and 2 <= G <= _lib.FILTER_MAX_GRID


def test_filter_cases_reach_what_they_claim():
    grids = {G for _, G, _, _, _ in D.FILTER_CASES}
    assert any(G ** 3 % 4 for G in grids), "no case takes the scalar finish pass"
    assert 2 in grids and max(grids) == 127
    assert any(R == _lib.FILTER_MAX_RADIUS == G - 1 for _, G, R, _, _ in D.FILTER_CASES)
    assert any(floor == 0.0 for _, _, _, floor, _ in D.FILTER_CASES)
    assert D.FILTER_ALIGN_CASE[1] ** 3 % 4 == 0                  # the fast pass is what an offset base turns off
    assert D.FILTER_CUT_CASE in D.FILTER_CASES and D.FILTER_CUT_CASE[1] % 2 == 1


# ------------------------------------------------------------------------------------------------------------------ the skeleton
@pytest.mark.parametrize("frames,tree,G,R,floor", D.SKELETON_CASES + [D.SKELETON_BATCH_CASE])
def test_skeleton_case_meets_the_models_condition(frames, tree, G, R, floor):
    k = D.skeleton_inputs(frames, tree, G, R)
    J, N = len(k["parents"]), G ** 3
    assert k["p"].dtype == np.float32 and k["p"].shape == (frames, J, N) and k["taps"].shape == (J, (2 * R + 1) ** 3)
    small = D.skeleton_condition(D.skeleton_want(frames, tree, G, R, floor))
    B = belief_bound(k["parents"], R)
    print(f"frames {frames} {tree} G {G} R {R} floor {floor}: smallest normaliser {small:.3g}; belief bound {B / U:.0f} u")
    assert B < 0.01
    assert 0 <= R <= min(_lib.SKELETON_MAX_RADIUS, G - 1) and 1 <= J <= _lib.SKELETON_MAX_JOINTS


def test_skeleton_cases_reach_what_they_claim():
    cases = D.SKELETON_CASES
    assert any(G > 64 for _, _, G, _, _ in cases) and any(G % 2 for _, _, G, _, _ in cases)
    assert any(G > 64 and G % 2 for _, _, G, _, _ in cases)
    assert any(R == _lib.SKELETON_MAX_RADIUS == 24 for _, _, _, R, _ in cases)
    assert sum(len(D.TREES[t]) == _lib.SKELETON_MAX_JOINTS == 32 for _, t, _, _, _ in cases) == 3
    for name in ("chain32", "heap2_32", "heap4_32"):
        par = D.TREES[name]
        assert par[0] == 0 and all(0 <= par[j] < j for j in range(1, 32))
    depth = [0] * 32
    for j in range(1, 32):
        depth[j] = depth[D.TREES["chain32"][j]] + 1
    assert max(depth) == 31
    kids = lambda par: max(sum(1 for c in range(1, 32) if par[c] == j) for j in range(32))
    assert kids(D.TREES["heap2_32"]) == 2 and kids(D.TREES["heap4_32"]) == 4
    # the model's FFT form needs a floor: every case it serves has one
    assert all(floor > 0 for _, _, G, _, floor in cases if D.skeleton_method(G) == "fft")
    assert D.SKELETON_BATCH_CASE[0] == 5 and D.SKELETON_BATCH_CASE[2] % 2 == 1
    assert all((G + 63) // 64 == 2 for G, _ in D.CORRELATE_CASES) and all(G % 4 for G, _ in D.CORRELATE_CASES)
    G, R, bones = D.CORRELATE_DEEP
    assert (G + 63) // 64 == 2 and R == _lib.SKELETON_MAX_RADIUS and (1, "chain3", G, R, 1e-3) in cases and max(bones) + 1.5 < R


@pytest.mark.parametrize("G,R", D.CORRELATE_CASES)
def test_correlation_inputs_and_voxels(G, R):
    k = D.correlate_inputs(G, R)
    assert k["a"].shape == (2, G ** 3) and k["a"].dtype == np.float32 and (k["a"] > 0).all()
    assert k["taps"].shape == (3, (2 * R + 1) ** 3) and not np.array_equal(k["taps"][1], k["taps"][2])
    v = D.correlate_voxels(G)
    last_plane = np.arange(G * G) + (G - 1) * G * G
    assert np.isin(last_plane, v).all() and v.max() == G ** 3 - 1
    n = np.arange(G ** 3)
    assert np.isin(n[n % G >= 64], v).all() and len(v) >= 4096 + G * G


# ------------------------------------------------------------------------------------------------------------------ the guards
def test_guarded_views_on_the_host():
    for dtype, numel, off in ((torch.float32, 27, 0), (torch.float32, 27, 4), (torch.int32, 3, 4), (torch.uint8, 1001, 0)):
        view, check = D.guarded(numel, dtype, off, device="cpu")
        assert view.numel() == numel and view.dtype == dtype and view.is_contiguous() and view.data_ptr() % 4 == 0
        check()
        view.zero_()
        check()
    view, check = D.guarded(8, torch.float32, 4, device="cpu")
    check.buffer[D.GUARD_BYTES + 3] = 0     # one byte of the skipped offset: the band before
    with pytest.raises(AssertionError):
        check()
    view, check = D.guarded(8, torch.float32, 0, device="cpu")
    check.buffer[D.GUARD_BYTES + 32] = 0     # the first byte behind the payload
    with pytest.raises(AssertionError):
        check()
    assert D.GUARD_BYTES >= 64 * 1024 and D.GUARD_BYTES >= 128 * 128 * 4
    x = D.nan_banded(np.arange(6, dtype=np.float32), 4, device="cpu")
    assert x.tolist() == [0, 1, 2, 3, 4, 5]
    whole = x.buffer
    assert torch.isnan(whole[:D.GUARD_BYTES].view(torch.float32)).all() and torch.isnan(whole[-D.GUARD_BYTES:].view(torch.float32)).all()


# ------------------------------------------------------------------------------------------------------------------ the classes
def test_the_classes_accept_the_domain_without_a_device():
    side, G = 2.0, 96
    coord = np.zeros((1, 3), dtype=np.float32)                   # refused by its size only after the radius is checked
    with pytest.raises(ValueError) as err:
        SkeletonPrior(coord, G, side, np.linspace(0.15, 0.45, 14))
    assert "26 voxels" in str(err.value) and "24" in str(err.value)
    coord96 = torch.zeros((G ** 3, 3))
    s = SkeletonPrior(coord96, G, side, np.linspace(0.15, 0.40, 14))
    assert s.radius == int(np.ceil((0.40 + 0.09) / (side / G))) == 24 <= _lib.SKELETON_MAX_RADIUS
    assert s.taps.shape == (15, 49 ** 3) and s.joints == 15 and not s._dev
    coord9 = torch.zeros((9, 9, 9, 3))
    f = VolumeFilter(coord9, 9, side, sigma=0.10)
    assert f.radius == default_radius(0.10, 9, side) == min(16, 8, int(np.ceil(0.30 / (side / 9)))) == 2
    assert f.taps.shape == (5,) and f.voxels == 729 and f.state is None and not f._dev
    assert VolumeFilter(coord9, 9, side, sigma=1.0).radius == 8                         # G - 1 caps it
    assert VolumeFilter(torch.zeros((8, 3)), 2, side, sigma=1.0).radius == 1
    assert SkeletonPrior(coord9, 9, side, [0.5, 0.3], parents=(0, 0, 1)).radius == int(np.ceil((0.5 + 0.09) / (side / 9))) == 3
