"""CPU: the numpy model of the scene distance field holds together, and the case lists of tests/test_gpu_scene_field.py contain what
they say they contain.

The separable three-pass transform that carries the key (d2, index) is held to the definition - brute force over all (voxel, site)
pairs in exact integers - exhaustively at G = 2, on random patterns at G = 3, 5, 8, 9 and 16, on the empty grid, the full grid and
built ties, and at 64^3 against a few hundred sites."""
import numpy as np
import pytest

import scene_field_cases as C
import scene_field_model as M


def both(sites, G):
    s = np.asarray(sites, dtype=np.uint8).reshape(-1)
    want = M.distance_brute(s, G)
    got = M.distance_separable(s, G)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]), f"G {G}: {int((got[0] != want[0]).sum())} distances differ"
    assert np.array_equal(got[1], want[1]), f"G {G}: {int((got[1] != want[1]).sum())} nearest indices differ"
    return want


def test_separable_equals_brute_force_on_all_256_patterns_at_2():
    for pattern in range(256):
        s = np.array([(pattern >> n) & 1 for n in range(8)], dtype=np.uint8)
        d2, near = both(s, 2)
        if pattern == 0:
            assert (d2 == M.NO_SITE).all() and (near == -1).all()
        else:
            assert d2.max() <= 3 and (s[near] == 1).all() and (d2[s == 1] == 0).all()


@pytest.mark.parametrize("G", [3, 5, 8, 9, 16])
def test_separable_equals_brute_force_on_random_patterns(G):
    g = np.random.default_rng(G)
    for density in (1.5 / G ** 3, 0.02, 0.3, 0.9):
        s = (g.random(G ** 3) < density).astype(np.uint8) * g.choice(np.array([1, 7, 255], dtype=np.uint8), size=G ** 3)
        both(s, G)


@pytest.mark.parametrize("G", [2, 3, 8, 9])
def test_empty_and_full_grids(G):
    N = G ** 3
    d2, near = both(np.zeros(N, dtype=np.uint8), G)
    assert (d2 == 0x7fffffff).all() and (near == -1).all()
    d2, near = both(np.ones(N, dtype=np.uint8), G)
    assert (d2 == 0).all() and np.array_equal(near, np.arange(N))


def test_built_ties_go_to_the_lower_index():
    G = 9
    name, g, frames = next(c for c in C.transform_cases() if c[0] == "equidistant pairs")
    assert g == G
    centre = (4 * G + 4) * G + 4
    for b, (a_site, b_site) in enumerate([((4, 4, 2), (4, 4, 6)), ((4, 2, 4), (4, 6, 4)), ((2, 4, 4), (6, 4, 4))]):   # along k, j, i
        d2, near = both(frames[b], G)
        lo, hi = C._flat(G, a_site, b_site)
        assert lo < hi and d2[centre] == 4 and near[centre] == lo
    d2, near = both(frames[3], G)                            # three sites at distance 1 from the origin, one per axis
    assert d2[0] == 1 and near[0] == min(C._flat(G, (0, 1, 0), (1, 0, 0), (0, 0, 1)))
    # ties that no single pass sees on its own line: the 81 voxels with i == j are equidistant from (1, 7, 3) and (7, 1, 3)
    for b, least in ((4, 81), (5, 1)):
        d2, near = both(frames[b], G)
        ties = 0
        sites = np.flatnonzero(frames[b])
        for n in range(G ** 3):
            q = sorted(((n // 81 - m // 81) ** 2 + ((n // 9) % 9 - (m // 9) % 9) ** 2 + (n % 9 - m % 9) ** 2, m) for m in sites)
            ties += q[0][0] == q[1][0]
            assert (d2[n], near[n]) == q[0]
        assert ties >= least, "the case holds too few equidistant voxels"


def test_separable_equals_brute_force_at_64_cubed():
    G = 64
    g = np.random.default_rng(64)
    s = np.zeros(G ** 3, dtype=np.uint8)
    s[g.choice(G ** 3, size=500, replace=False)] = 1
    s[C.corners(G)] = 1
    d2, near = both(s, G)
    assert 0 < d2.max() < 3 * 63 * 63


def test_transform_cases_meet_their_conditions():
    cases = {name: (G, s) for name, G, s in C.transform_cases()}
    G, s = cases["all 256 patterns"]
    assert G == 2 and s.shape == (256, 8) and len({bytes(r) for r in s}) == 256
    assert {G for G, _ in cases.values()} >= {2, 3, 5, 9, 17, 33, 16, 64, 127, 128}
    for G in (3, 5, 9, 17, 33):
        assert cases[f"odd grid {G}"][1].any(axis=1).all()
    for G in (16, 64):
        s = cases[f"densities at {G}"][1]
        assert not s[0].any() and s[2].all() and 0.005 < (s[1] != 0).mean() < 0.02
    for G in (127, 128):
        s = cases[f"corners at {G}"][1]
        assert ((s != 0).sum(axis=1) <= 64).all() and (s[2][C.corners(G)] != 0).all()
        # one corner alone: the opposite corner lies 3 (G - 1)^2 away, 48 387 at G = 128
        assert np.flatnonzero(s[0]).tolist() == [0] and np.flatnonzero(s[1]).tolist() == [G ** 3 - 1]
    assert 3 * 127 * 127 == 48387
    G, s = cases["single plane"]
    for b, axis in enumerate((0, 1, 2)):
        at = np.argwhere(s[b].reshape(G, G, G) != 0)
        assert len(at) == G * G and len(set(at[:, axis])) == 1
    G, s = cases["empty and full frames"]
    kinds = {(int(r.any()), int(r.all())) for r in s}
    assert kinds == {(0, 0), (1, 1), (1, 0)}
    for name, G, s in C.transform_cases():
        assert s.dtype == np.uint8 and s.shape[1] == G ** 3 and 2 <= G <= 128, name
    # any non-zero byte is a site: the random cases carry site bytes other than 1
    assert all(set(np.unique(cases[f"odd grid {G}"][1])) >= {0, 1, 2, 255} for G in (9, 17, 33))


@pytest.mark.parametrize("G,side", C.SITE_GRIDS)
@pytest.mark.parametrize("dh,dw", C.SITE_DEPTH_SHAPES)
def test_sites_cases_meet_their_conditions(G, side, dh, dw):
    depth, ray, planted = C.sites_case(G, side, dh, dw)
    assert depth.dtype == np.float32 and ray.dtype == np.float64 and ray.shape == (C.FRAME_H, C.FRAME_W, 3)
    h = side / (G - 1)
    assert h == 2.0 ** round(np.log2(h)), "the voxel spacing must be a power of two"
    want = M.sites(depth, ray, G, side, C.MIN_Z, C.MAX_DEPTH)
    kinds = {p[0] for p in planted}
    assert {"depth 0", "depth negative", "depth NaN", "depth above max_depth", "z == min_z", "z below min_z", "ray NaN", "ray +inf",
            "outside low x", "outside high x", "outside low y", "outside high y", "outside high z", "half to even, down",
            "half to even, up"} <= kinds
    halves = outside = 0
    for kind, b, y, x, q, voxel in planted:
        py, px = (y * dh) // C.FRAME_H, (x * dw) // C.FRAME_W
        d = float(depth[b, py, px])
        if q is None:
            if kind.startswith("depth"):
                assert not (d > 0.0 and d <= C.MAX_DEPTH), kind
            elif kind.startswith("z"):
                assert ray[y, x, 2] * d <= C.MIN_Z and ray[y, x, 2] * d > 0, kind
                assert (ray[y, x, 2] * d == C.MIN_Z) == (kind == "z == min_z")
            else:
                assert not np.isfinite(ray[y, x]).all(), kind
            continue
        s = ray[y, x] * d
        got = (((s[0] + side / 2.0) * (G - 1)) / side, ((s[1] + side / 2.0) * (G - 1)) / side, (s[2] * (G - 1)) / side)
        assert got == tuple(float(v) for v in q), (kind, got, q)          # the planted coordinate is exact
        r = [float(np.rint(v)) for v in got]
        inside = all(0 <= v <= G - 1 for v in r)
        halves += any(v - np.floor(v) == 0.5 for v in got)
        outside += not inside
        if voxel is None:
            assert not inside, kind
        else:
            assert inside and tuple(int(v) for v in r) == voxel, (kind, r, voxel)
            assert want[b, (voxel[0] * G + voxel[1]) * G + voxel[2]] == 1, kind
    assert halves >= 8 and outside >= 6
    assert 0 < want.mean() < 0.5


def test_sites_model_marks_nothing_for_an_empty_frame():
    depth, ray, _ = C.sites_case(9, 2.0, 16, 20)
    assert not M.sites(np.zeros_like(depth), ray, 9, 2.0, C.MIN_Z, C.MAX_DEPTH).any()
    assert not M.sites(np.full_like(depth, np.nan), ray, 9, 2.0, C.MIN_Z, C.MAX_DEPTH).any()


def test_reduction_cases_meet_their_conditions():
    import re
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "test_gpu_scene_constraint.py")).read()
    block = re.search(r"CASES = \[(.*?)\]\s*#[^\n]*\n\n", text, flags=re.S).group(1)
    theirs = [(int(a), int(b)) for a, b in re.findall(r"\((\d+), (\d+)\)", block)]
    assert [(r, G) for r, G, _ in C.REDUCTION_CASES] == theirs, "the (rows, G) cases of tests/test_gpu_scene_constraint.py"
    ks = {len(r) for _, _, r in C.REDUCTION_CASES}
    assert {1, 8} <= ks
    assert any(0 in r for _, _, r in C.REDUCTION_CASES) and any(48387 in r for _, _, r in C.REDUCTION_CASES)
    assert all(list(r) == sorted(r) for _, _, r in C.REDUCTION_CASES)
    assert {1 if rows % 15 else 15 for rows, _, _ in C.REDUCTION_CASES} == {1, 15}
    d2, free = C.reduction_field(3, 8, seed=1)
    assert (d2[2] == M.NO_SITE).all() and (d2[:2] < M.NO_SITE).all() and (d2[:2] == 0).sum() == 10
    assert set(np.unique(free)) == {0, 1, 2, 255}


def test_expectation_model_on_a_one_hot_volume():
    G = 4
    N = G ** 3
    d2, free = C.reduction_field(1, G, seed=3)
    p = np.zeros((1, N), dtype=np.float32)
    p[0, 37] = 1.0
    out, mag = M.expectation(p, d2, free, (0, 2, 48387), 1)
    f = free[0, 37] != 0
    assert out[0, 0] == 1 and out[0, 1] == (0 if f else 1)
    assert out[0, 2] == np.sqrt(float(d2[0, 37])) and out[0, 3] == (out[0, 2] if f else 0)
    assert out[0, 4:7].tolist() == [float(d2[0, 37] <= r) for r in (0, 2, 48387)]
    assert out[0, 12:15].tolist() == [float(d2[0, 37] <= r and f) for r in (0, 2, 48387)]
    assert (out[0, 7:12] == 0).all() and (out[0, 15:] == 0).all() and np.array_equal(out, mag)
    p[0, 5] = np.nan
    assert np.isnan(M.expectation(p, d2, free, (1,), 1)[0]).all()
