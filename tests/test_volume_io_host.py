"""CPU only: the float64 models of tests/volume_io_model.py agree with the oracle's restatement of the reference, and the cases of
tests/volume_io_cases.py can tell a subtly wrong kernel from a right one.  Nothing here runs a kernel: the discrimination checks are
conditions on the inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import volume_io_cases as C
import volume_io_model as M
from oracle import sceneego_oracle as O
from sceneego_amd import op, synth


# ------------------------------------------------------------------------------------------------------------------ models vs oracle
def test_voxelize_model_equals_oracle_at_real_size(oracle_constants):
    """The one heavy case: a 1024 x 1280 depth map, the calibrated rays, 64^3, side 2, through both forms."""
    c = oracle_constants(64)
    _, depth = synth.make_inputs(11, 1, "uniform")
    d = depth.numpy()
    d[0, 5, 7], d[0, 600, 640], d[0, 1000, 900] = 0.0, np.inf, 400.0
    tab = op.build_voxelizer_ray_table(c.ray, 1280, 1024)
    got = M.voxelize_model(d, tab, 1024, 128, 64, 2.0)
    assert np.array_equal(got[0], O.depth_to_voxel(d[0], c.ray, 64, 2).numpy() != 0)
    full_tab = np.ascontiguousarray(c.ray.reshape(1280, 1024, 3).transpose(1, 0, 2))
    got = M.voxelize_model(d, full_tab, (1024, 1280), 0, 64, 2.0)
    assert np.array_equal(got[0], O.depth_to_voxel_full(d[0], c.ray, 64, 2).numpy() != 0)


def test_voxelize_model_resize_indices_match_oracle_at_odd_sizes():
    for dst, src in ((24, 17), (24, 29), (40, 17), (40, 29), (40, 40), (24, 40)):
        img = np.arange(src * src, dtype=np.float32).reshape(src, src)
        want = O.resize_nearest(img, dst, dst)
        i = M.nearest_index(dst, src)
        assert np.array_equal(img[i][:, i], want)


def test_gather_model_agrees_with_float64_grid_sample():
    H, W, Cn, V = 9, 11, 4, 343
    img = torch.from_numpy(synth.normal(2, "vioh/img", (2, Cn, H, W)))
    g = torch.from_numpy(synth.uniform(3, "vioh/g", (1, V, 1, 2), -1.15, 1.15))
    idx, w = op.build_gather_table_generic(g.reshape(-1, 2), H, W)
    assert int((idx < 0).sum()) > 0 and int((idx >= 0).sum()) > 0
    feat = img.permute(0, 2, 3, 1).reshape(2, H * W, Cn).contiguous().numpy()
    got, mag = M.gather_model(feat, idx.numpy(), w.numpy())
    want = F.grid_sample(img.double(), g.double().expand(2, -1, -1, -1), align_corners=True).reshape(2, Cn, V).permute(0, 2, 1).numpy()
    # the table's weights are float32 products of float32 coordinates: ix = ((g + 1) / 2) * (W - 1) is off by <= 3 * 2^-24 * (W - 1),
    # a weight by twice that plus its own rounding, < 4e-6; four taps of |feat| <= max|feat| each
    assert float(np.abs(got - want).max()) <= 4 * float(np.abs(feat).max()) * 4e-6
    assert np.all(mag >= np.abs(got) - 1e-12)


@pytest.mark.parametrize("mode", [1, 0])
def test_softargmax_model_agrees_with_oracle_float64(mode):
    G = 8
    lg = synth.normal(5, "vioh/lg", (2, 3, G, G, G), 6.0)
    coord = C.sa_coord(G ** 3)
    want_kp, want_v = O.integrate(torch.from_numpy(lg), torch.from_numpy(coord).reshape(G, G, G, 3), softmax=bool(mode), accumulate64=True)
    m = M.softargmax_model(lg.reshape(6, -1), coord, mode)
    # the oracle returns its float64 values cast to float32: half a float32 step
    kp = want_kp.numpy().reshape(6, 3).astype(np.float64)
    assert np.all(np.abs(m["joints"] - kp) <= 2.0 ** -24 * np.abs(kp) + 1e-12)
    v = want_v.numpy().reshape(6, -1).astype(np.float64)
    assert np.all(np.abs(m["vol"] - v) <= 2.0 ** -24 * np.abs(v) + 1e-45)


def test_softargmax_model_non_finite_rows_as_torch():
    lg, nan_rows = C.sa_nan_rows()
    m = M.softargmax_model(lg, C.sa_coord(1000), 1)
    want = torch.softmax(torch.from_numpy(lg).double(), dim=1).numpy()
    assert np.array_equal(np.isnan(m["vol"]), np.isnan(want))
    ok = [r for r in range(15) if r not in nan_rows]
    assert np.isnan(m["vol"][list(nan_rows)]).all() and np.isnan(m["joints"][list(nan_rows)]).all()
    assert np.isfinite(m["vol"][ok]).all() and np.isfinite(m["joints"][ok]).all()
    assert np.allclose(m["vol"][ok], want[ok], rtol=1e-12, atol=0)
    assert (m["vol"][12, 0:4] == 0).all()


def test_intersection_model_is_one_float32_multiply():
    buf = synth.normal(1, "vioh/ib", (2, 5, 12))
    occ = synth.uniform(1, "vioh/io", (2, 5), -2.0, 2.0)
    got = M.intersection_model(buf, occ, 4)
    assert got.dtype == np.float32 and np.array_equal(got[..., :4], buf[..., :4]) and np.array_equal(got[..., 8:], buf[..., 8:])
    assert np.array_equal(got[..., 4:8], (buf[..., :4].astype(np.float64) * occ[..., None].astype(np.float64)).astype(np.float32))


def test_bf16_round_matches_torch():
    x = synth.normal(4, "vioh/bf", (4096,), 3.0)
    x[:4] = [1.0, 1.00390625, 1.01171875, -0.0]               # exact, tie to even (down), tie to even (up), signed zero
    assert np.array_equal(M.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


# ------------------------------------------------------------------------------------------------------------------ cases: shapes
def test_voxel_cases_cover_the_shapes():
    cs = [C.voxel_case(n) for n in C.VOXEL_CASES]
    assert {c["up"] for c in cs} == {24, 40} and all((c["up"] ** 2) % 256 for c in cs)
    assert {(c["dh"], c["dw"]) for c in cs} == {(17, 29), (40, 40)}
    assert {c["pad_x"] for c in cs} == {0, 8} and {c["G"] for c in cs} == {6, 8, 16} and {c["B"] for c in cs} == {1, 3}
    assert {c["side"] for c in cs} == {2.0, 2.4, 0.7}
    for c in cs + [C.voxel_full_case(n) for n in C.VOXEL_FULL_CASES]:
        d = c["depth"]
        assert d.dtype == np.float32 and c["ray"].dtype == np.float64
        assert (d == 0).any() and np.isinf(d).any() and (d == np.float32(50.0 * c["side"])).any()
        assert float(np.abs(np.linalg.norm(c["ray"], axis=-1) - 1).max()) < 1e-6      # unit up to the tie adjustment of one component
        occ = M.voxelize_model(d, c["ray"], c["up"], c["pad_x"], c["G"], c["side"])
        assert occ.any() and not occ.all()
        assert all(occ[b].sum() > 8 for b in range(c["B"]))


def test_voxel_tie_depths_sit_on_rounding_boundaries_of_all_axes_and_both_range_edges():
    """Per case: among the pixels' float64 voxel coordinates before rounding, some lie within one float32 step of k + 0.5 on every
    axis, at k = -1 and at k = G - 1 (just in and just out of range)."""
    for name in C.VOXEL_CASES:
        c = C.voxel_case(name)
        G, side, up = c["G"], c["side"], c["up"]
        d = c["depth"][:, M.nearest_index(up, c["dh"])][:, :, M.nearest_index(up, c["dw"])].astype(np.float64)
        seen = set()
        with np.errstate(all="ignore"):
            for a in range(3):
                p = c["ray"][None, :, :, a] * d
                q = ((p + (0.0 if a == 2 else side / 2)) * G) / side
                near = np.abs(q - (np.floor(q) + 0.5)) <= 2.0 ** -22 * np.maximum(np.abs(q), 1.0) * 4
                ks = np.floor(q[near & np.isfinite(q)])
                assert len(ks) >= 10, (name, a, len(ks))
                seen |= {int(k) for k in ks}
        assert -1 in seen and G - 1 in seen, (name, sorted(seen))


@pytest.mark.parametrize("side", [2.4, 0.7, 2.0])
def test_voxel_cases_tell_wrong_evaluations_from_the_right_one(side):
    """Each deliberately wrong float64 / float32 evaluation of ((p + side/2) * G) / side must give another occupied set than the right
    one on the cases of this side.  For side 2 (G / side an exact power of two) only float32 can differ."""
    names = [n for n in list(C.VOXEL_CASES) if C.VOXEL_CASES[n][6] == side]
    fulls = [n for n in C.VOXEL_FULL_CASES if C.VOXEL_FULL_CASES[n][4] == side]
    variants = ("float32",) if side == 2.0 else ("prescale", "divfirst", "float32")
    for v in variants:
        total = 0
        for c in [C.voxel_case(n) for n in names] + [C.voxel_full_case(n) for n in fulls]:
            right = M.voxelize_model(c["depth"], c["ray"], c["up"], c["pad_x"], c["G"], c["side"])
            wrong = M.voxelize_model(c["depth"], c["ray"], c["up"], c["pad_x"], c["G"], c["side"], variant=v)
            n = int((right != wrong).sum())
            print(f"side {side} G {c['G']} up {c['up']}: variant {v} differs in {n} voxels")
            total += n
        assert total >= 1, (side, v)


def test_gather_cases_cover_the_shapes():
    cl = C.GATHER_CL_CASES
    assert {c[2] for c in cl} == {4, 12, 32} and {c[5] for c in cl} == {0, 8} and all(c[4] > c[5] + c[2] for c in cl)
    assert {c[3] for c in cl} == {1, 257, 1000} and {c[1] for c in cl} == {1, 35} and {c[0] for c in cl} == {1, 3}
    assert any((c[3] * c[2] // 4) % 256 and 256 % (c[2] // 4) for c in cl)          # a workgroup ends inside a voxel
    pl = C.GATHER_PLANAR_CASES
    assert {c[2] for c in pl} == {16, 32, 64}
    spare = {3 * c[4] - c[2] for c in pl}
    assert 1 in spare and 2 in spare and any(s >= 3 for s in spare)
    assert {c[5] - c[2] for c in pl} == {0, 3}
    for voxels, texels in {(c[3], c[1]) for c in cl + pl}:
        idx, w = C.gather_table(voxels, texels)
        assert idx.min() >= -1 and idx.max() <= texels - 1 and idx.dtype == np.int32 and w.dtype == np.float32
        if voxels > 1:
            live = (idx >= 0).sum(axis=1)
            assert set(live.tolist()) == {0, 1, 2, 3, 4}
            assert ((idx == idx[:, :1]).all(axis=1) & (live == 4)).any()           # all taps on one texel
            assert (idx == 0).any() and (idx == texels - 1).any()
            assert (w == 0).any() and (w == 1).any() and (w < 0).any() and (w[idx < 0] != 0).any()


def test_intersection_cases_cover_the_shapes():
    assert {c[2] for c in C.INTERSECTION_CASES} == {4, 32}
    assert all(c[3] > 2 * c[2] for c in C.INTERSECTION_CASES)
    assert any((c[0] * c[1] * c[2] // 4) % 256 for c in C.INTERSECTION_CASES)


def test_softargmax_cases_cover_every_regime_and_chunk_geometry():
    assert {C.sa_splits(r) for r in C.SA_ROWS} == {256, 128, 64, 32}
    for lo, hi in ((29, 30), (59, 60), (119, 120)):
        assert C.sa_splits(lo) != C.sa_splits(hi)
    geo = {(r, n): (C.sa_chunk(r, n), C.sa_splits(r)) for r, n in C.SA_RANDOM_CASES}
    assert any(ch * s > n + ch for (r, n), (ch, s) in geo.items())                  # empty chunks
    assert any(n % ch for (r, n), (ch, s) in geo.items())                            # a ragged last chunk
    assert C.sa_chunk(*C.SA_BIG) == 2000 > 1024
    kinds = set()
    for rows, voxels in C.SA_SPIKE_CASES:
        lg, pos = C.sa_spike(rows, voxels)
        assert (lg.max(axis=1) == 80).all() and ((lg == 80).sum(axis=1) == 1).all() and np.sort(lg, axis=1)[:, -2].max() <= 0
        ch = C.sa_chunk(rows, voxels)
        for p in pos:
            kinds |= {("first", p % ch == 0), ("last", (p + 1) % ch == 0 or p == voxels - 1), ("mod4", p % 4), ("end", p == voxels - 1),
                      ("lastchunk", p == ((voxels + ch - 1) // ch - 1) * ch)}
    assert {("first", True), ("last", True), ("mod4", 0), ("mod4", 1), ("mod4", 2), ("mod4", 3), ("end", True), ("lastchunk", True)} <= kinds
    c = C.sa_coord(1000)
    assert len({tuple(np.round(c[:, a], 6)) for a in range(3)}) == 3
    for rows, voxels in C.SA_NEGINF_CASES:
        lg = C.sa_neginf(rows, voxels)
        assert np.isfinite(lg).any(axis=1).all() and np.isneginf(lg).any() and not np.isnan(lg).any()
        ch = C.sa_chunk(rows, voxels)
        whole = [np.isneginf(lg[r, k * ch:min((k + 1) * ch, voxels)]).all() for r in range(rows) for k in range((voxels + ch - 1) // ch)]
        assert any(whole) or rows < 2
        if rows >= 4:
            assert (np.isfinite(lg).sum(axis=1) == 1).any()
