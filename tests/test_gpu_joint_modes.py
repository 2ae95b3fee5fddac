"""GPU: se_joint_modes_f32 (the K strongest local maxima of every softmaxed joint volume, with the mass and the first moments of
their windows) against tests/joint_modes_model.py, fed the SAME float32 prob / coord the kernel gets.  The definition has one right
answer, so everything is compared exactly: index, count and total as integers, all 8 slots of every record bit for bit.

Inputs: logits of one or two Gaussian bumps standardised to a std of 5-10 plus 0.01 noise, softmaxed by se_softargmax3d_f32 on the
device, as the forward does; planted peaks, ties and plateaus on top of them."""
import ctypes
import functools
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLD, synthetic_state_dict
from joint_modes_model import QNAN_BITS, joint_modes_model
from sceneego_amd import _lib, load_config, op, synth
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIDE = 2.0

# (rows, G) -> the (K, radius) pairs run there.  The kernel cuts a volume into tiles of 4 i-planes x (256 / ceil(G / 4)) j-rows:
CONFIGS = {
    (1, 8): [(k, r) for k in (1, 4, 16) for r in (0, 2, 3)],     # one row; 2 slabs of 4 planes, one band
    (15, 8): [(k, r) for k in (1, 4, 16) for r in (0, 2, 3)],
    (30, 16): [(k, r) for k in (1, 4, 16) for r in (0, 2, 3)],
    (15, 24): [(1, 0), (4, 2), (16, 3)],                         # 6 threads per row: idle lanes in every group of 8
    (120, 16): [(4, 2), (16, 3)],
    (15, 64): [(4, 2)],                                          # the batch-1 production shape: 16 slabs x 4 bands of 16 rows
    (4, 10): [(4, 2), (16, 3)],                                  # G % 4 = 2: scalar staging, a partial last quad, a ragged last slab
    (3, 6): [(16, 1)],
}
CASES = [(rows, G, K, radius) for (rows, G), v in CONFIGS.items() for K, radius in v]


# ------------------------------------------------------------------------------------------------------------------ inputs, launch
def make_logits(rows, G, seed):
    rng = np.random.default_rng(seed)
    ax = np.arange(G, dtype=np.float64)
    out = np.empty((rows, G, G, G), dtype=np.float32)
    for r in range(rows):
        v = np.zeros((G, G, G))
        for b in range(1 + r % 2):                      # odd rows: two bumps (the two-peaked volumes the feature is for)
            c = rng.uniform(0.5, G - 1.5, size=3)
            w = rng.uniform(1.0, 3.0)
            g = [np.exp(-(ax - c[a]) ** 2 / (2 * w * w)) for a in range(3)]
            v += rng.uniform(0.6, 1.0) * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
        v = (v - v.mean()) / v.std() * rng.uniform(5.0, 10.0)
        out[r] = (v + 0.01 * rng.standard_normal(v.shape)).astype(np.float32)
    return out.reshape(rows, G * G * G)


def launch(prob, coord, G, K, radius, min_prob=0.0):
    rows = prob.shape[0]
    modes = torch.empty((rows, K, 8), device=DEV, dtype=torch.float32)
    index = torch.empty((rows, K), device=DEV, dtype=torch.int32)
    count = torch.empty((rows,), device=DEV, dtype=torch.int32)
    total = torch.empty((rows,), device=DEV, dtype=torch.int32)
    _lib.joint_modes(prob, coord, modes, index, count, total, rows, G ** 3, G, K, radius, min_prob)
    torch.cuda.synchronize()
    return modes.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy(), total.cpu().numpy()


def assert_same(got, want, tag=""):
    gm, gi, gc, gt = got
    wm, wi, wc, wt = want
    assert gi.dtype == np.int32 and gc.dtype == np.int32 and gt.dtype == np.int32 and gm.dtype == np.float32
    assert np.array_equal(gt, wt), f"{tag}: total {gt} != {wt}"
    assert np.array_equal(gc, wc), f"{tag}: count {gc} != {wc}"
    assert np.array_equal(gi, wi), f"{tag}: index differs in rows {np.flatnonzero((gi != wi).any(axis=1))}"
    same = gm.view(np.int32) == wm.view(np.int32)
    assert same.all(), f"{tag}: modes differ bitwise at (row, mode, slot) {np.argwhere(~same)[:8].tolist()}"


@functools.lru_cache(maxsize=None)
def inputs(rows, G):
    """Softmaxed volumes on the device and on the host, computed once and shared (nothing below modifies them)."""
    N = G ** 3
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    logits = torch.from_numpy(make_logits(rows, G, seed=1000 * G + rows)).to(DEV)
    prob = torch.empty_like(logits)
    joints = torch.empty((rows, 3), device=DEV, dtype=torch.float32)
    _lib.softargmax3d(logits, coord, prob, joints, rows, N, 1)
    torch.cuda.synchronize()
    return {"prob": prob, "coord": coord, "joints": joints, "p": prob.cpu().numpy(), "c": coord.cpu().numpy()}


@functools.lru_cache(maxsize=None)
def case(rows, G, K, radius):
    k = inputs(rows, G)
    return {"got": launch(k["prob"], k["coord"], G, K, radius), "want": joint_modes_model(k["p"], k["c"], G, K, radius)}


def planted(rows, G, plant, K=4, radius=2, min_prob=0.0):
    """inputs(rows, G) with ``plant`` = [(row, flat index, value)] written over them: (prob on the device, kernel answer, model answer)."""
    k = inputs(rows, G)
    prob = k["prob"].clone()
    p = k["p"].copy()
    for row, n, v in plant:
        prob[row, n] = float(v)
        p[row, n] = np.float32(v)
    return prob, launch(prob, k["coord"], G, K, radius, min_prob), joint_modes_model(p, k["c"], G, K, radius, min_prob)


def above(p_row):
    """A float32 above every probability of the row: some rows are one-hot after the softmax, so it lies above 1."""
    v = np.float32(1.5)
    assert v > p_row.max()
    return v


def flat(G, i, j, k):
    return (i * G + j) * G + k


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("rows,G,K,radius", CASES)
def test_exact_against_the_model(rows, G, K, radius):
    c = case(rows, G, K, radius)
    assert_same(c["got"], c["want"], f"rows {rows} G {G} K {K} radius {radius}")
    total = c["want"][3]
    print(f"rows {rows} G {G} K {K} radius {radius}: total min {total.min()} median {int(np.median(total))} max {total.max()}")


def test_the_cases_exercise_the_cap_from_both_sides():
    more = less = 0
    for rows, G, K, radius in CASES:
        total = case(rows, G, K, radius)["want"][3]
        more += int((total > K).sum())
        less += int(((total >= 0) & (total < K)).sum())
    print(f"rows with total > K: {more}, rows with total < K: {less}")
    assert more > 0 and less > 0


def test_a_tie_across_every_cut():
    """48 rows at G = 16: row r holds, above everything else, an equal adjacent pair on planes r % 16 and r % 16 + 1 along axis
    r // 16 (a single peak on the last plane where the second would lie outside): wherever the kernel cuts the volume, on
    whichever axis, a tie straddles the cut."""
    rows, G = 48, 16
    k = inputs(rows, G)
    plant, lower = [], []
    for r in range(rows):
        axis, pl = r // 16, r % 16
        at = [5, 9, 6]
        at[axis] = pl
        v = above(k["p"][r])
        plant.append((r, flat(G, *at), v))
        lower.append(flat(G, *at))
        if pl + 1 < G:
            at[axis] = pl + 1
            plant.append((r, flat(G, *at), v))
    _, got, want = planted(rows, G, plant)
    assert np.array_equal(got[1][:, 0], np.array(lower, dtype=np.int32)), "mode 0 is not the lower index of the pair"
    assert np.array_equal(got[3], want[3])
    assert_same(got, want, "ties across cuts")


@pytest.mark.parametrize("radius", [2, 3])
def test_borders_clip_and_do_not_wrap(radius):
    rows, G = 15, 8
    N = G ** 3
    k = inputs(rows, G)
    #       corner       corner        corner       edge         edge         face         face         n = 0   n = N - 1 (next to row + 1's n = 0)
    at = [(0, 0, 7), (7, 0, 0), (0, 7, 0), (0, 3, 0), (7, 7, 4), (4, 0, 3), (2, 5, 7), (0, 0, 0), (7, 7, 7), (0, 0, 0)]
    plant = [(r + 1, flat(G, *a), above(k["p"][r + 1])) for r, a in enumerate(at)]
    _, got, want = planted(rows, G, plant, K=4, radius=radius)
    for (r, n, v) in plant:
        assert got[1][r, 0] == n and got[0][r, 0, 0] == v
    assert plant[8][1] == N - 1 and plant[9][1] == 0 and plant[9][0] == plant[8][0] + 1
    assert_same(got, want, f"borders radius {radius}")


def test_ties_and_plateaus():
    rows, G = 15, 8
    k = inputs(rows, G)
    v = [above(k["p"][r]) for r in range(rows)]
    cube = [flat(G, 3 + a, 4 + b, 2 + c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    ell = [flat(G, 2, 2, 2), flat(G, 2, 2, 3), flat(G, 2, 2, 4), flat(G, 2, 3, 4), flat(G, 2, 4, 4), flat(G, 3, 4, 4)]
    plant = [(0, flat(G, 3, 3, 3), v[0]), (0, flat(G, 3, 3, 4), v[0]),          # adjacent along k
             (1, flat(G, 3, 3, 3), v[1]), (1, flat(G, 4, 2, 2), v[1]),          # adjacent along a diagonal: the higher index has lower j, k
             (2, flat(G, 3, 3, 3), v[2]), (2, flat(G, 3, 3, 5), v[2]),          # two voxels apart: both
             (3, flat(G, 1, 6, 2), v[3]), (3, flat(G, 3, 6, 2), v[3])]          # two planes apart: both
    plant += [(4, n, v[4]) for n in cube] + [(5, n, v[5]) for n in ell]
    _, got, want = planted(rows, G, plant, K=4, radius=1)
    modes, index, count, total = got
    for r, first, second in ((0, flat(G, 3, 3, 3), None), (1, flat(G, 3, 3, 3), None), (2, flat(G, 3, 3, 3), flat(G, 3, 3, 5)),
                             (3, flat(G, 1, 6, 2), flat(G, 3, 6, 2)), (4, cube[0], None)):
        assert index[r, 0] == first and modes[r, 0, 0] == v[r]
        if second is None:
            assert count[r] < 2 or modes[r, 1, 0] < v[r], f"row {r}: the tie gave two modes"
        else:
            assert index[r, 1] == second and modes[r, 1, 0] == v[r]
    assert_same(got, want, "ties and plateaus")          # the L-shaped plateau included: whatever the model says


def test_min_prob_threshold_is_inclusive():
    rows, G, K = 15, 8, 16
    k = inputs(rows, G)
    base = case(rows, G, K, 2)["want"]
    row = int(np.argmax(base[2] >= 2))                   # a row with at least two modes
    assert base[2][row] >= 2
    p1 = base[0][row, 1, 0]                              # the probability of its second mode
    for min_prob, kept in ((p1, True), (np.nextafter(p1, np.float32(np.inf)), False)):
        got = launch(k["prob"], k["coord"], G, K, 2, min_prob=float(min_prob))
        want = joint_modes_model(k["p"], k["c"], G, K, 2, min_prob=min_prob)
        assert_same(got, want, f"min_prob {min_prob!r}")
        assert (base[1][row, 1] in got[1][row]) == kept
        assert got[3][row] <= base[3][row]


def test_min_prob_above_the_peak_gives_unfilled_records():
    rows, G, K = 15, 8, 4
    k = inputs(rows, G)
    got = launch(k["prob"], k["coord"], G, K, 2, min_prob=2.0)
    modes, index, count, total = got
    assert (count == 0).all() and (total == 0).all() and (index == -1).all()
    bits = modes.view(np.uint32)
    assert (bits[:, :, :5] == 0).all(), "slots 0..4 of an unfilled record must be +0 (no sign bit)"
    assert (bits[:, :, 5:] == QNAN_BITS).all()
    assert_same(got, joint_modes_model(k["p"], k["c"], G, K, 2, min_prob=2.0))


def test_all_zero_row():
    rows, G, K = 15, 8, 4
    k = inputs(rows, G)
    prob = k["prob"].clone()
    prob[6] = 0.0
    p = k["p"].copy()
    p[6] = 0.0
    got = launch(prob, k["coord"], G, K, 2)
    assert got[2][6] == 0 and got[3][6] == 0 and (got[1][6] == -1).all()
    assert_same(got, joint_modes_model(p, k["c"], G, K, 2))


@pytest.mark.parametrize("rows,G,K,radius", [(15, 8, 4, 2), (15, 24, 4, 2)])
def test_nan_poisons_its_own_row_only(rows, G, K, radius):
    k = inputs(rows, G)
    base = case(rows, G, K, radius)
    row = 7
    peak = int(base["want"][1][row, 0])
    N = G ** 3
    far = (peak + N // 2) % N                            # half a grid away from the strongest mode
    for at in (peak + 1 if peak + 1 < N else peak - 1, far, 0, N - 1):
        prob = k["prob"].clone()
        prob[row, at] = float("nan")
        modes, index, count, total = launch(prob, k["coord"], G, K, radius)
        assert np.isnan(modes[row]).all() and (index[row] == -1).all() and count[row] == -1 and total[row] == -1
        other = np.arange(rows) != row
        assert_same((modes[other], index[other], count[other], total[other]), tuple(a[other] for a in base["got"]), f"NaN at {at}")


@pytest.mark.parametrize("rows,G,K,radius", [(15, 64, 4, 2), (120, 16, 4, 2)])
def test_two_launches_bitwise_equal(rows, G, K, radius):
    k = inputs(rows, G)
    assert_same(launch(k["prob"], k["coord"], G, K, radius), case(rows, G, K, radius)["got"])


def test_bad_arguments_raise_and_do_not_launch():
    rows, G, K = 15, 8, 4
    N = G ** 3
    k = inputs(rows, G)
    prob, coord = k["prob"], k["coord"]
    SENT = -7.0
    modes = torch.full((rows, K, 8), SENT, device=DEV)
    index = torch.full((rows, K), -7, device=DEV, dtype=torch.int32)
    count = torch.full((rows,), -7, device=DEV, dtype=torch.int32)
    total = torch.full((rows,), -7, device=DEV, dtype=torch.int32)

    def untouched():
        torch.cuda.synchronize()
        return bool((modes == SENT).all() and (index == -7).all() and (count == -7).all() and (total == -7).all())

    def call(prob=prob, coord=coord, modes=modes, index=index, count=count, total=total, rows=rows, voxels=N, G=G, K=K, radius=2,
             min_prob=0.0, scratch=None):
        return lambda: _lib.joint_modes(prob, coord, modes, index, count, total, rows, voxels, G, K, radius, min_prob, scratch=scratch)

    wide = torch.zeros((rows, 2 * N), device=DEV)
    bad = {
        "cpu prob": call(prob=prob.cpu()), "cpu coord": call(coord=coord.cpu()), "cpu count": call(count=count.cpu()),
        "float64 prob": call(prob=prob.double()), "float32 index": call(index=index.float()), "int64 total": call(total=total.long()),
        "non-contiguous prob": call(prob=wide[:, ::2]), "non-contiguous coord": call(coord=coord.t().contiguous().t()),
        "short modes": call(modes=modes[:, :2].contiguous()), "short coord": call(coord=coord[:-4].contiguous()),
        "rows 0": call(rows=0), "rows 65536": call(rows=65536), "G 1": call(G=1, voxels=1),
        "voxels != G^3": call(voxels=N - 4), "G != cbrt voxels": call(G=G + 1),
        "voxels % 4": call(prob=torch.zeros((rows, 125), device=DEV), coord=torch.zeros((125, 3), device=DEV), voxels=125, G=5),
        "K 0": call(K=0), "K 17": call(K=17), "radius -1": call(radius=-1), "radius 4": call(radius=4),
        "min_prob < 0": call(min_prob=-1e-9), "min_prob NaN": call(min_prob=float("nan")),
        "short scratch": call(scratch=torch.zeros(16, device=DEV, dtype=torch.uint8)),
        "float32 scratch": call(scratch=torch.zeros(1 << 16, device=DEV)),
    }
    for name, fn in bad.items():
        with pytest.raises(_lib.HipExtensionError):
            fn()
        assert untouched(), f"{name}: something was launched"

    # the C entry point's own checks, behind the wrapper's
    lib = _lib.load()
    need = _lib.joint_modes_scratch_bytes(rows, G, K)
    assert need > 0 and need % 4 == 0
    ws = torch.zeros(need + 16, device=DEV, dtype=torch.uint8)
    P = _lib._ptr
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)      # noqa: E731

    def c(prob=P(prob), coord=P(coord), modes=P(modes), index=P(index), count=P(count), total=P(total), scratch=P(ws),
          scratch_bytes=need, rows=rows, voxels=N, G=G, K=K, radius=2, min_prob=0.0):
        return lib.se_joint_modes_f32(prob, coord, modes, index, count, total, scratch, scratch_bytes, rows, voxels, G, K, radius,
                                      min_prob, None)

    for name, kw in {"null prob": dict(prob=None), "null coord": dict(coord=None), "null modes": dict(modes=None),
                     "null index": dict(index=None), "null count": dict(count=None), "null total": dict(total=None),
                     "null scratch": dict(scratch=None), "rows 0": dict(rows=0), "rows -1": dict(rows=-1), "rows 65536": dict(rows=65536),
                     "G 1": dict(G=1, voxels=1), "G 0": dict(G=0, voxels=0), "voxels != G^3": dict(voxels=N + 4), "G + 1": dict(G=G + 1),
                     "voxels & 3": dict(G=5, voxels=125), "K 0": dict(K=0), "K 17": dict(K=17), "radius -1": dict(radius=-1),
                     "radius 4": dict(radius=4), "min_prob < 0": dict(min_prob=-1.0), "min_prob NaN": dict(min_prob=float("nan")),
                     "prob + 4 bytes": dict(prob=off(prob, 4)), "coord + 8 bytes": dict(coord=off(coord, 8)),
                     "scratch one byte short": dict(scratch_bytes=need - 1), "scratch 0 bytes": dict(scratch_bytes=0)}.items():
        assert c(**kw) == -1, name
        assert untouched(), f"{name}: something was launched"
    assert lib.se_joint_modes_scratch_bytes(0, G, K) == 0 and lib.se_joint_modes_scratch_bytes(-3, G, K) == 0
    assert _lib.joint_modes_scratch_bytes(15, 64, 4) == 15 * 16 * 4 * (2 + 2 * 4) * 4      # 16 slabs x 4 bands, 2 + 2K words each
    assert c() == 0                                           # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not untouched()


# ------------------------------------------------------------------------------------------------------------------ the op
def test_op_surface():
    B, J, G, K = 2, 15, 16, 4
    k = inputs(B * J, G)
    vol = k["prob"].view(B, J, G, G, G)
    coord_volumes = k["coord"].view(1, G, G, G, 3).expand(3, -1, -1, -1, -1)
    r = op.joint_modes(vol, coord_volumes, k=K, radius=2, min_rel=0.02)
    torch.cuda.synchronize()
    assert tuple(r) == op.MODES_KEYS == ("coord", "peak_coord", "peak_prob", "mass", "index", "count", "total", "valid")
    assert tuple(r["coord"].shape) == (B, J, K, 3) and tuple(r["peak_coord"].shape) == (B, J, K, 3)
    assert all(tuple(r[n].shape) == (B, J, K) for n in ("peak_prob", "mass", "index", "valid"))
    assert all(tuple(r[n].shape) == (B, J) for n in ("count", "total"))
    assert r["index"].dtype == r["count"].dtype == r["total"].dtype == torch.int32 and r["valid"].dtype == torch.bool
    assert all(r[n].dtype == torch.float32 for n in ("coord", "peak_coord", "peak_prob", "mass"))
    modes, index, count, total = case(B * J, G, K, 2)["got"]
    h = {n: r[n].cpu().numpy().reshape((B * J,) + tuple(r[n].shape[2:])) for n in r}
    assert np.array_equal(h["index"], index) and np.array_equal(h["count"], count) and np.array_equal(h["total"], total)
    assert np.array_equal(h["peak_prob"].view(np.int32), modes[..., 0].view(np.int32))
    assert np.array_equal(h["mass"].view(np.int32), modes[..., 1].view(np.int32))
    assert np.array_equal(h["peak_coord"].view(np.int32), modes[..., 5:].view(np.int32))
    filled = index >= 0
    assert not filled.all() and filled.any()
    with np.errstate(invalid="ignore", divide="ignore"):
        quotient = modes[..., 2:5] / modes[..., 1:2]                                   # float32 / float32
    assert quotient.dtype == np.float32
    assert np.array_equal(h["coord"][filled].view(np.int32), quotient[filled].view(np.int32))
    assert np.isnan(h["coord"][~filled]).all()
    want_valid = filled & (modes[..., 0] >= np.float32(0.02) * modes[:, :1, 0])
    assert np.array_equal(h["valid"], want_valid)
    assert h["valid"][:, 0].all()
    # radius 0: the window is the mode's own voxel, mass == peak_prob, and op.joint_modes returns the voxel's centre as the centroid
    # (fl(fl(p c) / p) would only add rounding to it): exact
    r0 = op.joint_modes(vol, coord_volumes, k=K, radius=0)
    torch.cuda.synchronize()
    v0 = r0["valid"].cpu().numpy()
    m0 = case(B * J, G, K, 0)["got"][0]
    assert np.array_equal(r0["mass"].cpu().numpy().reshape(B * J, K)[filled], m0[..., 0][filled])
    assert v0.any() and np.array_equal(r0["coord"].cpu().numpy()[v0].view(np.int32), r0["peak_coord"].cpu().numpy()[v0].view(np.int32))
    s = op.joint_statistics(vol, coord_volumes, k["joints"].view(B, J, 3))
    assert torch.equal(r["index"][..., 0], s["peak_index"])
    frames = op.joint_modes_to_numpy(r)
    assert len(frames) == B and frames[1]["coord"].shape == (J, K, 3) and frames[1]["index"].dtype == np.int32
    assert tuple(frames[0]) == op.MODES_KEYS
    with pytest.raises(_lib.HipExtensionError):
        op.joint_modes(vol, coord_volumes, k=17)
    with pytest.raises(_lib.HipExtensionError):
        op.joint_modes(vol[:, :, :, :, :8], coord_volumes)


# ------------------------------------------------------------------------------------------------------------------ the module
@pytest.fixture(scope="module")
def net64():
    net = VoxelNetwork_depth(load_config(), device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def demo_forward(net64):
    """The golden demo frame and its EXR depth through the network: (image, depth, joints, volumes)."""
    from sceneego_amd.preprocess import load_depth, normalize_u8, prepare_depth
    img = normalize_u8(np.load(os.path.join(GOLD, "demo", "img_001000_256_bgr_u8.npz"))["img"])[None].to(DEV)
    depth = prepare_depth(load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr")))[None].to(DEV)
    with torch.no_grad():
        kp, _, vols, _ = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)
    torch.cuda.synchronize()
    return img, depth, kp.clone(), vols.clone()


def _module_answer_as_kernel_outputs(r):
    """The dict of net.joint_modes at batch 1 -> (peak_prob, mass, peak_coord, index, count, total) as [15, ...] numpy arrays."""
    return tuple(r[n][0].cpu().numpy() for n in ("peak_prob", "mass", "peak_coord", "index", "count", "total"))


def test_module_on_the_golden_demo_frame(net64, demo_forward):
    _, _, kp, vols = demo_forward
    G, K, radius = net64.volume_size, 4, 2
    assert G == 64
    r = net64.joint_modes(vols, k=K, radius=radius)
    torch.cuda.synchronize()
    assert tuple(r) == op.MODES_KEYS and tuple(r["coord"].shape) == (1, 15, K, 3)
    c = net64.coord_volumes[0].reshape(-1, 3).float().cpu().numpy()
    modes, index, count, total = joint_modes_model(vols.reshape(15, -1).cpu().numpy(), c, G, K, radius)
    peak, mass, peak_coord, gi, gc, gt = _module_answer_as_kernel_outputs(r)
    print("demo frame: modes per joint", total.tolist())
    assert np.array_equal(gi, index) and np.array_equal(gc, count) and np.array_equal(gt, total)
    assert np.array_equal(peak.view(np.int32), modes[..., 0].view(np.int32))
    assert np.array_equal(mass.view(np.int32), modes[..., 1].view(np.int32))
    assert np.array_equal(peak_coord.view(np.int32), modes[..., 5:].view(np.int32))
    filled = index >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        quotient = modes[..., 2:5] / modes[..., 1:2]
    assert np.array_equal(r["coord"][0].cpu().numpy()[filled].view(np.int32), quotient[filled].view(np.int32))
    s = net64.joint_statistics(vols, kp)
    assert torch.equal(r["index"][..., 0], s["peak_index"])


def test_module_under_graph_replay_leaves_the_forward_alone(net64, demo_forward):
    img, depth, _, vols0 = demo_forward
    eager = net64.joint_modes(vols0)
    eager = {n: eager[n].clone() for n in ("index", "total")}
    net64.enable_graphs(True)
    try:
        with torch.no_grad():
            net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)     # captures
            plain = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)[0].clone()
            kp, _, vols, _ = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)
            r = net64.joint_modes(vols)                                    # before the next forward: the buffers are static
            index, valid = r["index"].clone(), r["valid"].clone()
            after = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)[0].clone()
        torch.cuda.synchronize()
    finally:
        net64.enable_graphs(False)
    assert torch.equal(after, plain), "joint_modes() disturbed the replayed forward"
    assert (index[..., 0] >= 0).all() and valid[..., 0].all()
    assert tuple(index.shape) == tuple(eager["index"].shape)


def test_relu_volumes_are_refused():
    cfg = load_config()
    cfg.model.volume_softmax = False
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    G = net.volume_size
    with pytest.raises(ValueError):
        net.joint_modes(torch.zeros((1, 15, G, G, G), device=DEV))


# ------------------------------------------------------------------------------------------------------------------ command lines
def _check_frame(fr, K):
    assert tuple(fr) == op.MODES_KEYS
    assert fr["coord"].shape == (15, K, 3) and fr["peak_coord"].shape == (15, K, 3)
    assert all(fr[n].shape == (15, K) for n in ("peak_prob", "mass", "index", "valid"))
    assert fr["count"].shape == (15,) and fr["total"].shape == (15,)
    assert fr["index"].dtype == np.int32 and fr["valid"].dtype == np.bool_ and fr["coord"].dtype == np.float32
    assert fr["valid"][:, 0].all() and (fr["count"] >= 1).all() and (fr["total"] >= fr["count"]).all()
    v = fr["valid"]
    assert np.isfinite(fr["coord"][v]).all() and (fr["mass"][v] > 0).all() and (fr["mass"][v] <= 1 + 1e-6).all()
    assert (fr["mass"][v] >= fr["peak_prob"][v]).all()


def test_demo_modes_flag(tmp_path, capsys):
    import demo
    import evaluate
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg"), img_dir)
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), depth_dir)
    common = ["--img_dir", str(img_dir), "--depth_dir", str(depth_dir), "--weights", "synthetic"]
    demo.main(common + ["--output_dir", str(tmp_path / "plain")])
    demo.main(common + ["--output_dir", str(tmp_path / "modes"), "--modes", "true", "--modes_k", "3"])
    capsys.readouterr()
    assert sorted(os.listdir(tmp_path / "plain")) == ["img_001000.jpg.pkl"]
    assert sorted(os.listdir(tmp_path / "modes")) == ["img_001000.jpg.modes.pkl", "img_001000.jpg.pkl"]
    assert (tmp_path / "plain" / "img_001000.jpg.pkl").read_bytes() == (tmp_path / "modes" / "img_001000.jpg.pkl").read_bytes(), \
        "<img>.pkl differs between a run with and a run without --modes"
    with open(tmp_path / "modes" / "img_001000.jpg.modes.pkl", "rb") as f:
        _check_frame(pickle.load(f), 3)
    # evaluate.py skips the .modes.pkl files among the predictions and reads them through --modes
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((1, 15, 3)), f)
    res = evaluate.main(["--pred_dir", str(tmp_path / "modes"), "--gt", str(tmp_path / "gt.pkl"), "--modes", str(tmp_path / "modes")])
    capsys.readouterr()
    assert res["frames"] == 1 and np.isfinite(res["best_of_k_mpjpe"]) and 0.0 <= res["best_not_first_share"] <= 1.0


def test_run_sequence_modes_and_track_output(tmp_path, capsys):
    import evaluate
    import run_sequence
    depths = [os.path.join(GOLD, "demo", n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 3, depths, estimated_depth_name="est_depth", seed=5)
    common = ["--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
    plain = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl")])
    both = run_sequence.main(common + ["--output", str(tmp_path / "both.pkl"), "--modes_output", str(tmp_path / "m" / "modes.pkl"),
                                       "--track_output", str(tmp_path / "t" / "tracked.pkl"), "--track_sigma", "0.2"])
    out = capsys.readouterr().out
    assert (tmp_path / "plain.pkl").read_bytes() == (tmp_path / "both.pkl").read_bytes()
    assert "modes" not in plain and "tracked" not in plain and len(both["modes"]) == 3 == len(both["tracked"])
    assert "tracked modes" in out.splitlines()[-1]
    with open(tmp_path / "m" / "modes.pkl", "rb") as f:
        frames = pickle.load(f)
    assert len(frames) == 3
    for fr, mem in zip(frames, both["modes"]):
        _check_frame(fr, 4)
        assert all(np.array_equal(fr[n], mem[n], equal_nan=True) for n in op.MODES_KEYS)
    with open(tmp_path / "t" / "tracked.pkl", "rb") as f:
        tracked = pickle.load(f)
    with open(tmp_path / "plain.pkl", "rb") as f:
        preds = pickle.load(f)
    assert type(tracked) is type(preds) and len(tracked) == len(preds) == 3
    for a, b in zip(tracked, preds):
        assert type(a) is type(b) and a.dtype == b.dtype == np.float32 and a.shape == b.shape == (15, 3) and np.isfinite(a).all()
    choice = both["track_choice"]
    assert choice.shape == (3, 15) and (choice >= 0).all() and (choice < 4).all()       # mode 0 is always valid: no fallback
    for t in range(3):
        assert np.array_equal(tracked[t], frames[t]["coord"][np.arange(15), choice[t]])
    # evaluate.py reads the tracked pickle as it reads a prediction directory, with the modes beside it
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((3, 15, 3)), f)
    res = evaluate.main(["--pred_dir", str(tmp_path / "t" / "tracked.pkl"), "--gt", str(tmp_path / "gt.pkl"),
                         "--modes", str(tmp_path / "m" / "modes.pkl")])
    assert res["frames"] == 3 and res["best_of_k_mpjpe"] <= res["mpjpe"] + 1e-12
    # the flags on two streams: the same kind of output (the joints themselves differ by the backbone's split-K atomics between any
    # two runs on several streams, sceneego_amd/pipeline.py, so the byte comparison above is the single-stream one)
    two = run_sequence.main(common + ["--streams", "2", "--output", str(tmp_path / "two.pkl"), "--modes_k", "2",
                                      "--modes_output", str(tmp_path / "two_modes.pkl"), "--track_output", str(tmp_path / "two_t.pkl")])
    capsys.readouterr()
    assert len(two["modes"]) == 3 == len(two["tracked"])
    for fr in two["modes"]:
        _check_frame(fr, 2)
    assert np.abs(np.stack(two["predictions"]) - np.stack(plain["predictions"])).max() <= 2e-5
    assert np.stack(two["tracked"]).shape == (3, 15, 3) and np.stack(two["tracked"]).dtype == np.float32
