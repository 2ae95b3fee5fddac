"""GPU: the scene-constrained joints.  se_scene_free_mask_u8 bit for bit against the float64 model of tests/scene_constraint_model.py
(every voxel compared); se_softargmax3d_masked_f32 against the same model fed the SAME float32 prob / coord and uint8 mask the kernel
gets: exact free peak (ties included), sums within the float32 summation bound, empty rows, NaN rows, run-to-run determinism, argument
checks; and the feature end to end (module method, demo.py, run_sequence.py).

Gate of the sums (derived, not measured; the constant of tests/test_gpu_joint_stats.py, whose reduction tree this kernel shares):
float32 summation of n terms in a tree of depth d has a relative error bound of d * 2^-24 of the sum of the magnitudes.  The longest
serial chain of a lane is voxels / 256 <= 1024 terms at these shapes, then log2(256) levels of the workgroup tree and 4 + 6 of the
fold: (1024 + 8 + 4) * 2^-24 ~= 6.2e-5, rounded up to 1e-4; the one rounding of each product p * c (2^-24) is far inside.  So
|slot - model| <= 1e-4 * sum |terms| (+ 1e-30 so that a row of zeros compares)."""
import functools
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import scene_constraint_model as M
from conftest import GOLD, synthetic_state_dict
from sceneego_amd import _lib, load_config, op, synth
from sceneego_amd.render import MAX_DEPTH
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIDE = 2.0
SUM_REL, SUM_ABS = 1e-4, 1e-30

#        rows, G     what it exercises (the chunk rule of se_sa_splits, as tests/test_gpu_joint_stats.py)
CASES = [(1, 8),     # 256 chunks of 4 voxels: half of them empty, skipped by position
         (15, 8),    # many rows, tiny chunks
         (30, 16), (60, 16), (120, 16),   # every value of se_sa_splits (128, 64, 32)
         (15, 24),   # chunk 56, not a divisor of 13 824: ragged last chunk, empty tail chunks
         (15, 64)]   # the batch-1 production shape: 256 chunks of 1024


# ------------------------------------------------------------------------------------------------------------------ the mask
FRAME_H, FRAME_W = 32, 40
MARGIN = 2.0 / 64          # the module's default at the shipped grid; a power of two, so d + margin == rng can be planted exactly


def mask_inputs(voxels, dh, dw, B, seed):
    """Synthetic sight table and depth maps with every special value planted at a depth pixel that some voxel looks at.  Returns
    (depth [B,dh,dw] float32, pix int32, rng float32, planted: list of (frame, voxel, expected free))."""
    g = np.random.default_rng(seed)
    pix = g.integers(0, FRAME_H * FRAME_W, size=voxels).astype(np.int32)
    pix[g.random(voxels) < 0.1] = -1
    pix[:2] = (0, FRAME_H * FRAME_W - 1)                                       # the first and the last pixel of the frame
    rng = g.uniform(0.5, 3.5, size=voxels).astype(np.float32)
    depth = g.uniform(0.2, 3.8, size=(B, dh, dw)).astype(np.float32)           # about half of the seen voxels end up blocked
    used, planted = set(), []

    def plant(b, n, value, expect):
        if pix[n] < 0:
            return False
        y, x = divmod(int(pix[n]), FRAME_W)
        at = (b, (y * dh) // FRAME_H, (x * dw) // FRAME_W)
        if at in used:                                                         # a depth pixel carries one planted value
            return False
        used.add(at)
        depth[at] = value
        planted.append((b, n, expect))
        return True

    m = np.float32(MARGIN)
    # rng - margin is exact in float32 here (margin = 2^-5 is a multiple of rng's ulp for rng >= 0.5), so (double)d + margin == rng
    specials = [(lambda r: np.float32(0.0), 1), (lambda r: np.float32(-1.5), 1), (lambda r: np.float32(np.nan), 1),
                (lambda r: np.float32(np.inf), 1), (lambda r: np.float32(MAX_DEPTH * 1.5), 1),
                (lambda r: np.float32(0.25), 0),                               # a plain surface well in front: blocked
                (lambda r: r - m, 1),                                          # (double)d + margin == rng: equal counts as free
                (lambda r: np.nextafter(r - m, np.float32(-np.inf)), 0),       # one ulp nearer: blocked
                (lambda r: np.nextafter(r - m, np.float32(np.inf)), 1)]        # one ulp farther: free
    order = iter(g.permutation(voxels))
    for b in range(B):
        for make, expect in specials * 3:
            n = int(next(order))
            while not plant(b, n, make(rng[n]), expect):
                n = int(next(order))
    return depth, pix, rng, planted


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dh,dw", [(16, 20), (32, 40)])
@pytest.mark.parametrize("voxels", [512, 4096])
def test_free_mask_equals_the_model_bit_for_bit(voxels, dh, dw, B):
    depth, pix, rng, planted = mask_inputs(voxels, dh, dw, B, seed=voxels + 7 * dh + B)
    want = M.free_mask(depth, pix, rng, FRAME_H, FRAME_W, MARGIN, MAX_DEPTH)
    # the model itself does what the definitions say at the planted values (equality included: (double)d + margin == rng is free)
    for b, n, expect in planted:
        assert want[b, n] == expect, (b, n, depth.dtype, expect)
    eq = [(b, n) for b, n, _ in planted
          if float(depth[b, (pix[n] // FRAME_W * dh) // FRAME_H, (pix[n] % FRAME_W * dw) // FRAME_W]) + MARGIN == float(rng[n])]
    assert len(eq) >= 3 * B, "the exact-equality cases were not planted"
    got = op.scene_free_mask(torch.from_numpy(depth).to(DEV), torch.from_numpy(pix).to(DEV), torch.from_numpy(rng).to(DEV),
                             FRAME_H, FRAME_W, MARGIN, MAX_DEPTH)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, voxels)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} voxels differ"
    assert (got[:, pix < 0] == 1).all()                                        # no pixel: free whatever the depth
    assert 0.2 < got[:, pix >= 0].mean() < 0.8, "the case does not exercise both outcomes"


def test_free_mask_other_margins():
    depth, pix, rng, _ = mask_inputs(4096, 16, 20, 2, seed=5)
    d, p, r = torch.from_numpy(depth).to(DEV), torch.from_numpy(pix).to(DEV), torch.from_numpy(rng).to(DEV)
    for margin, max_depth in ((0.03, MAX_DEPTH), (0.0, MAX_DEPTH), (-0.5, MAX_DEPTH), (MARGIN, 2.0)):
        got = op.scene_free_mask(d, p, r, FRAME_H, FRAME_W, margin, max_depth).cpu().numpy()
        assert np.array_equal(got, M.free_mask(depth, pix, rng, FRAME_H, FRAME_W, margin, max_depth)), (margin, max_depth)


def test_free_mask_bad_arguments_raise_and_do_not_launch():
    depth, pix, rng, _ = mask_inputs(512, 16, 20, 1, seed=3)
    d, p, r = torch.from_numpy(depth).to(DEV), torch.from_numpy(pix).to(DEV), torch.from_numpy(rng).to(DEV)
    free = torch.full((1, 512), 7, device=DEV, dtype=torch.uint8)
    odd = torch.full((1, 516), 7, device=DEV, dtype=torch.uint8)
    bad = {
        "cpu depth": lambda: _lib.scene_free_mask(d.cpu(), p, r, free, FRAME_H, FRAME_W, MARGIN, MAX_DEPTH),
        "cpu pix": lambda: _lib.scene_free_mask(d, p.cpu(), r, free, FRAME_H, FRAME_W, MARGIN, MAX_DEPTH),
        "float64 depth": lambda: _lib.scene_free_mask(d.double(), p, r, free, FRAME_H, FRAME_W, MARGIN, MAX_DEPTH),
        "int64 pix": lambda: _lib.scene_free_mask(d, p.long(), r, free, FRAME_H, FRAME_W, MARGIN, MAX_DEPTH),
        "short rng": lambda: _lib.scene_free_mask(d, p, r[:-4].contiguous(), free, FRAME_H, FRAME_W, MARGIN, MAX_DEPTH),
        "bool free": lambda: _lib.scene_free_mask(d, p, r, free.bool(), FRAME_H, FRAME_W, MARGIN, MAX_DEPTH),
        "non-contiguous depth": lambda: _lib.scene_free_mask(d.transpose(1, 2), p, r, free, FRAME_H, FRAME_W, MARGIN, MAX_DEPTH),
        "voxels % 4": lambda: _lib.scene_free_mask(d, p[:510].contiguous(), r[:510].contiguous(), free[:, :510].contiguous(), FRAME_H,
                                                   FRAME_W, MARGIN, MAX_DEPTH),
        "misaligned free": lambda: _lib.scene_free_mask(d, p, r, odd.view(-1)[1:513].view(1, 512), FRAME_H, FRAME_W, MARGIN, MAX_DEPTH),
        "NaN margin": lambda: _lib.scene_free_mask(d, p, r, free, FRAME_H, FRAME_W, float("nan"), MAX_DEPTH),
        "max_depth 0": lambda: _lib.scene_free_mask(d, p, r, free, FRAME_H, FRAME_W, MARGIN, 0.0),
        "height 0": lambda: _lib.scene_free_mask(d, p, r, free, 0, FRAME_W, MARGIN, MAX_DEPTH),
    }
    for name, call in bad.items():
        with pytest.raises(_lib.HipExtensionError):
            call()
        torch.cuda.synchronize()
        assert (free == 7).all() and (odd == 7).all(), f"{name}: something was launched"
    lib, q = _lib.load(), _lib._ptr
    assert lib.se_scene_free_mask_u8(q(d), q(p), q(r), None, 1, 16, 20, FRAME_H, FRAME_W, 512, MARGIN, MAX_DEPTH, None) == -1
    assert lib.se_scene_free_mask_u8(q(d), q(p), q(r), q(free), 0, 16, 20, FRAME_H, FRAME_W, 512, MARGIN, MAX_DEPTH, None) == -1
    assert lib.se_scene_free_mask_u8(q(d), q(p), q(r), q(free), 1, 16, 20, FRAME_H, FRAME_W, 510, MARGIN, MAX_DEPTH, None) == -1
    torch.cuda.synchronize()
    assert (free == 7).all()


# ------------------------------------------------------------------------------------------------------------------ the reduction
def make_logits(rows, G, seed):
    """One or two Gaussian bumps (width 1-3 voxels) standardised to a std of 5-10 plus small noise, as tests/test_gpu_joint_stats.py."""
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


def launch(prob, coord, free, rpf):
    rows, N = prob.shape
    out = torch.empty((rows, 8), device=DEV, dtype=torch.float32)
    idx = torch.empty((rows,), device=DEV, dtype=torch.int32)
    _lib.softargmax3d_masked(prob, coord, free, out, idx, rows, rpf, N)
    torch.cuda.synchronize()
    return out.cpu().numpy(), idx.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(rows, G):
    """Inputs on the device, the kernel's answer and the model's, computed once and shared (nothing below modifies them)."""
    N = G ** 3
    rpf = 15 if rows % 15 == 0 else 1
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    logits = torch.from_numpy(make_logits(rows, G, seed=1000 * G + rows)).to(DEV)
    prob = torch.empty_like(logits)
    joints = torch.empty((rows, 3), device=DEV, dtype=torch.float32)
    _lib.softargmax3d(logits, coord, prob, joints, rows, N, 1)
    g = np.random.default_rng(77 * G + rows)
    f = (g.random((rows // rpf, N)) < 0.5).astype(np.uint8)
    f[f == 1] = g.choice(np.array([1, 1, 1, 255, 2], dtype=np.uint8), size=int((f == 1).sum()))     # any non-zero byte is free
    free = torch.from_numpy(f).to(DEV)
    out, idx = launch(prob, coord, free, rpf)
    p, c, j = prob.cpu().numpy(), coord.cpu().numpy(), joints.cpu().numpy()
    want, want_idx, mag = M.masked_reduction(p, c, f, rpf)
    return {"prob": prob, "coord": coord, "free": free, "joints": joints, "rpf": rpf, "p": p, "c": c, "j": j, "f": f, "out": out, "idx": idx,
            "want": want, "want_idx": want_idx, "mag": mag}


def check_sums(out, want, mag, tag):
    bound = SUM_REL * mag + SUM_ABS
    ratio = float((np.abs(out[:, :4].astype(np.float64) - want[:, :4]) / bound).max())
    print(f"{tag}: sum error / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{tag}: the masked sums miss the float32 summation bound by {ratio:.3f}x"


def check_peak(out, idx, want, want_idx, c):
    assert idx.dtype == np.int32 and np.array_equal(idx, want_idx)
    assert np.array_equal(out[:, 4].view(np.int32), want[:, 4].astype(np.float32).view(np.int32))
    assert np.array_equal(out[:, 5:8].view(np.int32), c[idx].view(np.int32))


@pytest.mark.parametrize("rows,G", CASES)
def test_free_peak_exact(rows, G):
    k = case(rows, G)
    assert (k["idx"] >= 0).all() and (k["f"][np.arange(rows) // k["rpf"], k["idx"]] != 0).all()       # the peak voxel is free
    check_peak(k["out"], k["idx"], k["want"], k["want_idx"], k["c"])


@pytest.mark.parametrize("rows,G", CASES)
def test_sums_within_float32_summation_bound(rows, G):
    k = case(rows, G)
    assert np.isfinite(k["out"]).all()
    check_sums(k["out"], k["want"], k["mag"], f"rows {rows} G {G}")


# (rows, G, row, a, b): a < b; the positions of tests/test_gpu_joint_stats.py (chunk 56 at G = 24, lane t holds voxels 4t .. 4t + 3)
TIES = [(15, 24, 7, 2 * 56 + 1, 100 * 56 + 50),      # different chunks; lower index in the lower lane of both passes
        (15, 24, 7, 2 * 56 + 50, 100 * 56 + 1),      # lower index in the HIGHER lane of pass 1
        (15, 24, 3, 10 * 56 + 3, 70 * 56 + 3),       # lower index in the HIGHER lane of pass 2 (chunk 10 -> lane 10, chunk 70 -> lane 6)
        (15, 24, 0, 5 * 56 + 8, 5 * 56 + 10),        # one lane's own four voxels
        (1, 8, 0, 5, 301),                           # chunks of 4 voxels
        (15, 64, 14, 5 * 1024 + 12, 5 * 1024 + 800)]  # one chunk, waves 0 and 3 of the workgroup


@pytest.mark.parametrize("rows,G,row,a,b", TIES)
def test_ties(rows, G, row, a, b):
    k = case(rows, G)
    v = np.float32(0.5 * (float(k["p"][row].max()) + 1.0))             # above every probability of the row
    assert v > k["p"][row].max()
    prob = k["prob"].clone()
    prob[row, a] = float(v)
    prob[row, b] = float(v)
    other = np.arange(rows) != row
    #            a free, b free: the lowest index      a blocked: the free one      b blocked
    for fa, fb, winner in ((1, 1, a), (0, 1, b), (1, 0, a)):
        free = k["free"].clone()
        free[row // k["rpf"], a], free[row // k["rpf"], b] = fa, fb
        out, idx = launch(prob, k["coord"], free, k["rpf"])
        assert idx[row] == winner and out[row, 4] == v, (fa, fb, idx[row], out[row, 4])
        assert np.array_equal(out[row, 5:8].view(np.int32), k["c"][winner].view(np.int32))
        want, want_idx, _ = M.masked_reduction(prob[row:row + 1].cpu().numpy(), k["c"], free[row // k["rpf"]][None].cpu().numpy(), 1)
        assert want_idx[0] == winner and np.float32(want[0, 4]) == v
        if k["rpf"] == 1:
            continue
        # rows of other frames see their own, untouched mask
        far = other & (np.arange(rows) // k["rpf"] != row // k["rpf"])
        assert np.array_equal(out[far].view(np.int32), k["out"][far].view(np.int32)) and np.array_equal(idx[far], k["idx"][far])


@pytest.mark.parametrize("rows,G", [(15, 8), (15, 24), (30, 16)])
def test_all_free_mask_is_the_soft_argmax(rows, G):
    k = case(rows, G)
    N = G ** 3
    free = torch.ones((rows // k["rpf"], N), device=DEV, dtype=torch.uint8)
    out, idx = launch(k["prob"], k["coord"], free, k["rpf"])
    want, want_idx, mag = M.masked_reduction(k["p"], k["c"], np.ones((rows // k["rpf"], N), dtype=np.uint8), k["rpf"])
    check_sums(out, want, mag, f"all free rows {rows} G {G}")
    check_peak(out, idx, want, want_idx, k["c"])
    assert np.array_equal(idx, k["p"].argmax(axis=1).astype(np.int32))
    # free_mass against 1: the model's own sum is 1 up to the float32 rounding of the softmax (same bound); then the bound of the kernel
    assert np.abs(out[:, 0].astype(np.float64) - 1.0).max() <= 2 * SUM_REL
    # the quotient (float32, as the wrapper takes it) against the soft-argmax joints: both are float32 sums of the same terms, each
    # within SUM_REL * sum p |c| of the exact value, and the division by a mass within SUM_REL of 1 moves it by SUM_REL |joint| more
    quot = out[:, 1:4] / out[:, 0:1]
    bound = 2 * SUM_REL * mag[:, 1:4] + 2 * SUM_REL * np.abs(k["j"]) + 1e-7
    ratio = float((np.abs(quot.astype(np.float64) - k["j"]) / bound).max())
    print(f"all free rows {rows} G {G}: |quotient - soft-argmax joint| / bound = {ratio:.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("rows,G", [(15, 8), (15, 24)])
def test_all_blocked_mask_gives_empty_rows(rows, G):
    k = case(rows, G)
    free = torch.zeros((rows // k["rpf"], G ** 3), device=DEV, dtype=torch.uint8)
    out, idx = launch(k["prob"], k["coord"], free, k["rpf"])
    assert np.array_equal(out[:, :5], np.zeros((rows, 5), dtype=np.float32)) and not np.signbit(out[:, :5]).any()
    assert np.isnan(out[:, 5:8]).all() and (idx == -1).all()


def test_one_blocked_frame_among_free_ones():
    rows, G = 30, 16
    k = case(rows, G)
    free = k["free"].clone()
    free[1] = 0
    out, idx = launch(k["prob"], k["coord"], free, 15)
    assert np.array_equal(out[:15].view(np.int32), k["out"][:15].view(np.int32)) and np.array_equal(idx[:15], k["idx"][:15])
    assert (out[15:, :5] == 0).all() and np.isnan(out[15:, 5:8]).all() and (idx[15:] == -1).all()


@pytest.mark.parametrize("rows,G,row,at,blocked", [(15, 8, 7, 300, True), (15, 24, 14, 100 * 56 + 9, False), (15, 24, 0, 0, True)])
def test_nan_row_poisons_only_itself(rows, G, row, at, blocked):
    k = case(rows, G)
    prob = k["prob"].clone()
    prob[row, at] = float("nan")
    free = k["free"].clone()
    free[0, at] = 0 if blocked else 1                  # a NaN under a blocked voxel poisons the row too
    out, idx = launch(prob, k["coord"], free, k["rpf"])
    assert np.isnan(out[row]).all() and idx[row] == -1
    other = np.arange(rows) != row
    want, want_idx, mag = M.masked_reduction(prob.cpu().numpy(), k["c"], free.cpu().numpy(), k["rpf"])
    assert np.isnan(want[row]).all() and want_idx[row] == -1
    check_sums(out[other], want[other], mag[other], "NaN row: the others")
    check_peak(out[other], idx[other], want[other], want_idx[other], k["c"])
    if not (free.cpu().numpy() != k["f"]).any():       # the mask byte was already what the case wanted: the other rows are bitwise the same
        assert np.array_equal(out[other].view(np.int32), k["out"][other].view(np.int32))


@pytest.mark.parametrize("rows,G", [(15, 64), (120, 16), (15, 24)])
def test_two_launches_bitwise_equal(rows, G):
    k = case(rows, G)
    out, idx = launch(k["prob"], k["coord"], k["free"], k["rpf"])
    assert np.array_equal(out.view(np.int32), k["out"].view(np.int32)) and np.array_equal(idx, k["idx"])


def test_reduction_bad_arguments_raise_and_do_not_launch():
    rows, G = 15, 8
    N = G ** 3
    k = case(rows, G)
    SENT = -7.0
    out = torch.full((rows, 8), SENT, device=DEV)
    idx = torch.full((rows,), -7, device=DEV, dtype=torch.int32)
    prob, coord, free = k["prob"], k["coord"], k["free"]
    wide = torch.zeros((rows, 2 * N), device=DEV)
    odd = torch.ones((N + 4,), device=DEV, dtype=torch.uint8)
    call = _lib.softargmax3d_masked
    bad = {
        "cpu prob": lambda: call(prob.cpu(), coord, free, out, idx, rows, 15, N),
        "cpu free": lambda: call(prob, coord, free.cpu(), out, idx, rows, 15, N),
        "float64 prob": lambda: call(prob.double(), coord, free, out, idx, rows, 15, N),
        "bool free": lambda: call(prob, coord, free.bool(), out, idx, rows, 15, N),
        "float32 peak_index": lambda: call(prob, coord, free, out, idx.float(), rows, 15, N),
        "non-contiguous prob": lambda: call(wide[:, ::2], coord, free, out, idx, rows, 15, N),
        "non-contiguous coord": lambda: call(prob, coord.t().contiguous().t(), free, out, idx, rows, 15, N),
        "voxels % 4": lambda: call(torch.zeros((rows, 125), device=DEV), torch.zeros((125, 3), device=DEV),
                                   torch.ones((1, 125), device=DEV, dtype=torch.uint8), out, idx, rows, 15, 125),
        "rows % rows_per_frame": lambda: call(prob, coord, free, out, idx, rows, 4, N),
        "rows_per_frame 0": lambda: call(prob, coord, free, out, idx, rows, 0, N),
        "free frames": lambda: call(prob, coord, free, out, idx, rows, 5, N),                  # 3 frames of mask needed, 1 given
        "coord voxels": lambda: call(prob, coord[:-4].contiguous(), free, out, idx, rows, 15, N),
        "out slots": lambda: call(prob, coord, free, torch.full((rows, 12), SENT, device=DEV), idx, rows, 15, N),
        "short scratch": lambda: call(prob, coord, free, out, idx, rows, 15, N, scratch=torch.zeros(8, device=DEV)),
        "misaligned free": lambda: call(prob, coord, odd[1:N + 1].view(1, N), out, idx, rows, 15, N),
        "rows 0": lambda: call(prob, coord, free, out, idx, 0, 15, N),
        "rows 65536": lambda: call(prob, coord, free, out, idx, 65536, 1, N),
    }
    for name, fn in bad.items():
        with pytest.raises(_lib.HipExtensionError):
            fn()
        torch.cuda.synchronize()
        assert (out == SENT).all() and (idx == -7).all(), f"{name}: something was launched"
    # the C entry point's own checks, behind the wrapper's
    lib = _lib.load()
    ws = torch.zeros(_lib.softargmax3d_masked_scratch_elems(rows), device=DEV)
    q = _lib._ptr
    f = lib.se_softargmax3d_masked_f32
    assert f(q(prob), q(coord), q(free), q(out), q(idx), q(ws), rows, 15, 125, None) == -1
    assert f(q(prob), q(coord), q(free), q(out), q(idx), q(ws), 0, 15, N, None) == -1
    assert f(q(prob), q(coord), q(free), q(out), q(idx), q(ws), 65536, 1, N, None) == -1
    assert f(q(prob), q(coord), q(free), q(out), q(idx), q(ws), rows, 4, N, None) == -1
    assert f(q(prob), q(coord), q(free), q(out), q(idx), q(ws), rows, 15, 0, None) == -1
    assert f(q(prob), None, q(free), q(out), q(idx), q(ws), rows, 15, N, None) == -1
    assert f(q(prob), q(coord), None, q(out), q(idx), q(ws), rows, 15, N, None) == -1
    assert f(q(prob), q(coord), q(free), q(out), None, q(ws), rows, 15, N, None) == -1
    assert f(q(prob[0, 1:]), q(coord), q(free), q(out), q(idx), q(ws), rows, 15, N, None) == -1          # prob + 4 bytes
    assert f(q(prob), q(coord), q(odd[1:]), q(out), q(idx), q(ws), rows, 15, N, None) == -1               # free + 1 byte
    assert lib.se_softargmax3d_masked_scratch_elems(0) == 0 and lib.se_softargmax3d_masked_scratch_elems(15) == 15 * 256 * 8
    torch.cuda.synchronize()
    assert (out == SENT).all() and (idx == -7).all()


def test_op_surface():
    B, J, G = 2, 15, 16
    k = case(B * J, G)
    vol = k["prob"].view(B, J, G, G, G)
    coord_volumes = k["coord"].view(1, G, G, G, 3).expand(3, -1, -1, -1, -1)
    free = k["free"].clone().view(B, G, G, G)
    free[1] = 0                                                        # frame 1 cannot be constrained
    joints = k["joints"].view(B, J, 3)
    r = op.constrained_joints(vol, coord_volumes, free, joints)
    torch.cuda.synchronize()
    assert set(r) == set(op.CONSTRAINT_KEYS)
    assert tuple(r["joints"].shape) == (B, J, 3) == tuple(r["free_peak_coord"].shape)
    assert all(tuple(r[n].shape) == (B, J) for n in ("constrained", "free_mass", "moved", "free_peak_prob", "free_peak_index"))
    assert r["constrained"].dtype == torch.bool and r["free_peak_index"].dtype == torch.int32
    con = r["constrained"].cpu().numpy()
    assert con[0].all() and not con[1].any()
    out = k["out"].reshape(B, J, 8)
    assert np.array_equal(r["joints"][0].cpu().numpy(), out[0, :, 1:4] / out[0, :, 0:1])                 # the float32 quotient
    assert np.array_equal(r["joints"][1].cpu().numpy(), k["j"].reshape(B, J, 3)[1])                      # the input joints, exactly
    assert (r["moved"][1] == 0).all() and (r["moved"][0] >= 0).all() and (r["free_mass"][1] == 0).all()
    d = (r["joints"] - joints).double().cpu().numpy()
    assert np.allclose(r["moved"].cpu().numpy(), np.sqrt((d * d).sum(axis=-1)), rtol=1e-5, atol=0)
    frames = op.scene_constraint_to_numpy(r)
    assert len(frames) == B and set(frames[0]) == set(op.CONSTRAINT_KEYS) and frames[1]["joints"].shape == (J, 3)
    # without the unconstrained joints there is nothing to fall back on
    r2 = op.constrained_joints(vol, coord_volumes, free)
    assert torch.equal(r2["joints"][0], r["joints"][0]) and torch.isnan(r2["joints"][1]).all() and torch.isnan(r2["moved"]).all()


# ------------------------------------------------------------------------------------------------------------------ the module
@pytest.fixture(scope="module")
def net64():
    net = VoxelNetwork_depth(load_config(), device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def demo_forward(net64):
    """The golden demo frame and its EXR depth through the network: (depth, joints, volumes), the volumes' float64 model inputs."""
    from sceneego_amd.preprocess import load_depth, normalize_u8, prepare_depth
    img = normalize_u8(np.load(os.path.join(GOLD, "demo", "img_001000_256_bgr_u8.npz"))["img"])[None].to(DEV)
    depth = prepare_depth(load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr")))[None].to(DEV)
    with torch.no_grad():
        kp, _, vols, _ = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)
    torch.cuda.synchronize()
    return depth, kp.clone(), vols.clone()


def test_module_on_the_golden_demo_frame(net64, demo_forward):
    depth, kp, vols = demo_forward
    G = net64.volume_size
    r = net64.constrain_to_scene(vols, kp, depth)
    torch.cuda.synchronize()
    assert set(r) == set(op.CONSTRAINT_KEYS) | {"free"}
    assert tuple(r["free"].shape) == (1, G, G, G) and r["free"].dtype == torch.uint8
    assert tuple(r["joints"].shape) == (1, 15, 3) and r["joints"].dtype == torch.float32
    mass = r["free_mass"].cpu().numpy()
    print("free_mass", mass.tolist(), "moved", r["moved"].cpu().numpy().tolist(), "free share", float(r["free"].float().mean()))
    assert ((mass >= 0) & (mass <= 1)).all()
    con = r["constrained"].cpu().numpy()
    assert np.array_equal(r["joints"].cpu().numpy()[~con], kp.cpu().numpy()[~con])
    assert np.array_equal(con, mass > 0)
    idx = r["free_peak_index"].cpu().numpy().reshape(-1)
    free = r["free"].cpu().numpy().reshape(1, -1)
    assert (free[0][idx[idx >= 0]] == 1).all()
    # the mask is the model's, bit for bit, at the full grid and frame; the reduction the model's within the bound
    pix, rng = op.build_sight_table(net64.grid_coord_proj, net64.coord_volume, net64.image_height, net64.image_width)
    want_free = M.free_mask(depth.float().cpu().numpy(), pix.numpy(), rng.numpy(), net64.image_height, net64.image_width,
                            net64.cuboid_side / G, MAX_DEPTH)
    assert np.array_equal(free, want_free)
    assert 0 < free.mean() < 1, "the demo frame's depth map blocks nothing or everything"
    c = net64.coord_volumes[0].reshape(-1, 3).float().cpu().numpy()
    want, want_idx, mag = M.masked_reduction(vols.reshape(15, -1).cpu().numpy(), c, want_free, 15)
    assert np.array_equal(idx, want_idx)
    got = np.concatenate([mass.reshape(15, 1), (r["joints"] * r["free_mass"][..., None]).cpu().numpy().reshape(15, 3)], axis=1)
    # slots 1..3 are rebuilt here as joint * mass: two more float32 roundings (2^-23 of the value) beside the summation bound
    bound = SUM_REL * mag + 2.0 ** -22 * np.abs(want[:, :4]) + SUM_ABS
    ratio = float((np.abs(got.astype(np.float64) - want[:, :4]) / bound)[con.reshape(-1)].max(initial=0.0))
    print(f"module: sum error / bound = {ratio:.3e}")
    assert ratio <= 1.0
    # a margin of its own is honoured: nothing lies a whole cuboid behind a surface
    assert (net64.constrain_to_scene(vols, kp, depth, margin=10.0)["free"] == 1).all()


def test_module_all_zero_depth_returns_the_soft_argmax(net64, demo_forward):
    depth, kp, vols = demo_forward
    r = net64.constrain_to_scene(vols, kp, torch.zeros_like(depth))
    torch.cuda.synchronize()
    assert (r["free"] == 1).all() and r["constrained"].all()
    c = net64.coord_volumes[0].reshape(-1, 3).float().cpu().numpy()
    p = vols.reshape(15, -1).cpu().numpy()
    mag = np.abs(p.astype(np.float64)) @ np.abs(c.astype(np.float64))
    j = kp.cpu().numpy().reshape(15, 3)
    assert np.abs(r["free_mass"].cpu().numpy().astype(np.float64) - 1.0).max() <= 2 * SUM_REL
    bound = 2 * SUM_REL * mag + 2 * SUM_REL * np.abs(j) + 1e-7              # as test_all_free_mask_is_the_soft_argmax
    ratio = float((np.abs(r["joints"].cpu().numpy().reshape(15, 3).astype(np.float64) - j) / bound).max())
    print(f"zero depth: |constrained - soft-argmax joint| / bound = {ratio:.3e}, moved {float(r['moved'].max()):.3e} m")
    assert ratio <= 1.0


def test_module_under_graph_replay_leaves_the_forward_alone(net64, demo_forward):
    from sceneego_amd.preprocess import normalize_u8
    depth, kp0, vols0 = demo_forward
    eager = net64.constrain_to_scene(vols0, kp0, depth)
    eager = {n: eager[n].clone() for n in ("free", "free_peak_index")}
    img = normalize_u8(np.load(os.path.join(GOLD, "demo", "img_001000_256_bgr_u8.npz"))["img"])[None].to(DEV)
    net64.enable_graphs(True)
    try:
        with torch.no_grad():
            net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)     # captures
            plain = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)[0].clone()
            kp, _, vols, _ = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)
            r = net64.constrain_to_scene(vols, kp, depth)                  # before the next forward: the buffers are static
            free, index = r["free"].clone(), r["free_peak_index"].clone()
            after = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)[0].clone()
        torch.cuda.synchronize()
    finally:
        net64.enable_graphs(False)
    assert torch.equal(after, plain), "constrain_to_scene() disturbed the replayed forward"
    assert torch.equal(free, eager["free"])                                # the mask depends on the depth map alone
    assert (index >= 0).all()


def test_relu_volumes_are_refused():
    cfg = load_config()
    cfg.model.volume_softmax = False
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    G = net.volume_size
    with pytest.raises(ValueError):
        net.constrain_to_scene(torch.zeros((1, 15, G, G, G), device=DEV), torch.zeros((1, 15, 3), device=DEV),
                               torch.zeros((1, 8, 8), device=DEV))


# ------------------------------------------------------------------------------------------------------------------ command lines
def _check_frame(fr, with_joints):
    keys = set(op.CONSTRAINT_KEYS) - (set() if with_joints else {"joints"})
    assert set(fr) == keys
    for key in keys:
        want = (15, 3) if key in ("joints", "free_peak_coord") else (15,)
        assert isinstance(fr[key], np.ndarray) and fr[key].shape == want, key
    assert fr["constrained"].dtype == np.bool_ and fr["free_peak_index"].dtype == np.int32
    assert ((fr["free_mass"] >= 0) & (fr["free_mass"] <= 1)).all() and (fr["moved"] >= 0).all()


def test_demo_constrained_dir(tmp_path, capsys):
    import demo
    import evaluate
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg"), img_dir)
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), depth_dir)
    common = ["--img_dir", str(img_dir), "--depth_dir", str(depth_dir), "--weights", "synthetic"]
    demo.main(common + ["--output_dir", str(tmp_path / "plain")])
    demo.main(common + ["--output_dir", str(tmp_path / "out"), "--constrained_dir", str(tmp_path / "con")])
    capsys.readouterr()
    assert sorted(os.listdir(tmp_path / "plain")) == ["img_001000.jpg.pkl"] == sorted(os.listdir(tmp_path / "out"))
    assert (tmp_path / "plain" / "img_001000.jpg.pkl").read_bytes() == (tmp_path / "out" / "img_001000.jpg.pkl").read_bytes()
    assert sorted(os.listdir(tmp_path / "con")) == ["img_001000.jpg.constraint.pkl", "img_001000.jpg.pkl"]
    with open(tmp_path / "con" / "img_001000.jpg.pkl", "rb") as f:
        joints = pickle.load(f)
    with open(tmp_path / "con" / "img_001000.jpg.constraint.pkl", "rb") as f:
        fr = pickle.load(f)
    with open(tmp_path / "plain" / "img_001000.jpg.pkl", "rb") as f:
        before = pickle.load(f)
    assert isinstance(joints, np.ndarray) and joints.dtype == np.float32 and joints.shape == (15, 3) and np.isfinite(joints).all()
    _check_frame(fr, with_joints=False)
    assert np.array_equal(joints[~fr["constrained"]], before[~fr["constrained"]])
    d = (joints - before).astype(np.float64)
    assert np.allclose(fr["moved"], np.sqrt((d * d).sum(axis=1)), rtol=1e-4, atol=1e-7)
    # evaluate.py reads the constrained directory as it reads any prediction directory
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((1, 15, 3)), f)
    res = evaluate.main(["--pred_dir", str(tmp_path / "con"), "--gt", str(tmp_path / "gt.pkl")])
    capsys.readouterr()
    assert res["frames"] == 1


def test_run_sequence_constrain_output(tmp_path, capsys):
    import run_sequence
    from sceneego_amd import metrics
    depths = [os.path.join(GOLD, "demo", n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 3, depths, estimated_depth_name="est_depth", seed=5)
    common = ["--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
    plain = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl")])
    assert "scene check:" not in capsys.readouterr().out
    both = run_sequence.main(common + ["--output", str(tmp_path / "both.pkl"), "--scene_output", str(tmp_path / "scene.pkl"),
                                       "--constrain_output", str(tmp_path / "con" / "c.pkl")])
    out = capsys.readouterr().out
    assert (tmp_path / "plain.pkl").read_bytes() == (tmp_path / "both.pkl").read_bytes()
    assert "constraint" not in plain and len(both["constraint"]) == 3 == len(both["scene"]) == len(both["scene_constrained"])
    with open(tmp_path / "con" / "c.pkl", "rb") as f:
        frames = pickle.load(f)
    assert len(frames) == 3
    for fr, mem, pred in zip(frames, both["constraint"], both["predictions"]):
        _check_frame(fr, with_joints=True)
        assert all(np.array_equal(fr[n], mem[n], equal_nan=True) for n in op.CONSTRAINT_KEYS)
        assert np.array_equal(fr["joints"][~fr["constrained"]], pred[~fr["constrained"]])
    with open(tmp_path / "scene.pkl", "rb") as f:
        scene = pickle.load(f)
    lines = out.splitlines()
    assert lines[-2] == metrics.format_scene_summary(metrics.scene_summary(scene))
    assert lines[-1] == "constrained joints: " + metrics.format_scene_summary(metrics.scene_summary(both["scene_constrained"]))
    # the flag alone, on two streams: the same constraint dicts, no scene lines
    alone = run_sequence.main(common + ["--streams", "2", "--constrain_output", str(tmp_path / "alone.pkl")])
    assert "scene check:" not in capsys.readouterr().out and "scene" not in alone and len(alone["constraint"]) == 3
    for fr in alone["constraint"]:
        _check_frame(fr, with_joints=True)
