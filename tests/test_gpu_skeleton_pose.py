"""GPU: the most probable pose (csrc/skeleton_pose.hip: se_skeleton_pose_f32, se_shell_maxcorr_f32, se_shell_argmax_i32) against its
float32 numpy model (tests/skeleton_pose_model.py), BIT FOR BIT: no tolerance, no case left out - the tie rule (greater value, then
lower index) makes every result defined.  Then its independence of how frames are batched, the fallback, bad arguments, the public
surface and the command line.

Inputs (tests/skeleton_prior_cases.py): a random pose with the case's bone lengths, one bump of logits per joint, odd joints with a
second static bump, 0.01 noise, softmaxed by se_softargmax3d_f32 on the device.
"""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD, synthetic_state_dict
from sceneego_amd import _lib, load_config, op, synth
from sceneego_amd.skeleton_pose import SkeletonPose
from sceneego_amd.skeleton_prior import KINEMATIC_PARENTS, shell_taps
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
from skeleton_pose_model import shell_max, shell_max_at, skeleton_pose_model
from skeleton_prior_cases import CHAIN3, SIDE, STAR5, lengths_for, make_logits, taps_for
from volume_viterbi_model import refine_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TREE = KINEMATIC_PARENTS
TREES = {"chain3": CHAIN3, "tree15": TREE, "star5": STAR5, "one": (0,)}

# frames, tree, G, R, floor: the cases of the sum-product test, and one that crosses the frame group
CASES = [
    (1, "chain3", 8, 3, 0.0),
    (2, "tree15", 8, 4, 1e-3),
    (1, "tree15", 6, 5, 1e-3),          # R = G - 1: every window clipped on both sides
    (3, "tree15", 10, 4, 1e-3),         # G % 4 = 2
    (2, "tree15", 16, 6, 0.0),
    (2, "tree15", 16, 6, 1e-3),
    (1, "star5", 8, 3, 1e-3),           # four children: the general product loop
    (1, "one", 8, 0, 0.0),
    (5, "chain3", 8, 3, 1e-3),          # five frames walk two groups inside one call
]


# ------------------------------------------------------------------------------------------------------------------ inputs, launch
def softmax_on_device(logits, coord):
    F, J, N = logits.shape
    x = torch.from_numpy(logits).to(DEV).reshape(F * J, N)
    prob = torch.empty_like(x)
    joints = torch.empty((F * J, 3), device=DEV, dtype=torch.float32)
    _lib.softargmax3d(x, coord, prob, joints, F * J, N, 1)
    torch.cuda.synchronize()
    return prob.view(F, J, N)


@functools.lru_cache(maxsize=None)
def case(frames, tree, G, R):
    """Softmaxed volumes [frames, J, N] on the device and on the host, the taps and the coordinates, computed once and shared (nothing
    below modifies them)."""
    parents = TREES[tree]
    N = G ** 3
    seed = 1000 * G + 10 * len(parents) + R
    lengths = lengths_for(parents, G, R, seed)
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    prob = softmax_on_device(make_logits(frames, parents, lengths, G, seed)[0], coord)
    taps = taps_for(lengths, G, R) if len(parents) > 1 else np.zeros((1, (2 * R + 1) ** 3), dtype=np.float32)
    return {"prob": prob, "coord": coord, "p": prob.cpu().numpy(), "c": coord.cpu().numpy(), "taps": taps, "parents": parents,
            "taps_dev": torch.from_numpy(taps).to(DEV), "lengths": lengths}


def launch(prob, taps, parents, G, R, floor):
    """One _lib-level call over all frames of ``prob`` [F, J, N]: host arrays (index, jumped, exponent, best_root, solved)."""
    F, J, N = prob.shape
    index = torch.full((F, J), -7, device=DEV, dtype=torch.int32)
    jumped = torch.full((F, J), -7, device=DEV, dtype=torch.int32)
    exponent = torch.full((F, J), -7, device=DEV, dtype=torch.int32)
    best_root = torch.full((F,), -7.0, device=DEV)
    solved = torch.full((F,), -7, device=DEV, dtype=torch.int32)
    _lib.skeleton_pose(prob.contiguous(), taps, parents, index, jumped, exponent, best_root, solved, F, N, G, R, floor)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (index, jumped, exponent, best_root, solved))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def equals_model(got, want):
    index, jumped, exponent, best_root, solved = got
    assert np.array_equal(solved, want["solved"].astype(np.int32))
    assert np.array_equal(index, want["index"]), (index.tolist(), want["index"].tolist())
    assert np.array_equal(jumped, want["jumped"].astype(np.int32))
    assert np.array_equal(exponent, want["exponent"])
    assert same_bits(best_root, want["best_root"])


# ------------------------------------------------------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("frames,tree,G,R,floor", CASES)
def test_against_the_model(frames, tree, G, R, floor):
    k = case(frames, tree, G, R)
    want = skeleton_pose_model(k["p"], k["taps"], k["parents"], G, floor)
    got = launch(k["prob"], k["taps_dev"], k["parents"], G, R, floor)
    print(f"frames {frames} {tree} G {G} R {R} floor {floor}: solved {got[4].tolist()}, jumps {int(got[1].sum())}, log score "
          f"{want['log_score'].round(3).tolist()}")
    assert want["solved"].all()
    equals_model(got, want)
    # the messages themselves, through the stand-alone entry point on the model's scaled scores: s_j in, keep * e3_j out
    J = len(k["parents"])
    if J > 1:
        keep = float(np.float32(1.0) - np.float32(floor))
        s = np.stack([want["s"][0][j] for j in range(1, J)])
        tap_row = torch.arange(1, J, device=DEV, dtype=torch.int32)
        out = torch.full((J - 1, G ** 3), float("nan"), device=DEV)
        _lib.shell_maxcorr(torch.from_numpy(s).to(DEV), k["taps_dev"], tap_row, out, J - 1, G, R, scale_mul=keep)
        step = out.cpu().numpy()
        assert same_bits(step, np.stack([np.float32(keep) * shell_max(want["s"][0][j], k["taps"][j], G, R)[0] for j in range(1, J)]))
        jump = np.float32(np.float32(floor) / np.float32(G ** 3)) * np.array([np.ldexp(want["M"][0, j], -int(want["exponent"][0, j]))
                                                                               for j in range(1, J)], dtype=np.float32)
        m = np.where(jump[:, None] > step, jump[:, None], step).astype(np.float32)
        assert same_bits(m, np.stack([want["m"][0][j] for j in range(1, J)]))


# ------------------------------------------------------------------------------------------------------------------ 2. every voxel
def shell_rows(G, seed):
    """[5, N] float32: random, uniform, random scaled into the subnormals (by 1e-38 in the planes i < G / 2: subnormal products; by
    1e-45 behind them: every product an exact zero), random with NaN cells, random under a tap row out of range."""
    N = G ** 3
    rng = np.random.default_rng(seed)
    a = rng.random((5, N), dtype=np.float32)
    a[1] = np.float32(1.0 / N)
    a[2] = a[2] * np.where(np.arange(N) // (G * G) < G // 2, np.float32(1e-38), np.float32(1e-45)).astype(np.float32)
    a[3, rng.choice(N, size=max(3, N // 50), replace=False)] = np.nan
    return a


@pytest.mark.parametrize("G,R", [(6, 5), (10, 4), (68, 3)])
def test_max_correlation_and_argument_at_every_voxel(G, R):
    """G = 68: two column tiles and the seam at k = 63 / 64."""
    N, h = G ** 3, SIDE / G
    taps = shell_taps([0.0, (R - 1.51) * h, min(1.6, R - 1.6) * h], 0.5 * h, h, R)
    a = shell_rows(G, 100 * G + R)
    rows = [1, 2, 1, 2, 7]                                               # 7: out of range
    scale = np.float32(0.999)
    a_dev, taps_dev = torch.from_numpy(a).to(DEV), torch.from_numpy(taps).to(DEV)
    tap_row = torch.tensor(rows, device=DEV, dtype=torch.int32)
    out = torch.full((5, N), -1.0, device=DEV)
    _lib.shell_maxcorr(a_dev, taps_dev, tap_row, out, 5, G, R, scale_mul=float(scale))
    query = torch.arange(N, device=DEV, dtype=torch.int32)
    out_tap = torch.full((5, N), -7, device=DEV, dtype=torch.int32)
    out_value = torch.full((5, N), -1.0, device=DEV)
    _lib.shell_argmax(a_dev, taps_dev, tap_row, query, out_tap, out_value, 5, G, R)
    torch.cuda.synchronize()
    out, out_tap, out_value = out.cpu().numpy(), out_tap.cpu().numpy(), out_value.cpu().numpy()
    assert np.isnan(out[4]).all() and np.isnan(out_value[4]).all() and (out_tap[4] == -1).all()
    for r in range(4):
        e3, arg = shell_max(a[r], taps[rows[r]], G, R)
        assert same_bits(out_value[r], e3), r
        assert same_bits(out[r], scale * e3), r
        assert np.array_equal(out_tap[r], arg), r
    e3, arg = shell_max(a[2], taps[rows[2]], G, R)
    assert (arg[e3 == 0] == -1).all() and ((e3 > 0) & (e3 < 2.0 ** -126)).any()                      # subnormals
    assert (e3 == 0).any() == (G - 1 - R >= G // 2)                      # ... and zeros, where a window fits behind plane G / 2
    assert not np.isnan(out[3]).any()                                    # a NaN cell never wins
    top = taps[rows[1]].max()                                            # the uniform row: the lowest of the tied taps
    inner = (np.arange(N) // (G * G) >= R) & (np.arange(N) // (G * G) < G - R) & (np.arange(N) // G % G >= R) \
        & (np.arange(N) // G % G < G - R) & (np.arange(N) % G >= R) & (np.arange(N) % G < G - R)
    assert (out_tap[1][inner] == int(np.flatnonzero(taps[rows[1]] == top)[0])).all()


# ------------------------------------------------------------------------------------------------------------------ 3. production shape
BONES = np.linspace(0.15, 0.45, 14)


def test_max_correlation_at_the_production_shape():
    """64^3, R = 18, one row per distinct shell of the bone lengths 0.15..0.45 m: values and arguments at a few hundred voxels - corners,
    edges, the row-tile seams j % 16 and the wave seams j % 4, both ends of the k row - against the model's direct maxima."""
    G, R, tau = 64, 18, 0.03
    N, h = G ** 3, SIDE / G
    lengths = np.concatenate([[0.0], BONES])
    assert int(np.ceil((0.45 + 3 * tau) / h)) == R
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    prob = softmax_on_device(make_logits(1, TREE, lengths, G, 6418)[0], coord)[0, 1:].contiguous()
    taps = shell_taps(lengths, tau, h, R)
    tap_row = torch.arange(1, 15, device=DEV, dtype=torch.int32)
    out = torch.full((14, N), float("nan"), device=DEV)
    _lib.shell_maxcorr(prob, torch.from_numpy(taps).to(DEV), tap_row, out, 14, G, R)
    rng = np.random.default_rng(3)
    ends = [0, 1, 3, 4, 15, 16, 17, 31, 32, 47, 48, 60, 62, 63]
    grid = [(i, j, k) for i in (0, 20, 63) for j in ends for k in (0, 1, 31, 62, 63)]
    voxels = np.unique(np.concatenate([[(i * G + j) * G + k for i, j, k in grid], rng.choice(N, size=120, replace=False)]))
    query = torch.from_numpy(voxels.astype(np.int32)).to(DEV)
    out_tap = torch.full((14, len(voxels)), -7, device=DEV, dtype=torch.int32)
    out_value = torch.full((14, len(voxels)), -1.0, device=DEV)
    _lib.shell_argmax(prob, torch.from_numpy(taps).to(DEV), tap_row, query, out_tap, out_value, 14, G, R)
    torch.cuda.synchronize()
    p, out, out_tap, out_value = prob.cpu().numpy(), out.cpu().numpy(), out_tap.cpu().numpy(), out_value.cpu().numpy()
    for r in range(14):
        e3, arg = shell_max_at(p[r], taps[r + 1], G, R, voxels)
        assert (e3 > 0).all()
        assert same_bits(out[r, voxels], e3) and same_bits(out_value[r], e3) and np.array_equal(out_tap[r], arg), r


# ------------------------------------------------------------------------------------------------------------------ 4. batching
def test_results_do_not_depend_on_how_frames_are_batched():
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    args = (k["taps_dev"], TREE, G, R, 1e-3)
    three = launch(k["prob"], *args)
    parts = [launch(k["prob"][:1], *args), launch(k["prob"][1:], *args)]
    for x in range(5):
        assert same_bits(np.concatenate([p[x] for p in parts]), three[x]), x
    assert all(same_bits(a, b) for a, b in zip(launch(k["prob"], *args), three)) and three[4].all()


# ------------------------------------------------------------------------------------------------------------------ 5. fallback
def test_fallback_and_nan_cells_equal_the_model():
    G, R = 10, 4
    N = G ** 3
    k = case(3, "tree15", G, R)
    prob = k["prob"].clone()
    prob[0, 9] = 0.0                                                     # a row of zeros: frame 0 falls back
    prob[2, 5, int(np.argmin(k["p"][2, 5]))] = float("nan")              # a single NaN cell: frame 2 stays solved
    p = prob.cpu().numpy()
    want = skeleton_pose_model(p, k["taps"], TREE, G, 1e-3)
    assert want["solved"].tolist() == [False, True, True] and want["index"][0, 9] == -1
    got = launch(prob, k["taps_dev"], TREE, G, R, 1e-3)
    equals_model(got, want)
    clean = launch(k["prob"], k["taps_dev"], TREE, G, R, 1e-3)
    assert all(same_bits(a[1:], b[1:]) for a, b in zip(got, clean))      # the NaN cell lies off the pose: nothing changes
    # floor 0: the root's volume is a compact box and joint 1's volume is zero wherever the root's shell reaches: M_0 = 0
    prob = k["prob"][:2].clone()
    box = torch.zeros((G, G, G), device=DEV)
    box[4:6, 4:6, 4:6] = 0.125
    prob[0, 0] = box.reshape(-1)
    reach = shell_max((box.reshape(N) > 0).float().cpu().numpy(), k["taps"][1], G, R)[0] > 0
    assert 0 < reach.sum() < N
    prob[0, 1][torch.from_numpy(reach).to(DEV)] = 0.0
    p = prob.cpu().numpy()
    want = skeleton_pose_model(p, k["taps"], TREE, G, 0.0)
    assert want["solved"].tolist() == [False, True] and want["M"][0, 0] == 0.0 and (want["index"][0] >= 0).all()
    equals_model(launch(prob, k["taps_dev"], TREE, G, R, 0.0), want)
    bridged = skeleton_pose_model(p, k["taps"], TREE, G, 1e-3)           # with the floor the edge jumps and the frame is solved
    assert bridged["solved"].all() and bridged["jumped"][0, 1]
    equals_model(launch(prob, k["taps_dev"], TREE, G, R, 1e-3), bridged)


# ------------------------------------------------------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments_raise_and_do_not_launch():
    G, R = 10, 4
    k = case(3, "tree15", G, R)
    N, J = G ** 3, 15
    prob = k["prob"][:2].contiguous()
    outs = {"index": torch.full((2, J), -7, device=DEV, dtype=torch.int32), "jumped": torch.full((2, J), -7, device=DEV, dtype=torch.int32),
            "exponent": torch.full((2, J), -7, device=DEV, dtype=torch.int32), "best_root": torch.full((2,), -7.0, device=DEV),
            "solved": torch.full((2,), -7, device=DEV, dtype=torch.int32)}

    def call(**kw):
        a = {"prob": prob, "taps": k["taps_dev"], "parents": TREE, **outs, "frames": 2, "voxels": N, "grid": G, "radius": R, "floor": 1e-3}
        a.update(kw)
        return _lib.skeleton_pose(**a)

    bad_tree = list(TREE)
    bad_tree[5] = 5
    for kw in ({"radius": 25}, {"radius": -1}, {"radius": G}, {"floor": -0.1}, {"floor": 1.1}, {"floor": float("nan")}, {"frames": 0},
               {"frames": 3}, {"grid": G + 1}, {"voxels": N + 1}, {"grid": 1, "voxels": 1, "radius": 0}, {"parents": bad_tree},
               {"parents": [1] + list(TREE[1:])}, {"parents": list(TREE) + [3]}, {"parents": [0] * 33}, {"parents": []}, {"parents": None},
               {"prob": prob.cpu()}, {"prob": prob.double()}, {"prob": prob[:, :, ::2]}, {"taps": k["taps_dev"][:-1]},
               {"taps": k["taps"]}, {"index": outs["index"].float()}, {"jumped": outs["jumped"][:1]}, {"exponent": None},
               {"best_root": torch.empty((3,), device=DEV)}, {"solved": torch.empty((2,), device=DEV)},
               {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        with pytest.raises(_lib.HipExtensionError):
            call(**kw)
    a = prob[0, :2].contiguous()
    tr, out = torch.ones(2, device=DEV, dtype=torch.int32), torch.full((2, N), -7.0, device=DEV)
    both = torch.empty((3, N), device=DEV)
    for kw in ({"radius": 25}, {"radius": G}, {"grid": G + 1}, {"rows": 3}, {"rows": 0}, {"out": a}, {"tap_row": tr.float()},
               {"a": both[:2], "out": both[1:]}, {"taps": k["taps_dev"].reshape(-1)},
               {"scratch": torch.empty(16, device=DEV, dtype=torch.uint8)}):
        b = {"a": a, "taps": k["taps_dev"], "tap_row": tr, "out": out, "rows": 2, "grid": G, "radius": R}
        b.update(kw)
        with pytest.raises(_lib.HipExtensionError):
            _lib.shell_maxcorr(**b)
    q = torch.zeros(4, device=DEV, dtype=torch.int32)
    ot, ov = torch.full((2, 4), -7, device=DEV, dtype=torch.int32), torch.full((2, 4), -7.0, device=DEV)
    for kw in ({"radius": 25}, {"grid": G + 1}, {"rows": 3}, {"query": q.float()}, {"query": q[:0]}, {"out_tap": ot[:1]}, {"out_value": ot},
               {"taps": k["taps_dev"].reshape(-1)}):
        b = {"a": a, "taps": k["taps_dev"], "tap_row": tr, "query": q, "out_tap": ot, "out_value": ov, "rows": 2, "grid": G, "radius": R}
        b.update(kw)
        with pytest.raises(_lib.HipExtensionError):
            _lib.shell_argmax(**b)
    # the C entry points refuse on their own what the wrappers check first
    import ctypes
    lib = _lib.load()
    ws = torch.empty(_lib.skeleton_pose_scratch_bytes(2, J, G, R), device=DEV, dtype=torch.uint8)
    P = _lib._ptr

    def raw(radius=R, floor=1e-3, frames=2, grid=G, voxels=N, scratch_bytes=ws.numel(), parents=TREE, index=outs["index"], scratch=ws, n=J):
        par = (ctypes.c_int * len(parents))(*parents)
        return lib.se_skeleton_pose_f32(P(prob), P(k["taps_dev"]), ctypes.cast(par, ctypes.c_void_p), P(index), P(outs["jumped"]),
                                        P(outs["exponent"]), P(outs["best_root"]), P(outs["solved"]),
                                        ctypes.c_void_p(scratch.data_ptr()) if scratch is not None else None, scratch_bytes, frames, n,
                                        voxels, grid, radius, floor, _lib._stream())
    assert raw(radius=25) == raw(radius=G) == raw(floor=2.0) == raw(floor=float("nan")) == raw(frames=0) == raw(voxels=N + 4) == -1
    assert raw(grid=129) == raw(scratch_bytes=ws.numel() - 1) == raw(index=None) == raw(parents=bad_tree) == raw(n=0) == raw(n=33) == -1
    assert raw(scratch=ws[1:], scratch_bytes=ws.numel() - 1) == -1               # misaligned
    assert lib.se_skeleton_pose_scratch_bytes(2, 33, G, R) == 0 and lib.se_skeleton_pose_scratch_bytes(2, J, G, G) == 0
    rs = torch.empty(_lib.shell_correlate_scratch_bytes(J, R), device=DEV, dtype=torch.uint8)

    def raw_m(radius=R, grid=G, rows=2, out_=out, scratch_bytes=rs.numel()):
        return lib.se_shell_maxcorr_f32(P(a), P(k["taps_dev"]), P(tr), P(out_), P(rs), scratch_bytes, rows, J, grid, radius, 1.0,
                                        _lib._stream())

    def raw_a(radius=R, grid=G, rows=2, queries=4, query=q):
        return lib.se_shell_argmax_i32(P(a), P(k["taps_dev"]), P(tr), P(query), P(ot), P(ov), rows, queries, J, grid, radius, _lib._stream())
    assert raw_m(radius=25) == raw_m(radius=G) == raw_m(grid=1) == raw_m(rows=0) == raw_m(out_=a) == raw_m(scratch_bytes=8) == -1
    assert raw_a(radius=25) == raw_a(radius=G) == raw_a(grid=1) == raw_a(rows=0) == raw_a(queries=0) == raw_a(query=None) == -1
    torch.cuda.synchronize()
    # nothing was launched: the pre-filled outputs are unchanged
    assert all((t == -7).all() for t in outs.values()) and (out == -7).all() and (ot == -7).all() and (ov == -7).all()
    # ... and the good calls write them
    call()
    assert raw() == 0 and raw_m() == 0 and raw_a() == 0
    torch.cuda.synchronize()
    assert (outs["solved"] == 1).all() and (out != -7).all() and (ot != -7).all()


# ------------------------------------------------------------------------------------------------------------------ 7. public surface
@pytest.fixture(scope="module")
def net64():
    net = VoxelNetwork_depth(load_config(), device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def two_forwards(net64):
    """Two B = 2 forwards: [(joints, volumes)] cloned."""
    out = []
    for seed in (31, 32):
        img, depth = synth.make_inputs(seed, 2, "floor")
        with torch.no_grad():
            kp, _, vols, _ = net64(img.to(DEV), net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth.to(DEV))
        out.append((kp.clone(), vols.clone()))
    torch.cuda.synchronize()
    return out


def test_module_pose_equals_the_library_call(net64, two_forwards):
    G, J = net64.volume_size, 15
    assert G == 64
    N = G ** 3
    sp = net64.skeleton_pose(BONES)
    assert isinstance(sp, SkeletonPose) and sp.tau == 0.03 and sp.floor == 1e-3 and sp.refine == 1 and sp.parents == TREE
    assert sp.radius == int(np.ceil((0.45 + 0.09) / (net64.cuboid_side / G))) <= 24
    res = [sp.solve(vols, joints=kp) for kp, vols in two_forwards]
    torch.cuda.synchronize()
    for r in res:
        assert tuple(r) == ("joints", "index", "coord", "jumped", "solved", "log_score", "bone_error", "shift", "bone_error_before")
        assert tuple(r["joints"].shape) == tuple(r["coord"].shape) == (2, J, 3) and tuple(r["index"].shape) == (2, J)
        assert r["jumped"].dtype == r["solved"].dtype == torch.bool and tuple(r["solved"].shape) == (2,) and tuple(r["jumped"].shape) == (2, J)
        assert r["log_score"].dtype == torch.float64 and tuple(r["log_score"].shape) == (2,) and r["index"].dtype == torch.int32
        assert tuple(r["bone_error"].shape) == tuple(r["bone_error_before"].shape) == (2, J - 1) and tuple(r["shift"].shape) == (2, J)
    coord = net64.coord_volumes[0].reshape(N, 3).float().contiguous().to(DEV)
    vols = torch.cat([v for _, v in two_forwards]).reshape(4, J, N)
    taps = shell_taps(np.concatenate([[0.0], BONES]), 0.03, net64.cuboid_side / G, sp.radius)
    index, jumped, exponent, best_root, solved = launch(vols, torch.from_numpy(taps).to(DEV), TREE, G, sp.radius, 1e-3)
    assert np.array_equal(torch.cat([r["index"] for r in res]).cpu().numpy(), index)
    assert np.array_equal(torch.cat([r["jumped"] for r in res]).cpu().numpy(), jumped != 0)
    assert np.array_equal(torch.cat([r["solved"] for r in res]).cpu().numpy(), solved != 0) and solved.all()
    want_score = np.log(best_root.astype(np.float64)) + np.log(2.0) * exponent.astype(np.float64).sum(axis=1)
    assert np.allclose(torch.cat([r["log_score"] for r in res]).cpu().numpy(), want_score, rtol=1e-14, atol=0)
    c = coord.cpu().numpy()
    joints = torch.cat([r["joints"] for r in res])
    assert same_bits(joints.cpu().numpy(), refine_model(vols.cpu().numpy(), c, index, G, 1))
    assert same_bits(torch.cat([r["coord"] for r in res]).cpu().numpy(), c[index])
    kp = torch.cat([k for k, _ in two_forwards])
    assert torch.equal(torch.cat([r["shift"] for r in res]), (joints - kp).norm(dim=-1))
    par = list(TREE[1:])
    lengths = torch.from_numpy(BONES.astype(np.float32)).to(DEV)
    assert torch.equal(torch.cat([r["bone_error"] for r in res]), ((joints[:, 1:] - joints[:, par]).norm(dim=-1) - lengths).abs())
    assert torch.equal(torch.cat([r["bone_error_before"] for r in res]), ((kp[:, 1:] - kp[:, par]).norm(dim=-1) - lengths).abs())
    before, after = torch.cat([r["bone_error_before"] for r in res]), torch.cat([r["bone_error"] for r in res])
    print(f"synthetic weights: solved {solved.tolist()}, {int(jumped.sum())} jumps in {jumped.size} joints, log score "
          f"{want_score.round(2).tolist()}, mean bone error {float(before.mean()):.4f} -> {float(after.mean()):.4f} m")
    # refine = 0 keeps the voxel centres
    centre = net64.skeleton_pose(BONES, refine=0).solve(two_forwards[0][1])
    assert torch.equal(centre["joints"], centre["coord"]) and torch.equal(centre["index"], res[0]["index"])
    frames = op.skeleton_pose_to_numpy(res[0])
    assert len(frames) == 2 and tuple(frames[0]) == op.POSE_KEYS + ("shift", "bone_error_before")
    assert frames[1]["joints"].shape == (J, 3) and frames[1]["solved"].dtype == np.bool_ and frames[1]["bone_error"].shape == (J - 1,)


# ------------------------------------------------------------------------------------------------------------------ 8. command line
def test_run_sequence_map_outputs(tmp_path, capsys):
    import evaluate
    import run_sequence
    from sceneego_amd.jpeg_device import JpegFile
    demo_exr = os.path.join(GOLD, "demo", "img_001000.jpg.exr")
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 5, [demo_exr], estimated_depth_name="est_depth", seed=5)
    cfg_path = tmp_path / "batch2.yaml"
    with open(os.path.join(os.path.dirname(GOLD), "..", "experiments", "sceneego", "test", "sceneego.yaml")) as f:
        text = f.read()
    assert text.count("  batch_size: 8\n") == 1
    cfg_path.write_text(text.replace("  batch_size: 8\n", "  batch_size: 2\n"))
    np.save(tmp_path / "bones.npy", BONES)
    common = ["--config", str(cfg_path), "--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth",
              "--weights", "synthetic"]
    res = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl"), "--map_output", str(tmp_path / "m" / "map.pkl"),
                                      "--map_info_output", str(tmp_path / "m" / "info.pkl"), "--bone_lengths", str(tmp_path / "bones.npy"),
                                      "--skeleton_output", str(tmp_path / "m" / "coupled.pkl")])
    out = capsys.readouterr().out
    last = out.splitlines()[-1]
    assert "most probable pose" in last and "mpjpe" in last and "coupled" in last and "mean bone error" in last
    with open(tmp_path / "m" / "map.pkl", "rb") as f:
        posed = pickle.load(f)
    with open(tmp_path / "m" / "info.pkl", "rb") as f:
        info = pickle.load(f)
    with open(tmp_path / "plain.pkl", "rb") as f:
        preds = pickle.load(f)
    assert type(posed) is type(preds) and len(posed) == len(preds) == len(info) == 5
    for a, b, fr in zip(posed, preds, info):
        assert type(a) is type(b) and a.dtype == b.dtype == np.float32 and a.shape == b.shape == (15, 3) and np.isfinite(a).all()
        assert tuple(fr) == op.POSE_KEYS + ("shift", "bone_error_before") and np.array_equal(fr["joints"], a)
        assert np.allclose(fr["shift"], np.linalg.norm(a.astype(np.float64) - b, axis=1), rtol=1e-5, atol=1e-7)
        assert fr["solved"] and np.isfinite(fr["log_score"]) and (fr["index"] >= 0).all()
    assert np.isfinite(res["map_mpjpe"]) and len(res["map"]) == 5 == len(res["map_info"]) and np.isfinite(res["coupled_mpjpe"])
    # evaluate.py reads the file as it reads --output's, with and without the bone lengths and a ground truth
    ev = evaluate.main(["--pred_dir", str(tmp_path / "m" / "map.pkl"), "--bones", str(tmp_path / "bones.npy")])
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(np.zeros((5, 15, 3)), f)
    both = evaluate.main(["--pred_dir", str(tmp_path / "m" / "map.pkl"), "--gt", str(tmp_path / "gt.pkl"), "--bones"])
    capsys.readouterr()
    assert ev["frames"] == 5 and ev["bones"]["std"].shape == (14,)
    assert np.isclose(ev["bones"]["mean_deviation"], np.mean([fr["bone_error"] for fr in info]), rtol=1e-4)
    assert np.isfinite(both["mpjpe"]) and "deviation" not in both["bones"]
    # driving SkeletonPose.solve by hand on the same volumes gives the same joints, bit for bit
    runner = run_sequence.SequenceRunner(load_config(str(cfg_path)), weights="synthetic")
    images, _, depths = run_sequence.frame_list(str(tmp_path / "seq"), "zseq", "est_depth")
    sp = runner.net.skeleton_pose(BONES, tau=0.03, floor=1e-3, refine=1)
    by_hand = []
    for i in range(0, 5, 2):
        img = runner._images([JpegFile(p) for p in images[i:i + 2]])
        depth = runner._depths(depths[i:i + 2])
        with torch.no_grad():
            kp, _, vol, _ = runner.net(img, runner.net.grid_coord_proj_batch, runner.net.coord_volumes, depth_map_batch=depth)
        by_hand.extend(sp.solve(vol, joints=kp)["joints"].cpu().numpy())
    assert len(by_hand) == 5 and all(same_bits(a, b) for a, b in zip(by_hand, posed))
