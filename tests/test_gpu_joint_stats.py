"""GPU: se_joint_stats_f32 (per-joint covariance about the soft-argmax joint, entropy and peak of the softmaxed volumes) against a
float64 numpy model of its definitions, fed the SAME float32 prob / coord / joints the kernel gets; ties, NaN rows, closed forms,
run-to-run determinism, argument checks of the _lib wrapper, and the feature end to end (module method, graph replay, demo.py,
run_sequence.py).

Inputs: logits of one or two Gaussian bumps (width 1-3 voxels) standardised to a std of 5-10 plus small noise, turned into
(volumes, joints) by se_softargmax3d_f32 on the device, as the forward does.

Gates (derived, not measured): float32 summation of n terms in a tree of depth d has a relative error bound of (d)·2^-24 of the sum of
the magnitudes.  The longest serial chain of a lane is voxels/256 <= 1024 terms at these shapes, then log2(256) levels of the
workgroup tree and 4 + 6 of the fold, so (1024 + 8 + 4)·2^-24 ~= 6.2e-5, rounded up to 1e-4.  For c_ab the sum of magnitudes is
sum p|d_a||d_b| <= sqrt(c_aa c_bb) (Cauchy-Schwarz), hence |dc_ab| <= 1e-4·sqrt(c_aa·c_bb) + 1e-12 m^2; the entropy's terms are all
non-negative: |dH| <= 1e-4·H + 1e-6 nats (logf's ulp included)."""
import functools
import math
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import GOLD, synthetic_state_dict
from sceneego_amd import _lib, load_config, op, synth
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIDE = 2.0

#        rows, G     what it exercises
CASES = [(1, 8),     # 256 chunks of 4 voxels: half of them empty, skipped by position
         (15, 8),    # many rows, tiny chunks
         (30, 16), (60, 16), (120, 16),   # every value of se_sa_splits (128, 64, 32)
         (15, 24),   # chunk 56, not a divisor of 13 824: ragged last chunk, empty tail chunks
         (15, 64)]   # the batch-1 production shape: 256 chunks of 1024
COV_REL, COV_ABS = 1e-4, 1e-12
ENT_REL, ENT_ABS = 1e-4, 1e-6


# ------------------------------------------------------------------------------------------------------------------ model, inputs
def model(prob, coord, joints):
    """float64 numpy model of include/sceneego_hip.h's definitions on the float32 arrays the kernel reads."""
    rows = prob.shape[0]
    c = coord.astype(np.float64)
    cov = np.zeros((rows, 6))
    ent = np.zeros(rows)
    for r in range(rows):
        p = prob[r].astype(np.float64)
        d = c - joints[r].astype(np.float64)[None]
        m = (d * p[:, None]).T @ d
        cov[r] = [m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]]
        nz = p > 0
        ent[r] = -(p[nz] * np.log(p[nz])).sum()
    return cov, ent


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


def launch(prob, coord, joints):
    rows, N = prob.shape
    stats = torch.empty((rows, 12), device=DEV, dtype=torch.float32)
    idx = torch.empty((rows,), device=DEV, dtype=torch.int32)
    _lib.joint_stats(prob, coord, joints, stats, idx, rows, N)
    torch.cuda.synchronize()
    return stats.cpu().numpy(), idx.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(rows, G):
    """Inputs on the device, the kernel's answer and the model's, computed once and shared (nothing below modifies them)."""
    N = G ** 3
    coord = op.build_coord_volume(G, SIDE).reshape(N, 3).contiguous().to(DEV)
    logits = torch.from_numpy(make_logits(rows, G, seed=1000 * G + rows)).to(DEV)
    prob = torch.empty_like(logits)
    joints = torch.empty((rows, 3), device=DEV, dtype=torch.float32)
    _lib.softargmax3d(logits, coord, prob, joints, rows, N, 1)
    stats, idx = launch(prob, coord, joints)
    p, c, j = prob.cpu().numpy(), coord.cpu().numpy(), joints.cpu().numpy()
    cov, ent = model(p, c, j)
    return {"prob": prob, "coord": coord, "joints": joints, "p": p, "c": c, "j": j, "stats": stats, "idx": idx, "cov": cov, "ent": ent}


def check_cov(stats, cov, tag):
    diag = {0: (0, 0), 1: (1, 1), 2: (2, 2), 3: (0, 1), 4: (0, 2), 5: (1, 2)}
    worst = 0.0
    for k, (a, b) in diag.items():
        bound = COV_REL * np.sqrt(cov[:, a] * cov[:, b]) + COV_ABS
        ratio = float((np.abs(stats[:, k].astype(np.float64) - cov[:, k]) / bound).max())
        worst = max(worst, ratio)
    print(f"{tag}: covariance error / bound = {worst:.3e}")
    assert worst <= 1.0, f"{tag}: covariance misses the float32 summation bound by {worst:.3f}x"


def check_entropy(stats, ent, tag):
    ratio = float((np.abs(stats[:, 6].astype(np.float64) - ent) / (ENT_REL * ent + ENT_ABS)).max())
    print(f"{tag}: entropy error / bound = {ratio:.3e}")
    assert ratio <= 1.0, f"{tag}: entropy misses its bound by {ratio:.3f}x"


def check_sigma(stats):
    s = stats[:, :3].astype(np.float32)
    want = np.sqrt((s[:, 0] + s[:, 1]) + s[:, 2], dtype=np.float32)
    assert np.array_equal(stats[:, 11].view(np.int32), want.view(np.int32))


def check_peak(stats, idx, p, c):
    assert idx.dtype == np.int32
    assert np.array_equal(idx, p.argmax(axis=1).astype(np.int32))          # np.argmax: the lowest index of the maximum
    assert np.array_equal(stats[:, 7].view(np.int32), p.max(axis=1).view(np.int32))
    assert np.array_equal(stats[:, 8:11].view(np.int32), c[idx].view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("rows,G", CASES)
def test_peak_exact(rows, G):
    k = case(rows, G)
    check_peak(k["stats"], k["idx"], k["p"], k["c"])


@pytest.mark.parametrize("rows,G", CASES)
def test_covariance_within_float32_summation_bound(rows, G):
    k = case(rows, G)
    assert np.isfinite(k["stats"]).all()
    check_cov(k["stats"], k["cov"], f"rows {rows} G {G}")


@pytest.mark.parametrize("rows,G", CASES)
def test_entropy_within_bound(rows, G):
    k = case(rows, G)
    check_entropy(k["stats"], k["ent"], f"rows {rows} G {G}")


@pytest.mark.parametrize("rows,G", CASES)
def test_sigma_is_sqrtf_of_the_kernels_own_trace(rows, G):
    check_sigma(case(rows, G)["stats"])


# (rows, G, row, a, b): a < b.  At G = 24 a chunk is 56 voxels (lane t of pass 1 holds voxels 4t .. 4t+3 of it), pass 2's lane is chunk % 64
TIES = [(15, 24, 7, 2 * 56 + 1, 100 * 56 + 50),      # different chunks; lower index in the lower lane of both passes
        (15, 24, 7, 2 * 56 + 50, 100 * 56 + 1),      # lower index in the HIGHER lane of pass 1
        (15, 24, 3, 10 * 56 + 3, 70 * 56 + 3),       # lower index in the HIGHER lane of pass 2 (chunk 10 -> lane 10, chunk 70 -> lane 6)
        (15, 24, 0, 5 * 56 + 8, 5 * 56 + 10),        # one lane's own four voxels
        (1, 8, 0, 5, 301),                           # chunks of 4 voxels
        (15, 64, 14, 5 * 1024 + 12, 5 * 1024 + 800)]  # one chunk, waves 0 and 3 of the workgroup


@pytest.mark.parametrize("rows,G,row,a,b", TIES)
def test_tie_takes_the_lowest_index(rows, G, row, a, b):
    k = case(rows, G)
    v = np.float32(0.5 * (float(k["p"][row].max()) + 1.0))             # above every probability of the row
    assert v > k["p"][row].max()
    got = []
    for first, second in ((a, b), (b, a)):                              # the two positions swapped
        prob = k["prob"].clone()
        prob[row, first] = float(v)
        prob[row, second] = float(v)
        stats, idx = launch(prob, k["coord"], k["joints"])              # joints kept
        assert idx[row] == a and stats[row, 7] == v
        assert np.array_equal(stats[row, 8:11].view(np.int32), k["c"][a].view(np.int32))
        other = np.arange(rows) != row
        assert np.array_equal(stats[other].view(np.int32), k["stats"][other].view(np.int32))
        assert np.array_equal(idx[other], k["idx"][other])
        got.append((stats, idx))
    assert np.array_equal(got[0][0].view(np.int32), got[1][0].view(np.int32)) and np.array_equal(got[0][1], got[1][1])


def test_one_hot_rows():
    rows, G = 15, 8
    N = G ** 3
    coord = case(rows, G)["coord"]
    at = torch.tensor([(37 * r + 5) % N for r in range(rows)], device=DEV)
    at[0], at[1] = 0, N - 1
    prob = torch.zeros((rows, N), device=DEV)
    prob[torch.arange(rows, device=DEV), at] = 1.0
    stats, idx = launch(prob, coord, coord[at].contiguous())
    assert np.array_equal(idx, at.cpu().numpy().astype(np.int32))
    assert np.array_equal(stats[:, :7], np.zeros((rows, 7), dtype=np.float32))        # moments and entropy
    assert np.array_equal(stats[:, 7], np.ones(rows, dtype=np.float32))
    assert np.array_equal(stats[:, 8:11], coord[at].cpu().numpy())
    assert np.array_equal(stats[:, 11], np.zeros(rows, dtype=np.float32))


@pytest.mark.parametrize("G", [8, 24])
def test_uniform_rows(G):
    rows, N = 15, G ** 3
    k = case(rows, G)
    prob = torch.full((rows, N), 1.0 / N, device=DEV, dtype=torch.float32)
    mean = k["c"].astype(np.float64).mean(axis=0).astype(np.float32)
    joints = torch.from_numpy(np.tile(mean, (rows, 1))).to(DEV)
    stats, idx = launch(prob, k["coord"], joints)
    var = (SIDE / (G - 1)) ** 2 * (G * G - 1) / 12.0          # G equally spaced points over SIDE
    cov = np.tile(np.array([var, var, var, 0.0, 0.0, 0.0]), (rows, 1))
    # the float32 rounding of 1/N, of the coordinates and of the mean moves the model's own value by a few 2^-24 of var: far inside
    # the gate, so the analytic value is held to the same gate as the model
    check_cov(stats, cov, f"uniform G {G}")
    check_entropy(stats, np.full(rows, math.log(N)), f"uniform G {G}")
    assert (idx == 0).all() and (stats[:, 7] == np.float32(1.0 / N)).all()      # all equal: the lowest index
    check_sigma(stats)


@pytest.mark.parametrize("rows,G,row,at", [(15, 8, 7, 300), (15, 24, 14, 100 * 56 + 9), (15, 24, 0, 0)])
def test_nan_row(rows, G, row, at):
    k = case(rows, G)
    prob = k["prob"].clone()
    prob[row, at] = float("nan")
    stats, idx = launch(prob, k["coord"], k["joints"])
    assert np.isnan(stats[row]).all() and idx[row] == -1
    other = np.arange(rows) != row
    assert np.array_equal(stats[other].view(np.int32), k["stats"][other].view(np.int32))
    assert np.array_equal(idx[other], k["idx"][other])


@pytest.mark.parametrize("rows,G", [(15, 64), (120, 16), (15, 24)])
def test_two_launches_bitwise_equal(rows, G):
    k = case(rows, G)
    stats, idx = launch(k["prob"], k["coord"], k["joints"])
    assert np.array_equal(stats.view(np.int32), k["stats"].view(np.int32)) and np.array_equal(idx, k["idx"])


def test_bad_arguments_raise_and_do_not_launch():
    rows, G = 15, 8
    N = G ** 3
    k = case(rows, G)
    SENT = -7.0
    stats = torch.full((rows, 12), SENT, device=DEV)
    idx = torch.full((rows,), -7, device=DEV, dtype=torch.int32)
    prob, coord, joints = k["prob"], k["coord"], k["joints"]
    wide = torch.zeros((rows, 2 * N), device=DEV)
    bad = {
        "cpu prob": lambda: _lib.joint_stats(prob.cpu(), coord, joints, stats, idx, rows, N),
        "cpu joints": lambda: _lib.joint_stats(prob, coord, joints.cpu(), stats, idx, rows, N),
        "float64 prob": lambda: _lib.joint_stats(prob.double(), coord, joints, stats, idx, rows, N),
        "float32 peak_index": lambda: _lib.joint_stats(prob, coord, joints, stats, idx.float(), rows, N),
        "non-contiguous prob": lambda: _lib.joint_stats(wide[:, ::2], coord, joints, stats, idx, rows, N),
        "non-contiguous coord": lambda: _lib.joint_stats(prob, coord.t().contiguous().t(), joints, stats, idx, rows, N),
        "voxels % 4": lambda: _lib.joint_stats(torch.zeros((rows, 125), device=DEV), torch.zeros((125, 3), device=DEV), joints, stats, idx,
                                               rows, 125),
        "joints rows": lambda: _lib.joint_stats(prob, coord, torch.zeros((rows - 1, 3), device=DEV), stats, idx, rows, N),
        "coord voxels": lambda: _lib.joint_stats(prob, coord[:-4].contiguous(), joints, stats, idx, rows, N),
        "short scratch": lambda: _lib.joint_stats(prob, coord, joints, stats, idx, rows, N, scratch=torch.zeros(8, device=DEV)),
        "rows 0": lambda: _lib.joint_stats(prob, coord, joints, stats, idx, 0, N),
    }
    for name, call in bad.items():
        with pytest.raises(_lib.HipExtensionError):
            call()
        torch.cuda.synchronize()
        assert (stats == SENT).all() and (idx == -7).all(), f"{name}: something was launched"
    # the C entry point's own checks, behind the wrapper's
    lib = _lib.load()
    ws = torch.zeros(_lib.joint_stats_scratch_elems(rows), device=DEV)
    p = _lib._ptr
    assert lib.se_joint_stats_f32(p(prob), p(coord), p(joints), p(stats), p(idx), p(ws), rows, 125, None) == -1
    assert lib.se_joint_stats_f32(p(prob), p(coord), p(joints), p(stats), p(idx), p(ws), 0, N, None) == -1
    assert lib.se_joint_stats_f32(p(prob), p(coord), p(joints), p(stats), p(idx), p(ws), rows, 0, None) == -1
    assert lib.se_joint_stats_f32(p(prob), None, p(joints), p(stats), p(idx), p(ws), rows, N, None) == -1
    assert lib.se_joint_stats_f32(p(prob), p(coord), p(joints), p(stats), None, p(ws), rows, N, None) == -1
    assert lib.se_joint_stats_scratch_elems(0) == 0 and lib.se_joint_stats_scratch_elems(15) == 15 * 256 * 12
    torch.cuda.synchronize()
    assert (stats == SENT).all() and (idx == -7).all()


def test_op_surface_shapes_and_symmetry():
    B, J, G = 2, 15, 16
    k = case(B * J, G)
    vol = k["prob"].view(B, J, G, G, G)
    coord_volumes = k["coord"].view(1, G, G, G, 3).expand(3, -1, -1, -1, -1)
    s = op.joint_statistics(vol, coord_volumes, k["joints"].view(B, J, 3))
    torch.cuda.synchronize()
    assert set(s) == set(op.STAT_KEYS)
    assert tuple(s["cov"].shape) == (B, J, 3, 3) and tuple(s["peak_coord"].shape) == (B, J, 3)
    assert all(tuple(s[n].shape) == (B, J) for n in ("sigma", "entropy", "peak_prob", "peak_index"))
    assert s["peak_index"].dtype == torch.int32
    cov = s["cov"].cpu().numpy().reshape(B * J, 3, 3)
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    st = k["stats"]
    assert np.array_equal(cov[:, [0, 1, 2, 0, 0, 1], [0, 1, 2, 1, 2, 2]], st[:, :6])
    assert np.array_equal(s["sigma"].cpu().numpy().reshape(-1), st[:, 11]) and np.array_equal(s["entropy"].cpu().numpy().reshape(-1), st[:, 6])
    assert np.array_equal(s["peak_index"].cpu().numpy().reshape(-1), k["idx"])
    frames = op.joint_statistics_to_numpy(s)
    assert len(frames) == B and frames[1]["cov"].shape == (J, 3, 3) and frames[1]["peak_index"].dtype == np.int32


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def net64():
    net = VoxelNetwork_depth(load_config(), device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    return net.to(DEV).eval()


def _check_module_stats(net, kp, vols, tag):
    s = net.joint_statistics(vols, kp)                  # before anything else is queued: under graphs the buffers are static
    torch.cuda.synchronize()
    B, J = kp.shape[:2]
    p = vols.reshape(B * J, -1).cpu().numpy()
    c = net.coord_volumes[0].reshape(-1, 3).float().cpu().numpy()
    j = kp.reshape(B * J, 3).cpu().numpy()
    cov, ent = model(p, c, j)
    cv = s["cov"].cpu().numpy().reshape(B * J, 3, 3)
    stats = np.zeros((B * J, 12), dtype=np.float32)
    stats[:, :6] = cv[:, [0, 1, 2, 0, 0, 1], [0, 1, 2, 1, 2, 2]]
    stats[:, 6] = s["entropy"].cpu().numpy().reshape(-1)
    stats[:, 7] = s["peak_prob"].cpu().numpy().reshape(-1)
    stats[:, 8:11] = s["peak_coord"].cpu().numpy().reshape(-1, 3)
    stats[:, 11] = s["sigma"].cpu().numpy().reshape(-1)
    check_peak(stats, s["peak_index"].cpu().numpy().reshape(-1), p, c)
    check_cov(stats, cov, tag)
    check_entropy(stats, ent, tag)
    check_sigma(stats)


def test_module_joint_statistics_on_golden_forward(net64, golden_meta):
    m = next(c for c in golden_meta["cases"] if c["name"] == "b1_floor")
    img, depth = synth.make_inputs(m["input_seed"], m["batch"], m["depth_kind"])
    img, depth = img.to(DEV), depth.to(DEV)
    with torch.no_grad():
        kp, _, vols, _ = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)
    _check_module_stats(net64, kp, vols, "b1_floor eager")
    net64.enable_graphs(True)
    try:
        with torch.no_grad():
            kp, _, vols, _ = net64(img, net64.grid_coord_proj_batch, net64.coord_volumes, depth_map_batch=depth)
        _check_module_stats(net64, kp, vols, "b1_floor graph replay")
    finally:
        net64.enable_graphs(False)


def test_relu_volumes_are_refused():
    cfg = load_config()
    cfg.model.volume_softmax = False
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    G = net.volume_size
    with pytest.raises(ValueError):
        net.joint_statistics(torch.zeros((1, 15, G, G, G), device=DEV), torch.zeros((1, 15, 3), device=DEV))


def _check_frame_stats(st):
    assert set(st) == set(op.STAT_KEYS)
    assert st["cov"].shape == (15, 3, 3) and st["peak_coord"].shape == (15, 3) and st["peak_index"].dtype == np.int32
    assert all(st[n].shape == (15,) for n in ("sigma", "entropy", "peak_prob", "peak_index"))
    assert all(np.isfinite(st[n]).all() for n in ("cov", "sigma", "entropy", "peak_prob", "peak_coord"))
    tr = (st["cov"][:, 0, 0] + st["cov"][:, 1, 1]) + st["cov"][:, 2, 2]
    assert np.array_equal(st["sigma"], np.sqrt(tr, dtype=np.float32))
    assert (st["peak_prob"] > 0).all() and (st["peak_prob"] <= 1).all() and (st["peak_index"] >= 0).all() and (st["peak_index"] < 64 ** 3).all()
    assert (st["entropy"] >= 0).all() and (st["entropy"] <= math.log(64 ** 3) * (1 + 1e-4)).all()


def test_demo_stats_flag_writes_both_pickles(tmp_path, capsys):
    import shutil

    import demo
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg"), img_dir)
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), depth_dir)
    common = ["--img_dir", str(img_dir), "--depth_dir", str(depth_dir), "--weights", "synthetic"]
    demo.main(common + ["--output_dir", str(tmp_path / "plain")])
    demo.main(common + ["--output_dir", str(tmp_path / "stats"), "--stats", "true"])
    capsys.readouterr()
    assert sorted(os.listdir(tmp_path / "plain")) == ["img_001000.jpg.pkl"]
    assert sorted(os.listdir(tmp_path / "stats")) == ["img_001000.jpg.pkl", "img_001000.jpg.stats.pkl"]
    a = (tmp_path / "plain" / "img_001000.jpg.pkl").read_bytes()
    b = (tmp_path / "stats" / "img_001000.jpg.pkl").read_bytes()
    print("max |joints with --stats - joints without| =", float(np.abs(pickle.loads(a) - pickle.loads(b)).max()))
    assert a == b, "<img>.pkl differs between a run with and a run without --stats"
    with open(tmp_path / "stats" / "img_001000.jpg.stats.pkl", "rb") as f:
        _check_frame_stats(pickle.load(f))


def test_run_sequence_stats_output(tmp_path, capsys):
    import run_sequence
    depths = [os.path.join(GOLD, "demo", n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 11, depths, estimated_depth_name="est_depth", seed=5)
    common = ["--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
    plain = run_sequence.main(common)
    out = str(tmp_path / "out" / "stats.pkl")
    with_stats = run_sequence.main(common + ["--streams", "2", "--stats_output", out])
    capsys.readouterr()
    assert "stats" not in plain and len(with_stats["stats"]) == 11
    a, b = np.stack(plain["predictions"]), np.stack(with_stats["predictions"])
    assert a.shape == (11, 15, 3) and np.abs(a - b).max() <= 2e-5          # split-K atomics of the backbone (pipeline.py)
    with open(out, "rb") as f:
        frames = pickle.load(f)
    assert len(frames) == 11
    for st, mem in zip(frames, with_stats["stats"]):
        _check_frame_stats(st)
        assert all(np.array_equal(st[n], mem[n]) for n in op.STAT_KEYS)
    # the peak of a softmaxed volume and its soft-argmax sit in the same cuboid; sigma bounds their distance only loosely, so just
    # check that the statistics belong to the frames they are listed under: frames differ, so do their sigmas
    assert not np.array_equal(frames[0]["sigma"], frames[1]["sigma"])
