"""GPU: the scene check.  se_scene_probe_f64 against tests/scene_model.py bit for bit (np.array_equal on the raw bits of `out` and
on `index`: no tolerance, no mask, each case launched twice), its argument checks, SceneConsistency at full size on the demo frame
stated without the model, check() on the network's joints, and the three command lines."""
import functools
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import scene_cases as C
import scene_model as M
from conftest import CALIB, GOLD, synthetic_state_dict
from sceneego_amd import _lib, metrics, synth
from sceneego_amd.op import SCENE_KEYS, scene_check_to_numpy
from sceneego_amd.scene_check import SceneConsistency

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.0


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared inputs are read-only


def gpu_probe(k):
    depth, tab, probes = dev(k["depth"]), dev(k["ray_tab"]), dev(k["probes"])
    B, P = probes.shape[:2]
    out = torch.full((B, P, 8), SENT, device=DEV, dtype=torch.float64)
    index = torch.full((B, P, 2), 77, device=DEV, dtype=torch.int32)
    _lib.scene_probe(depth, tab, probes, out, index, min_z=C.MIN_Z, max_depth=C.MAX_DEPTH)
    torch.cuda.synchronize()
    return out.cpu().numpy(), index.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", C.CASES)
def test_probe_equals_the_model_bit_for_bit(name):
    k = C.inputs(name)
    out, index = gpu_probe(k)
    want_out, want_index = C.model(name)
    print(f"{name}: B={k['probes'].shape[0]} P={k['probes'].shape[1]} rays {k['ray_tab'].shape[:2]}: "
          f"{int((M.bits(out) != M.bits(want_out)).sum())} of {out.size} values and {int((index != want_index).sum())} of {index.size} "
          f"indices differ")
    assert np.array_equal(M.bits(out), M.bits(want_out))
    assert index.dtype == np.int32 and np.array_equal(index, want_index)
    again_out, again_index = gpu_probe(k)
    assert np.array_equal(M.bits(again_out), M.bits(out)) and np.array_equal(again_index, index), "two launches differ"


def test_edge_rows_stated_without_the_model():
    out, index = gpu_probe(C.inputs("empty_frame"))
    assert np.isposinf(out[1, :, 0]).all() and np.isnan(out[1, :, 1:4]).all() and (index[1, :, 0] == -1).all()
    assert np.isfinite(out[1, :, 4:6]).all() and (index[1, :, 1] >= 0).all() and (out[1, :, 7] == 0.0).all()     # the sight half
    assert np.isfinite(out[[0, 2], :, :6]).all() and (index[[0, 2]] >= 0).all()
    out, index = gpu_probe(C.inputs("bad_probe"))
    assert np.isnan(out[0, 3]).all() and np.isnan(out[1, 14]).all() and (index[0, 3] == -1).all() and (index[1, 14] == -1).all()
    rest = np.ones((2, 15), dtype=bool)
    rest[0, 3] = rest[1, 14] = False
    assert np.isfinite(out[rest][:, :6]).all() and (index[rest] >= 0).all()
    k = C.inputs("multi_tile")
    out, index = gpu_probe(k)
    H, W = k["ray_tab"].shape[:2]
    assert out[1, 59, 0] == 0.0 and index[1, 59, 0] == H * W - 1 and out[0, 0, 0] == 0.0 and index[0, 0, 0] == 2048
    k = C.inputs("ties")
    out, index = gpu_probe(k)
    for n in (index[0, 0, 0], index[0, 1, 0], index[0, 2, 1]):                 # the first pixel of a 4 x 4 block of equal rays
        y, x = divmod(int(n), k["ray_tab"].shape[1])
        assert y % 4 == 0 and x % 4 == 0


def test_bad_arguments():
    k = C.inputs("small")
    depth, tab, probes = dev(k["depth"]), dev(k["ray_tab"]), dev(k["probes"])
    out = torch.full((2, 15, 8), SENT, device=DEV, dtype=torch.float64)
    index = torch.full((2, 15, 2), 77, device=DEV, dtype=torch.int32)
    need = _lib.scene_probe_scratch_bytes(2, 24, 40, 15)
    scratch = torch.zeros((need,), device=DEV, dtype=torch.uint8)
    lib, p = _lib.load(), _lib._ptr
    ptrs = [p(depth), p(tab), p(probes), p(out), p(index), p(scratch)]
    good = dict(scratch_bytes=need, batch=2, depth_h=12, depth_w=20, height=24, width=40, n_probes=15, min_z=0.1, max_depth=100.0)

    def call(ptrs=ptrs, **change):
        a = dict(good, **change)
        return lib.se_scene_probe_f64(*ptrs, a["scratch_bytes"], a["batch"], a["depth_h"], a["depth_w"], a["height"], a["width"],
                                      a["n_probes"], a["min_z"], a["max_depth"], None)

    bad = [dict(batch=0), dict(batch=-1), dict(batch=65536), dict(n_probes=0), dict(n_probes=65), dict(depth_h=0), dict(depth_w=-3),
           dict(height=0), dict(width=0), dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(min_z=-0.1), dict(min_z=float("nan")),
           dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=float("nan"))]
    for change in bad:
        assert call(**change) == -1, change
    for i in range(6):
        assert call(ptrs=ptrs[:i] + [None] + ptrs[i + 1:]) == -1, f"null pointer {i}"
    torch.cuda.synchronize()
    assert (out == SENT).all() and (index == 77).all() and (scratch == 0).all(), "a refused call launched something"
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(M.bits(out.cpu().numpy()), M.bits(C.model("small")[0]))

    wrong = [lambda: _lib.scene_probe(depth.double(), tab, probes, out, index),                       # dtype
             lambda: _lib.scene_probe(depth, tab.float(), probes, out, index),
             lambda: _lib.scene_probe(depth, tab, probes.float(), out, index),
             lambda: _lib.scene_probe(depth, tab, probes[:1], out, index),                            # batch mismatch
             lambda: _lib.scene_probe(depth, tab, probes, out[:, :14], index),                        # shape
             lambda: _lib.scene_probe(depth, tab, probes, out, index.long()),
             lambda: _lib.scene_probe(depth, tab.permute(1, 0, 2), probes, out, index),               # contiguity
             lambda: _lib.scene_probe(depth.cpu(), tab, probes, out, index),                          # device
             lambda: _lib.scene_probe(depth, tab, torch.zeros((2, 65, 3), device=DEV, dtype=torch.float64), out, index),
             lambda: _lib.scene_probe(depth, tab, probes, out, index, scratch=scratch[:-1]),
             lambda: _lib.scene_probe(depth, tab, probes, out, index, min_z=-1.0)]
    for fn in wrong:
        with pytest.raises(_lib.HipExtensionError):
            fn()


# ------------------------------------------------------------------------------------------------------------------ full size
@functools.lru_cache(maxsize=None)
def demo_scene():
    """(depth [512,640] float32 of the golden demo frame, SceneConsistency at 1024 x 1280, its ray table on the host)."""
    from sceneego_amd.preprocess import load_depth
    depth = load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr"))
    sc = SceneConsistency(CALIB, device=DEV)
    assert tuple(sc.ray_tab.shape) == (1024, 1280, 3) and sc.voxel_edge == 2.0 / 64
    return depth, sc, sc.ray_tab.cpu().numpy()


def test_hand_placed_probes_on_the_demo_frame():
    depth, sc, tab = demo_scene()
    H, W = tab.shape[:2]
    dh, dw = depth.shape
    y, x = 600, 700
    n = y * W + x
    d = float(depth[(y * dh) // H, (x * dw) // W])
    assert 0.0 < d <= 100.0 and tab[y, x, 2] * d > 0.1, "the picked pixel must be a scene point"
    ray = tab[y, x]
    three = np.stack([ray * (0.9 * d), ray * np.float64(d), ray * (1.1 * d)])
    depth2 = np.stack([depth, depth])
    r = sc.probe(depth2, np.stack([three, three]))
    r = {k: v.cpu().numpy() for k, v in r.items()}
    flat = tab.reshape(-1, 3)
    for b in range(2):
        for p in range(3):
            m = int(r["sight_index"][b, p])
            assert m == n or (m < n and np.array_equal(flat[m], flat[n])), (b, p, m, n)
        assert r["nearest_q"][b, 1] == 0.0 and r["in_view"][b].all()
        c = r["clearance"][b]
        print(f"frame {b}: pixel {n} at {d:.6f} m: clearance {c.tolist()}, penetration depth {r['penetration_depth'][b]:.6f}")
        assert c[0] > 0 and c[2] < 0 and abs(c[1]) <= 1e-9
        assert abs(c[0] - 0.1 * d) <= 1e-9 and abs(c[2] + 0.1 * d) <= 1e-9
        assert r["penetrating"][b] and abs(r["penetration_depth"][b] - 0.1 * d) <= 1e-9
    without = sc.probe(depth2, np.stack([three[:2], three[:2]]))
    assert not without["penetrating"].any().item() and float(without["penetration_depth"].max()) <= 1e-9
    # a shared table: the SceneRenderer's upload serves the check too
    other = SceneConsistency(None, device=DEV, ray_tab=sc.ray_tab)
    assert other.ray_tab.data_ptr() == sc.ray_tab.data_ptr()
    again = other.probe(depth2, np.stack([three, three]))
    assert np.array_equal(M.bits(again["clearance"].cpu().numpy()), M.bits(r["clearance"]))


@functools.lru_cache(maxsize=None)
def network():
    from sceneego_amd import load_config
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    net = VoxelNetwork_depth(load_config(), device="cpu", verbose=False)
    net.load_state_dict(synthetic_state_dict(False), strict=True)
    return net.to(DEV).eval()


def _forward(net, img, depth):
    with torch.no_grad():
        kp, _, _, _ = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)
    return kp


def test_check_on_the_network_joints_of_the_demo_frame():
    from sceneego_amd.preprocess import normalize_u8, prepare_depth
    depth_half, sc, _ = demo_scene()
    net = network()
    img = normalize_u8(np.load(os.path.join(GOLD, "demo", "img_001000_256_bgr_u8.npz"))["img"])[None].to(DEV)
    depth = prepare_depth(depth_half)[None].to(DEV)
    net.enable_graphs(True)
    try:
        _forward(net, img, depth)                                      # captures
        plain = _forward(net, img, depth).clone()                      # a second forward with nothing in between
        torch.cuda.synchronize()
        kp = _forward(net, img, depth)
        r = sc.check(depth, kp)
        after = _forward(net, img, depth).clone()                      # ... and one with a check() between two forwards
        torch.cuda.synchronize()
    finally:
        net.enable_graphs(False)
    assert torch.equal(after, plain), "check() disturbed the replayed forward"

    shapes = {"nearest_dist": ((1, 15), torch.float64), "nearest_point": ((1, 15, 3), torch.float64),
              "nearest_index": ((1, 15), torch.int32), "range": ((1, 15), torch.float64), "sight_index": ((1, 15), torch.int32),
              "in_view": ((1, 15), torch.bool), "clearance": ((1, 15), torch.float64), "bone_clearance": ((1, 15), torch.float64),
              "penetration_depth": ((1,), torch.float64), "penetrating": ((1,), torch.bool), "contact": ((1, 15), torch.bool)}
    assert set(r) == set(shapes) == set(SCENE_KEYS)
    for key, (shape, dtype) in shapes.items():
        assert tuple(r[key].shape) == shape and r[key].dtype == dtype and r[key].device.type == "cuda", key
    host = scene_check_to_numpy(r)
    assert len(host) == 1 and host[0]["nearest_point"].shape == (15, 3) and host[0]["penetration_depth"].shape == ()

    # bone_clearance against the NaN-ignoring minimum recomputed on the host from a P = 60 kernel call
    probes = SceneConsistency.probes(plain, 3)
    assert tuple(probes.shape) == (1, 60, 3)
    out = torch.empty((1, 60, 8), device=DEV, dtype=torch.float64)
    index = torch.empty((1, 60, 2), device=DEV, dtype=torch.int32)
    _lib.scene_probe(depth.contiguous(), sc.ray_tab, probes, out, index)    # prepare_depth returns a strided view
    o = out.cpu().numpy()[0]
    rng = np.sqrt(o[:, 4])
    with np.errstate(invalid="ignore", divide="ignore"):
        in_view = (rng > 0) & (o[:, 5] / rng >= np.cos(np.radians(1.0)))
    clearance = np.where(in_view, o[:, 6] - rng, np.nan)
    want = np.full(15, np.nan)
    for e, (a, b) in enumerate(_lib.SKELETON_LINES):
        vals = np.concatenate([clearance[[a, b]], clearance[15 + 3 * e:15 + 3 * e + 3]])
        if not np.isnan(vals).all():
            want[e] = np.nanmin(vals)
    got = host[0]["bone_clearance"]
    print(f"bone clearance {got.tolist()}, joints in view {int(host[0]['in_view'].sum())} of 15")
    # the kernel's part is exact; the square root of the range is taken on the device there and on the host here, and the two may
    # round differently: one unit in the last place of the range (a few metres at most), which the subtraction passes on
    tol = 4 * np.finfo(np.float64).eps * max(float(rng.max()), 10.0)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.abs(got[~np.isnan(got)] - want[~np.isnan(want)]).max(initial=0.0) <= tol
    mine = host[0]["clearance"]
    assert np.array_equal(np.isnan(mine), np.isnan(clearance[:15]))
    assert np.abs(mine[~np.isnan(mine)] - clearance[:15][~np.isnan(mine)]).max(initial=0.0) <= tol
    defined = clearance[~np.isnan(clearance)]
    assert abs(host[0]["penetration_depth"] - (max(0.0, -defined.min()) if len(defined) else 0.0)) <= tol
    assert host[0]["penetrating"] == (host[0]["penetration_depth"] > 2.0 / 64)
    assert np.array_equal(host[0]["contact"], np.sqrt(o[:15, 0]) <= 4.0 / 64)


# ------------------------------------------------------------------------------------------------------------------ command lines
def _check_frame(fr):
    assert set(fr) == set(SCENE_KEYS)
    for key in SCENE_KEYS:
        want = () if key in ("penetration_depth", "penetrating") else (15, 3) if key == "nearest_point" else (15,)
        assert isinstance(fr[key], np.ndarray) and fr[key].shape == want, key


def test_demo_scene_check_and_evaluate(tmp_path, capsys):
    import demo
    import evaluate
    img_dir, depth_dir = tmp_path / "imgs", tmp_path / "depths"
    img_dir.mkdir()
    depth_dir.mkdir()
    for name in ("a_001000.jpg", "b_001000.jpg"):
        shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg"), img_dir / name)
    shutil.copy(os.path.join(GOLD, "demo", "img_001000.jpg.exr"), depth_dir / "a_001000.jpg.exr")
    shutil.copy(os.path.join(GOLD, "demo", "img_001796.jpg.exr"), depth_dir / "b_001000.jpg.exr")
    common = ["--img_dir", str(img_dir), "--depth_dir", str(depth_dir), "--weights", "synthetic"]
    demo.main(common + ["--output_dir", str(tmp_path / "plain")])
    demo.main(common + ["--output_dir", str(tmp_path / "checked"), "--scene_check", "true"])
    capsys.readouterr()
    names = ["a_001000.jpg", "b_001000.jpg"]
    assert sorted(os.listdir(tmp_path / "plain")) == [n + ".pkl" for n in names]
    assert sorted(os.listdir(tmp_path / "checked")) == sorted([n + ".pkl" for n in names] + [n + ".scene.pkl" for n in names])
    frames = []
    for n in names:
        assert (tmp_path / "plain" / (n + ".pkl")).read_bytes() == (tmp_path / "checked" / (n + ".pkl")).read_bytes()
        with open(tmp_path / "checked" / (n + ".scene.pkl"), "rb") as f:
            frames.append(pickle.load(f))
        _check_frame(frames[-1])
    gt = np.zeros((2, 15, 3))
    with open(tmp_path / "gt.pkl", "wb") as f:
        pickle.dump(gt, f)
    r = evaluate.main(["--pred_dir", str(tmp_path / "checked"), "--gt", str(tmp_path / "gt.pkl"), "--scene", str(tmp_path / "checked")])
    out = capsys.readouterr().out
    assert r["frames"] == 2 and r["scene_summary"] == metrics.scene_summary(frames)
    assert out.splitlines()[-1] == metrics.format_scene_summary(r["scene_summary"])


def test_run_sequence_scene_output(tmp_path, capsys):
    import run_sequence
    depths = [os.path.join(GOLD, "demo", n) for n in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
    synth.make_sequence(str(tmp_path / "seq"), "zseq", 2, depths, estimated_depth_name="est_depth", seed=5)
    common = ["--root_dir", str(tmp_path / "seq"), "--seq_name", "zseq", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
    plain = run_sequence.main(common + ["--output", str(tmp_path / "plain.pkl")])
    assert "scene check:" not in capsys.readouterr().out
    checked = run_sequence.main(common + ["--output", str(tmp_path / "checked.pkl"), "--scene_output", str(tmp_path / "scene.pkl")])
    out = capsys.readouterr().out
    assert (tmp_path / "plain.pkl").read_bytes() == (tmp_path / "checked.pkl").read_bytes()
    assert "scene" not in plain and len(checked["scene"]) == 2
    with open(tmp_path / "scene.pkl", "rb") as f:
        frames = pickle.load(f)
    assert len(frames) == 2
    for fr in frames:
        _check_frame(fr)
    assert out.splitlines()[-1] == metrics.format_scene_summary(metrics.scene_summary(frames))
