#!/usr/bin/env python3
"""Cost of the scene distance field at the shipped grid (64^3, 15 joints) and the demo frame's 512 x 640 depth map:
``SceneField.build`` split into its parts (se_scene_sites_u8, se_scene_distance_i32, the torch epilogue) with the free mask
(se_scene_free_mask_u8) beside them; se_scene_expect_f32 beside se_joint_stats_f32 and se_softargmax3d_masked_f32 on the same volumes
(all three read the same probability bytes once: the ratio to them is the figure to report); both against the same quantities written
in plain torch on the same device; and all of it beside the forward of the same batch.

    python tools/bench_scene_field.py [--batches 1 8 32] [--warmup 3] [--reps 20] [--baseline_reps 5] [--no_forward]
                                      [--no_baseline] [--out result.json]

HIP events around one call, median of --reps after --warmup.  ``sites_ms`` / ``distance_ms`` / ``mask_ms`` / ``expect_ms`` /
``joint_stats_ms`` / ``masked_ms`` time the bare ``_lib`` calls, ``build_ms`` the whole ``SceneField.build`` and ``method_ms`` the
whole ``VoxelNetwork_depth.scene_expectations`` with a field built before.  ``*_gbps``: the bytes of the volumes (rows x voxels x
4 B, read once; the field and the mask, 5 B per voxel and FRAME, are shared by the frame's 15 rows) over the time: MB / ms = GB / s.
The volumes are random probabilities, not a forward's: the time of a streaming reduction does not depend on the values.  Prints one
JSON line per batch."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sceneego_amd import _lib, load_config, op, synth  # noqa: E402
from sceneego_amd.render import MAX_DEPTH, MIN_Z  # noqa: E402
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def timed(fn, warmup, reps):
    """(median, min, max) milliseconds of fn()."""
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def put(r, name, t):
    r[name], r[name + "_range"] = round(t[0], 4), [round(t[1], 4), round(t[2], 4)]


def torch_sites(depth, ray_tab, G, side):
    """The sites in plain torch (float64, the same operations): uint8 [B, G^3]."""
    B, dh, dw = depth.shape
    H, W = ray_tab.shape[:2]
    pix = torch.arange(H * W, device=depth.device)
    py, px = (pix // W * dh) // H, (pix % W * dw) // W
    ray = ray_tab.reshape(-1, 3)
    d = depth[:, py, px].double()                                                      # [B, H W]
    ok = torch.isfinite(ray).all(dim=1)[None] & (d > 0) & (d <= MAX_DEPTH)
    s = ray[None] * d[..., None]
    ok = ok & (s[..., 2] > MIN_Z)
    q = torch.stack([torch.round(((s[..., 0] + side / 2) * (G - 1)) / side), torch.round(((s[..., 1] + side / 2) * (G - 1)) / side),
                     torch.round((s[..., 2] * (G - 1)) / side)], dim=-1)              # torch.round: half to even
    ok = ok & (q >= 0).all(dim=-1) & (q <= G - 1).all(dim=-1)
    n = torch.where(ok, (q[..., 0] * G + q[..., 1]) * G + q[..., 2], torch.zeros_like(d)).long()
    out = torch.zeros((B, G ** 3), device=depth.device, dtype=torch.uint8)
    out.view(-1)[(torch.arange(B, device=depth.device)[:, None] * G ** 3 + n)[ok]] = 1
    return out


def torch_distance(sites, G):
    """The exact transform in plain torch: three separable passes of a G x G minimum over int64 keys d2 * 2^32 + index, one slab of
    G^3 candidates at a time.  (d2, nearest) int32 [B, G^3]."""
    B = sites.shape[0]
    dev = sites.device
    inf = (0x7fffffff << 32) | 0xffffffff
    idx = torch.arange(G ** 3, device=dev).view(1, G, G, G)
    key = torch.where(sites.view(B, G, G, G) != 0, idx, torch.full_like(idx, inf))
    a = torch.arange(G, device=dev)
    off = ((a[:, None] - a[None]) ** 2) << 32                                          # [out, cand]
    for axis in (3, 2, 1):
        k = key.movedim(axis, -1).contiguous()                                         # [B, a, b, cand]
        res = torch.empty_like(k)
        for b in range(B):
            for i in range(G):
                line = k[b, i][:, None, :]
                res[b, i] = torch.where(line >= inf, line, line + off).min(dim=-1).values
        key = res.movedim(-1, axis)
    none = key >= inf
    d2 = torch.where(none, torch.full_like(key, 0x7fffffff), key >> 32).int().reshape(B, -1)
    near = torch.where(none, torch.full_like(key, -1), key & 0xffffffff).int().reshape(B, -1)
    return d2, near


def torch_expect(vol, d2, free, rad):
    """The reduction in plain torch float32: [B, J, 4 + 2 K] (mass, blocked, distance, free distance, contact, free contact)."""
    B, J, N = vol.shape
    f = (free.view(B, 1, N) != 0)
    has = (d2.view(B, 1, N) != 0x7fffffff)
    t = vol * torch.sqrt(torch.where(has, d2.view(B, 1, N), torch.zeros_like(d2.view(B, 1, N))).float())
    within = d2.view(B, 1, N, 1) <= rad.view(1, 1, 1, -1)                              # [B,1,N,K]
    contact = torch.einsum("bjn,bnk->bjk", vol, within[:, 0].float())
    contact_free = torch.einsum("bjn,bnk->bjk", vol, (within[:, 0] & f[:, 0, :, None]).float())
    return torch.cat([vol.sum(2, keepdim=True), (vol * (~f)).sum(2, keepdim=True), t.sum(2, keepdim=True), (t * f).sum(2, keepdim=True),
                      contact, contact_free], dim=2)


def measure(net, sf, depth_half, B, args):
    dev = depth_half.device
    G, J = net.volume_size, net.num_joints
    N, rows = G ** 3, B * J
    H, W = net.image_height, net.image_width
    margin = net.cuboid_side / G
    depth = depth_half[None].expand(B, -1, -1).contiguous()
    g = torch.Generator(device=dev).manual_seed(B)
    vol = torch.softmax(8.0 * torch.randn((B, J, N), device=dev, generator=g), dim=2).view(B, J, G, G, G).contiguous()
    coord = net.coord_volumes[0].reshape(N, 3).to(device=dev, dtype=torch.float32).contiguous()
    joints = (vol.view(B, J, N) @ coord).contiguous()
    pix, rng = (t.to(dev) for t in op.build_sight_table(net.grid_coord_proj, net.coord_volume, H, W))
    free = torch.empty((B, N), device=dev, dtype=torch.uint8)
    sites = torch.empty((B, N), device=dev, dtype=torch.uint8)
    d2 = torch.empty((B, N), device=dev, dtype=torch.int32)
    near = torch.empty((B, N), device=dev, dtype=torch.int32)
    ws = torch.empty(_lib.scene_distance_scratch_bytes(B, G), device=dev, dtype=torch.uint8)
    rad = torch.tensor(op.DEFAULT_RADII2, device=dev, dtype=torch.int32)
    out = torch.empty((rows, _lib.EXPECT_SLOTS), device=dev, dtype=torch.float32)
    scratch = torch.empty(_lib.scene_expect_scratch_elems(rows), device=dev, dtype=torch.float32)
    m_out = torch.empty((rows, _lib.MASKED_SLOTS), device=dev, dtype=torch.float32)
    index = torch.empty((rows,), device=dev, dtype=torch.int32)
    m_scratch = torch.empty(_lib.softargmax3d_masked_scratch_elems(rows), device=dev, dtype=torch.float32)
    stats = torch.empty((rows, _lib.JOINT_STATS_SLOTS), device=dev, dtype=torch.float32)
    js_scratch = torch.empty(_lib.joint_stats_scratch_elems(rows), device=dev, dtype=torch.float32)
    r = {"batch": B, "rows": rows, "grid": G, "frame": [H, W], "depth": list(depth.shape[1:])}
    mb = rows * N * 4 / 1e6
    r["volumes_mb"] = round(mb, 1)

    put(r, "sites_ms", timed(lambda: _lib.scene_sites(depth, sf.ray_tab, sites, G, sf.side, MIN_Z, MAX_DEPTH), args.warmup, args.reps))
    r["site_share"] = round(float((sites != 0).float().mean()), 5)
    put(r, "distance_ms", timed(lambda: _lib.scene_distance(sites, d2, near, B, G, scratch=ws), args.warmup, args.reps))
    put(r, "mask_ms", timed(lambda: _lib.scene_free_mask(depth, pix, rng, free, H, W, margin, MAX_DEPTH), args.warmup, args.reps))
    put(r, "build_ms", timed(lambda: sf.build(depth), args.warmup, args.reps))
    put(r, "expect_ms", timed(lambda: _lib.scene_expect(vol, d2, free, rad, out, rows, J, N, scratch=scratch), args.warmup, args.reps))
    r["expect_gbps"] = round(mb / r["expect_ms"], 1)
    put(r, "joint_stats_ms", timed(lambda: _lib.joint_stats(vol, coord, joints.view(rows, 3), stats, index, rows, N, scratch=js_scratch),
                                   args.warmup, args.reps))
    r["joint_stats_gbps"] = round(mb / r["joint_stats_ms"], 1)
    put(r, "masked_ms", timed(lambda: _lib.softargmax3d_masked(vol, coord, free, m_out, index, rows, J, N, scratch=m_scratch),
                              args.warmup, args.reps))
    r["masked_gbps"] = round(mb / r["masked_ms"], 1)
    r["expect_over_joint_stats"] = round(r["expect_ms"] / r["joint_stats_ms"], 3)
    r["expect_over_masked"] = round(r["expect_ms"] / r["masked_ms"], 3)
    field = sf.build(depth)
    put(r, "method_ms", timed(lambda: net.scene_expectations(vol, depth=depth, field=field), args.warmup, args.reps))

    if not args.no_baseline:
        # the baselines, and that they compute the same thing
        ts = torch_sites(depth, sf.ray_tab, G, sf.side)
        td2, tnear = torch_distance(ts[:1], G)                                         # one frame: the frames repeat
        te = torch_expect(vol.view(B, J, N), d2, free, rad)
        K = rad.numel()
        mine = out.view(B, J, -1)
        mine = torch.cat([mine[..., :4], mine[..., 4:4 + K], mine[..., 12:12 + K]], dim=2)
        r["baseline_matches"] = bool(torch.equal(ts, sites) and torch.equal(td2[0], d2[0]) and torch.equal(tnear[0], near[0])
                                     and torch.allclose(te, mine, rtol=1e-4, atol=1e-7))
        put(r, "torch_sites_ms", timed(lambda: torch_sites(depth, sf.ray_tab, G, sf.side), 1, args.baseline_reps))
        put(r, "torch_distance_ms_per_frame", timed(lambda: torch_distance(ts[:1], G), 0, max(1, args.baseline_reps // 3)))
        put(r, "torch_expect_ms", timed(lambda: torch_expect(vol.view(B, J, N), d2, free, rad), 1, args.baseline_reps))
        r["torch_expect_over_expect"] = round(r["torch_expect_ms"] / r["expect_ms"], 1)

    if not args.no_forward:
        img, d = synth.make_inputs(77, B, "floor")
        img, d = img.to(dev), d.to(dev)

        def forward():
            with torch.no_grad():
                net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=d)
        put(r, "forward_ms", timed(forward, 2, max(3, args.reps // 4)))
        r["field_and_method_share_of_forward"] = round((r["build_ms"] + r["method_ms"]) / r["forward_ms"], 4)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline_reps", type=int, default=5)
    ap.add_argument("--no_forward", action="store_true", help="skip the forward beside it")
    ap.add_argument("--no_baseline", action="store_true", help="skip the torch baselines (profiler runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_field.py needs an MI355X (HIP device)")
    from sceneego_amd.config import resolve_calibration_path
    from sceneego_amd.preprocess import load_depth
    from sceneego_amd.scene_field import SceneField
    dev = torch.device("cuda")
    cfg = load_config()
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(dev).eval()
    sf = SceneField(resolve_calibration_path(cfg.dataset.camera_calibration_path),
                    frame_size=(cfg.dataset.image_height, cfg.dataset.image_width), config=cfg, device=dev)
    depth_half = torch.from_numpy(load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr"))).to(dev)
    results = []
    for B in args.batches:
        r = measure(net, sf, depth_half, B, args)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
