#!/usr/bin/env python3
"""Cost of the scene-constrained joints (VoxelNetwork_depth.constrain_to_scene: se_scene_free_mask_u8 + se_softargmax3d_masked_f32 +
its torch epilogue) beside the forward of the same batch, beside se_joint_stats_f32 on the same volumes (both read the same bytes: the
yardstick) and beside the same mask and reductions written in plain torch on the same device, at the shipped grid (64^3, 15 joints)
and the demo frame's 512 x 640 depth map.

    python tools/bench_scene_constraint.py [--batches 1 8 32] [--warmup 3] [--reps 20] [--baseline_reps 5] [--no_forward]
                                           [--no_baseline] [--out result.json]

HIP events around one call, median of --reps after --warmup.  ``mask_ms`` times the bare ``_lib.scene_free_mask`` call, ``reduce_ms``
the bare ``_lib.softargmax3d_masked`` call (both launches), ``method_ms`` the whole ``constrain_to_scene``; ``joint_stats_ms`` the bare
``_lib.joint_stats`` call on the same volumes.  ``reduce_gbps`` / ``joint_stats_gbps``: the bytes of the volumes (rows x voxels x 4 B,
read once; the coordinates and the mask stay in cache) over the time: MB / ms = GB / s.  The inputs are random probabilities, not a
forward's volumes: the time of a streaming reduction does not depend on the values.  Prints one JSON line per batch."""
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
from sceneego_amd.render import MAX_DEPTH  # noqa: E402
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


def torch_mask(depth, pix, rng, H, W, margin, max_depth):
    """The free mask in plain torch (float64 sum and comparison): uint8 [B,N]."""
    dh, dw = depth.shape[1:]
    seen = pix >= 0
    p = torch.where(seen, pix, torch.zeros_like(pix)).long()
    py, px = (p // W * dh) // H, (p % W * dw) // W
    d = depth[:, py, px].double()
    blocked = seen[None] & (d > 0) & (d <= max_depth) & (d + margin < rng.double()[None])
    return (~blocked).to(torch.uint8)


def torch_reduce(vol, coord, free, joints):
    """The masked reductions in plain torch float32: (joints, free_mass, free_peak_prob, free_peak_index)."""
    B, J, N = vol.shape
    f = free.view(B, 1, N) != 0
    pf = torch.where(f, vol, torch.zeros_like(vol))
    mass = pf.sum(dim=2)
    sums = pf @ coord                                                          # [B,J,3]
    peak, index = torch.where(f, vol, torch.full_like(vol, -1.0)).max(dim=2)
    out = torch.where((mass > 0)[..., None], sums / mass[..., None], joints)
    return out, mass, peak, index


def measure(net, depth_half, B, args):
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
    out = torch.empty((rows, _lib.MASKED_SLOTS), device=dev, dtype=torch.float32)
    index = torch.empty((rows,), device=dev, dtype=torch.int32)
    scratch = torch.empty(_lib.softargmax3d_masked_scratch_elems(rows), device=dev, dtype=torch.float32)
    stats = torch.empty((rows, _lib.JOINT_STATS_SLOTS), device=dev, dtype=torch.float32)
    js_scratch = torch.empty(_lib.joint_stats_scratch_elems(rows), device=dev, dtype=torch.float32)
    r = {"batch": B, "rows": rows, "grid": G, "frame": [H, W], "depth": list(depth.shape[1:]), "margin": margin}
    mb = rows * N * 4 / 1e6
    r["volumes_mb"] = round(mb, 1)

    put(r, "mask_ms", timed(lambda: _lib.scene_free_mask(depth, pix, rng, free, H, W, margin, MAX_DEPTH), args.warmup, args.reps))
    r["free_share"] = round(float(free.float().mean()), 4)
    put(r, "reduce_ms", timed(lambda: _lib.softargmax3d_masked(vol, coord, free, out, index, rows, J, N, scratch=scratch),
                              args.warmup, args.reps))
    r["reduce_gbps"] = round(mb / r["reduce_ms"], 1)
    put(r, "joint_stats_ms", timed(lambda: _lib.joint_stats(vol, coord, joints.view(rows, 3), stats, index, rows, N, scratch=js_scratch),
                                   args.warmup, args.reps))
    r["joint_stats_gbps"] = round(mb / r["joint_stats_ms"], 1)
    r["reduce_over_joint_stats"] = round(r["reduce_ms"] / r["joint_stats_ms"], 3)
    put(r, "method_ms", timed(lambda: net.constrain_to_scene(vol, joints, depth), args.warmup, args.reps))

    if not args.no_baseline:
        # the baseline, and that it computes the same thing
        c = net.constrain_to_scene(vol, joints, depth)
        tf = torch_mask(depth, pix, rng, H, W, margin, MAX_DEPTH)
        tj, tm, tp, ti = torch_reduce(vol.view(B, J, N), coord, tf, joints)
        r["baseline_matches"] = bool(torch.equal(tf, c["free"].view(B, N)) and torch.equal(ti.int(), c["free_peak_index"])
                                     and torch.equal(tp, c["free_peak_prob"]) and torch.allclose(tm, c["free_mass"], rtol=1e-4, atol=0)
                                     and torch.allclose(tj, c["joints"], rtol=0, atol=1e-4))
        put(r, "torch_mask_ms", timed(lambda: torch_mask(depth, pix, rng, H, W, margin, MAX_DEPTH), 1, args.baseline_reps))
        put(r, "torch_reduce_ms", timed(lambda: torch_reduce(vol.view(B, J, N), coord, tf, joints), 1, args.baseline_reps))
        r["torch_over_method"] = round((r["torch_mask_ms"] + r["torch_reduce_ms"]) / r["method_ms"], 1)

    if not args.no_forward:
        img, d = synth.make_inputs(77, B, "floor")
        img, d = img.to(dev), d.to(dev)

        def forward():
            with torch.no_grad():
                net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=d)
        put(r, "forward_ms", timed(forward, 2, max(3, args.reps // 4)))
        r["method_share_of_forward"] = round(r["method_ms"] / r["forward_ms"], 4)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline_reps", type=int, default=5)
    ap.add_argument("--no_forward", action="store_true", help="skip the forward beside it")
    ap.add_argument("--no_baseline", action="store_true", help="skip the torch baseline (profiler runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_constraint.py needs an MI355X (HIP device)")
    from sceneego_amd.preprocess import load_depth
    dev = torch.device("cuda")
    cfg = load_config()
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(dev).eval()
    depth_half = torch.from_numpy(load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr"))).to(dev)
    results = []
    for B in args.batches:
        r = measure(net, depth_half, B, args)
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return results


if __name__ == "__main__":
    main()
