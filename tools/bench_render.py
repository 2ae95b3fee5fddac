#!/usr/bin/env python3
"""Cost of the headless renderer (csrc/render.hip) at the production size: a 1024 x 1280 frame, a 512 x 640 depth map and a
720 x 960 output, at B = 1 and 8.  HIP events around each entry point, warm, median of --iters (>= 20) calls; splat, resolve and
overlay are timed separately, with the ray-table bytes each reads per frame beside the time, and the batch-1 forward of the same
run for scale (what --render_dir adds to a frame).

    python tools/bench_render.py [--iters 30] [--out profiles/render_cost.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sceneego_amd import _lib, load_config, synth                      # noqa: E402
from sceneego_amd.config import resolve_calibration_path              # noqa: E402
from sceneego_amd.render import MAX_DEPTH, MIN_Z, NEAR, SceneRenderer, orbit_view   # noqa: E402
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth           # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def timed(fn, warmup, iters):
    """Median and minimum microseconds of ``fn`` (HIP events on the current stream)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_cost.txt"))
    args = ap.parse_args(argv)
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs an MI355X (HIP device)")
    from sceneego_amd.preprocess import load_depth, load_image_bgr
    dev = torch.device("cuda")
    cfg = load_config()
    frame = load_image_bgr(os.path.join(GOLD, "demo", "img_001000.jpg"))
    depth = load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr"))
    joints = np.load(os.path.join(GOLD, "demo_exr_b1.npz"))["joints"][0]
    r = SceneRenderer(resolve_calibration_path(cfg.dataset.camera_calibration_path), device=dev)
    H, W, Ho, Wo = r.H, r.W, r.Hout, r.Wout
    lines = [f"renderer cost, {torch.cuda.get_device_name(0)}; frame {H}x{W}, depth {depth.shape[0]}x{depth.shape[1]}, output {Ho}x{Wo}, "
             f"splat {r.splat}; HIP events, {args.warmup} warm-up + {args.iters} timed calls, median (minimum); library "
             f"{_lib.built_fingerprint()}",
             f"ray tables read per frame: splat and overlay {H * W * 24 / 1e6:.2f} MB (calibrated rays), resolve {Ho * Wo * 24 / 1e6:.2f} MB "
             f"(pinhole rays)", ""]
    lines.append(f"{'B':>2} {'entry point':<24} {'us/call':>10} {'(min)':>10} {'us/frame':>10} {'ray-table GB/s':>15}")
    view = torch.from_numpy(orbit_view()).to(dev)
    for B in (1, 8):
        img = torch.from_numpy(np.stack([frame] * B)).to(dev)
        d = torch.from_numpy(np.stack([depth] * B)).to(dev)
        j = torch.from_numpy(np.stack([joints] * B)).to(dev, torch.float64)
        R, t = view[:9].view(3, 3), view[9:]
        jv = (j @ R.T + t).contiguous()
        zbuf, out, over = r._buffers(B)
        steps = (("se_render_splat_f64", H * W * 24,
                  lambda: _lib.render_splat(d, r.ray_tab, img, view, zbuf, r.f, r.cx, r.cy, splat=r.splat, min_z=MIN_Z, max_depth=MAX_DEPTH, near=NEAR)),
                 ("se_render_resolve_f64", Ho * Wo * 24, lambda: _lib.render_resolve(r.pinhole, jv, zbuf, out, near=NEAR)),
                 ("se_render_overlay_f64", H * W * 24, lambda: _lib.render_overlay(r.ray_tab, j, img, over, depth=d, near=NEAR)),
                 ("render() + overlay()", 0, lambda: (r.render(d, img, j), r.overlay(img, j, depth=d))))
        for name, ray_bytes, fn in steps:
            med, lo = timed(fn, args.warmup, args.iters)
            # the table is read once per frame of the batch (from L2 / MALL after the first)
            bw = f"{ray_bytes * B / (med * 1e-6) / 1e9:15.1f}" if ray_bytes else f"{'':>15}"
            lines.append(f"{B:>2} {name:<24} {med:10.1f} {lo:10.1f} {med / B:10.1f} {bw}")
    # the batch-1 forward of the same run, graph replay as demo.py runs it
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(dev).eval()
    net.enable_graphs(True)
    im, dp = synth.make_inputs(77, 1, "floor")
    im, dp = im.to(dev), dp.to(dev)

    def forward():
        with torch.no_grad():
            net(im, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=dp)
    med, lo = timed(forward, args.warmup, args.iters)
    lines += ["", f" 1 {'forward (graph replay)':<24} {med:10.1f} {lo:10.1f} {med:10.1f}",
              "", "render() + overlay() is what --render_dir adds per rendered frame on the device (the joints' move to view space in torch "
              "included); the PNG encoding on the host comes on top and is not timed here."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
