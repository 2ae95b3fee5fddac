#!/usr/bin/env python3
"""Cost of the volume renderer (csrc/render_volume.hip) at the production size: a 1024 x 1280 frame, a 720 x 960 view, G = 64, at
B = 1 and 8, on the volumes of a synthetic-weights forward.  HIP events around each call, warm, median of --iters (>= 20) calls: the
pack pass, the view march and the overlay march separately (all joints and one joint), then SceneRenderer.render_volumes() +
overlay_volumes() end to end beside render() + overlay() and beside the forward of the same batch, all from one run.

    python tools/bench_volume_render.py [--iters 30] [--out profiles/volume_render_cost.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench_render import GOLD, timed                                   # noqa: E402
from sceneego_amd import _lib, load_config, synth                      # noqa: E402
from sceneego_amd.config import resolve_calibration_path              # noqa: E402
from sceneego_amd.render import NEAR, SceneRenderer, orbit_view        # noqa: E402
from sceneego_amd.voxel_net_depth import VoxelNetwork_depth           # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_render_cost.txt"))
    args = ap.parse_args(argv)
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_volume_render.py needs an MI355X (HIP device)")
    from sceneego_amd.preprocess import load_depth, load_image_bgr
    dev = torch.device("cuda")
    cfg = load_config()
    frame = load_image_bgr(os.path.join(GOLD, "demo", "img_001000.jpg"))
    depth = load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr"))
    r = SceneRenderer(resolve_calibration_path(cfg.dataset.camera_calibration_path), device=dev)
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(dev).eval()
    net.enable_graphs(True)
    G, side = net.volume_size, net.cuboid_side
    H, W, Ho, Wo = r.H, r.W, r.Hout, r.Wout
    lines = [f"volume renderer cost, {torch.cuda.get_device_name(0)}; frame {H}x{W}, depth {depth.shape[0]}x{depth.shape[1]}, view {Ho}x{Wo}, "
             f"G = {G}, cuboid {side} m; volumes of a synthetic-weights forward; HIP events, {args.warmup} warm-up + {args.iters} timed "
             f"calls, median (minimum); library {_lib.built_fingerprint()}",
             f"per frame: volumes {15 * G ** 3 * 4 / 1e6:.2f} MB read and packed copy {16 * G ** 3 * 4 / 1e6:.2f} MB written by the pack pass; "
             f"{Ho * Wo} view rays, {H * W} overlay rays; the marches are plain cell walks (no brick skip is built)", ""]
    lines.append(f"{'B':>2} {'step':<52} {'us/call':>10} {'(min)':>10} {'us/frame':>10}")
    view = orbit_view()
    for B in (1, 8):
        im, dp = synth.make_inputs(77, B, "floor")
        im, dp = im.to(dev), dp.to(dev)

        def forward():
            with torch.no_grad():
                return net(im, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=dp)
        kp, _, vol, _ = forward()
        torch.cuda.synchronize()
        peak = vol.amax(dim=(2, 3, 4))
        lines.append(f"{B:>2} volumes: per-joint maximum {peak.min().item():.3e} .. {peak.max().item():.3e}, uniform would be {1 / G ** 3:.3e}")
        img = torch.from_numpy(np.stack([frame] * B)).to(dev)
        d = torch.from_numpy(np.stack([depth] * B)).to(dev)
        j = kp.double()
        scale = (1.0 / peak.double()).contiguous()
        packed = torch.empty(_lib.render_volume_packed_elems(B, G), device=dev, dtype=torch.float32)
        zbuf, out, over = r._buffers(B)
        r.render(d, img, j, view=view)                       # fills the z-buffer the occluded view march reads
        r.overlay(img, j, depth=d)
        _lib.render_volume_pack(vol, packed)
        one = 1 << 9
        steps = [("se_render_volume_pack_f32", lambda: _lib.render_volume_pack(vol, packed))]
        for tag, mask in (("all joints", _lib.RENDER_VOLUME_ALL), ("one joint", one)):
            for occ, zb, dd in (("occluded", zbuf, d), ("open", None, None)):
                steps.append((f"se_render_volume_view_f64, {tag}, {occ}",
                              lambda mask=mask, zb=zb: _lib.render_volume_view(packed, scale, r.pinhole, view, zb, out, G, side, near=NEAR,
                                                                               joint_mask=mask)))
                steps.append((f"se_render_volume_overlay_f64, {tag}, {occ}",
                              lambda mask=mask, dd=dd: _lib.render_volume_overlay(packed, scale, r.ray_tab, over, G, side, depth=dd,
                                                                                  near=NEAR, joint_mask=mask)))
        steps += [("render() + overlay()", lambda: (r.render(d, img, j, view=view), r.overlay(img, j, depth=d))),
                  ("render_volumes() + overlay_volumes()",
                   lambda: (r.render_volumes(d, img, j, vol, side, view=view), r.overlay_volumes(img, j, vol, side, depth=d))),
                  ("forward (graph replay)", forward)]
        for name, fn in steps:
            med, lo = timed(fn, args.warmup, args.iters)
            lines.append(f"{B:>2} {name:<52} {med:10.1f} {lo:10.1f} {med / B:10.1f}")
        lines.append("")
    lines += ["The marches draw in place, so the timed calls composite over their own previous output: the work per call does not depend "
              "on the base picture.  render_volumes() + overlay_volumes() contain render() + overlay(), the default scale (torch: nan_to_num "
              "and amax over the volumes), two pack passes and the two marches; the PNG / JPEG encoding comes on top and is not timed here."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
