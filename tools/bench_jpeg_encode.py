#!/usr/bin/env python3
"""Cost of the device JPEG encoder (csrc/jpeg_enc.hip) against the host paths it replaces, on the rendered views of the demo frame:
the 720 x 960 third-person view and the 1024 x 1280 overlay, at B = 1 and 8.

  * se_jpeg_encode_u8 alone: HIP events, warm, median of --iters (>= 20) calls;
  * JpegEncoder.encode, read-back of the compressed bytes and file assembly included: wall clock around a synchronised call;
  * PIL's save(format="PNG") (what --render_dir does at the parent commit, the device-to-host copy of the raw image not included)
    and save(format="JPEG") of the same frames, on one host core in the same run;
  * run_sequence.py frames/s on a synthetic sequence: no rendering, --render_dir with PNG at --render_every 1, and --render_video.

    python tools/bench_jpeg_encode.py [--iters 30] [--sequence_frames 256] [--out profiles/jpeg_encode_cost.txt]
"""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sceneego_amd import _lib, load_config, synth                      # noqa: E402
from sceneego_amd.config import resolve_calibration_path              # noqa: E402
from sceneego_amd.jpeg_encode import JpegEncoder, quant_tables        # noqa: E402
from sceneego_amd.render import SceneRenderer                         # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def timed_events(fn, warmup, iters):
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


def timed_wall(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us), min(us)


def pil_save(rgb, fmt, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format=fmt, **kw)
    return b.tell()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host_iters", type=int, default=5, help="timed calls of the PIL saves (tens of milliseconds each)")
    ap.add_argument("--sequence_frames", type=int, default=256, help="0 skips the run_sequence.py part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_cost.txt"))
    args = ap.parse_args(argv)
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode.py needs an MI355X (HIP device)")
    from sceneego_amd.preprocess import load_depth, load_image_bgr
    torch.set_num_threads(1)
    dev = torch.device("cuda")
    cfg = load_config()
    frame = torch.from_numpy(load_image_bgr(os.path.join(GOLD, "demo", "img_001000.jpg")))[None].to(dev)
    depth = torch.from_numpy(load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr")))[None].to(dev)
    joints = torch.from_numpy(np.load(os.path.join(GOLD, "demo_exr_b1.npz"))["joints"][:1]).to(dev)
    r = SceneRenderer(resolve_calibration_path(cfg.dataset.camera_calibration_path), device=dev)
    views = {"render 720x960": r.render(depth, frame, joints).clone(), "overlay 1024x1280": r.overlay(frame, joints, depth=depth).clone()}
    enc = JpegEncoder(dev)
    lines = [f"JPEG encoder cost, {torch.cuda.get_device_name(0)}; rendered views of the demo frame; quality 90; device kernels: HIP "
             f"events, {args.warmup} warm-up + {args.iters} timed calls; encode(): wall clock of a synchronised call, same counts; PIL "
             f"{__import__('PIL').__version__} on one host core, 1 warm-up + {args.host_iters} timed calls; median (minimum); library "
             f"{_lib.built_fingerprint()}", "",
             f"{'view':<18} {'B':>2} {'path':<38} {'us/call':>11} {'(min)':>11} {'us/frame':>11} {'bytes/frame':>12}"]
    for name, img in views.items():
        host = img[0].cpu().numpy()
        for B in (1, 8):
            batch = img.expand(B, -1, -1, -1).contiguous()
            for sub in ("444", "420"):
                ql, qc = quant_tables(90)
                med, lo = timed_events(lambda: enc.launch(batch, ql, qc, sub), args.warmup, args.iters)
                size = len(enc.encode(batch, subsampling=sub)[0])
                lines.append(f"{name:<18} {B:>2} {'se_jpeg_encode_u8 ' + sub:<38} {med:11.1f} {lo:11.1f} {med / B:11.1f} {size:12d}")
                med, lo = timed_wall(lambda: enc.encode(batch, subsampling=sub), args.warmup, args.iters)
                lines.append(f"{name:<18} {B:>2} {'JpegEncoder.encode ' + sub + ' (with read-back)':<38} {med:11.1f} {lo:11.1f} {med / B:11.1f} {size:12d}")
            med, lo = timed_wall(lambda: batch.cpu(), 1, args.host_iters)
            lines.append(f"{name:<18} {B:>2} {'raw frames to the host (.cpu())':<38} {med:11.1f} {lo:11.1f} {med / B:11.1f} {host.nbytes:12d}")
        for label, fmt, kw in (("PIL save PNG", "PNG", {}), ("PIL save JPEG 444", "JPEG", {"quality": 90, "subsampling": 0}),
                               ("PIL save JPEG 420", "JPEG", {"quality": 90, "subsampling": 2})):
            size = pil_save(host, fmt, **kw)
            med, lo = timed_wall(lambda: pil_save(host, fmt, **kw), 1, args.host_iters)
            lines.append(f"{name:<18} {1:>2} {label + ' (host, one core)':<38} {med:11.1f} {lo:11.1f} {med:11.1f} {size:12d}")
        print("\n".join(lines[-9:]), flush=True)
    if args.sequence_frames > 0:
        import contextlib

        import run_sequence
        n = args.sequence_frames
        depths = [os.path.join(GOLD, "demo", f) for f in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
        lines += ["", f"run_sequence.py on a synthetic sequence of {n} frames (batch {cfg.test.batch_size}, --weights synthetic, one stream), frames/s:"]
        with tempfile.TemporaryDirectory() as tmp:
            synth.make_sequence(os.path.join(tmp, "seq"), "bench", n, depths, estimated_depth_name="est_depth", seed=5)
            common = ["--root_dir", os.path.join(tmp, "seq"), "--seq_name", "bench", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
            forms = (("no rendering", []),
                     ("--render_dir, PNG, --render_every 1", ["--render_dir", os.path.join(tmp, "png")]),
                     ("--render_dir, --render_format jpg", ["--render_dir", os.path.join(tmp, "jpg"), "--render_format", "jpg"]),
                     ("--render_video (4:2:0, quality 90)", ["--render_video", os.path.join(tmp, "seq.avi")]))
            for label, extra in forms:
                with contextlib.redirect_stdout(io.StringIO()):
                    res = run_sequence.main(common + extra)
                lines.append(f"  {label:<40} {res['fps']:8.2f}")
                print(lines[-1], flush=True)
            lines.append(f"  AVI of {n} frames: {os.path.getsize(os.path.join(tmp, 'seq.avi')) / 1e6:.1f} MB; PNG directory: "
                         f"{sum(os.path.getsize(os.path.join(tmp, 'png', f)) for f in os.listdir(os.path.join(tmp, 'png'))) / 1e6:.1f} MB")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
