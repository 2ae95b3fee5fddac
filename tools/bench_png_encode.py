#!/usr/bin/env python3
"""Cost of the device PNG encoder (csrc/png_enc.hip) against PIL's PNG writer, which --render_dir uses by default, and beside the
device JPEG encoder, on the rendered views of the demo frame: the 720 x 960 third-person view and the 1024 x 1280 overlay, B = 1 and 8.

  * se_png_encode_u8 alone (its four kernels): HIP events, warm, median of --iters (>= 20) calls; the kernels one by one from
    `rocprofv3 --kernel-trace --stats` over a child process per view and batch size that only launches the encoder
    (`--kernels_only VIEW:B`; `--no_trace` skips them);
  * PngEncoder.encode, read-back of the compressed bytes, chunk CRCs and file assembly included: wall clock around a synchronised
    call; the host part (zlib.crc32 and the chunk assembly on the bytes that came back) also on its own;
  * se_jpeg_encode_u8 / JpegEncoder.encode (quality 90, 4:4:4) on the same frames;
  * PIL's save(format="PNG") of the same pixels on one host core in the same run, the copy of the raw image to the host not included;
  * file sizes against PIL's on the third-person view, the overlay (photo content) and a volume view;
  * run_sequence.py frames/s on a synthetic sequence: no rendering, --render_dir with --png_encoder host and with --png_encoder device.

    python tools/bench_png_encode.py [--iters 30] [--sequence_frames 256] [--out profiles/png_encode_cost.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_jpeg_encode import GOLD, pil_save, timed_events, timed_wall    # noqa: E402
from sceneego_amd import _lib, load_config, synth                        # noqa: E402
from sceneego_amd.config import resolve_calibration_path                # noqa: E402
from sceneego_amd.jpeg_encode import JpegEncoder, quant_tables          # noqa: E402
from sceneego_amd.png_encode import PngEncoder, png_file                # noqa: E402
from sceneego_amd.render import SceneRenderer                           # noqa: E402


def blob_volumes(grid, device, seed=0):
    """float32 [1,15,G,G,G]: one normalised Gaussian blob per joint, enough to put colour ramps into the volume views."""
    g = torch.Generator().manual_seed(seed)
    centre = (torch.rand((15, 3), generator=g) * 0.5 + 0.25) * grid
    ax = torch.arange(grid, dtype=torch.float32)
    d2 = sum((ax.view(*[-1 if k == a else 1 for k in range(3)]) - centre[:, a].view(15, 1, 1, 1)) ** 2 for a in range(3))
    v = torch.exp(-d2 / (2 * 2.5 ** 2))
    return (v / v.sum(dim=(1, 2, 3), keepdim=True))[None].contiguous().to(device)


def kernel_trace(view, batch, warmup, iters):
    """The png_* rows of rocprofv3's kernel statistics over warm-up + iters calls of one view and batch size, in a child process of
    its own: (header, rows) as the tool wrote them, or (None, [why])."""
    import glob
    import shutil
    import subprocess
    if shutil.which("rocprofv3") is None:
        return None, ["rocprofv3 is not on the PATH"]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "png", "--", sys.executable, os.path.abspath(__file__),
               "--kernels_only", f"{view}:{batch}", "--warmup", str(warmup), "--iters", str(iters)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if done.returncode != 0 or not found:
            return None, [f"rocprofv3 ended with {done.returncode}, statistics file: {found}"] + done.stdout.splitlines()[-3:]
        with open(found[0]) as f:
            rows = f.read().splitlines()
    return rows[0], [r for r in rows[1:] if "png_" in r]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host_iters", type=int, default=5, help="timed calls of the PIL saves (tens of milliseconds each)")
    ap.add_argument("--sequence_frames", type=int, default=256, help="0 skips the run_sequence.py part")
    ap.add_argument("--kernels_only", default=None, metavar="VIEW:B",
                    help="only launch se_png_encode_u8 on that view and batch size, warm-up + iters times (what the kernel trace runs)")
    ap.add_argument("--no_trace", action="store_true", help="skip the rocprofv3 kernel traces")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode_cost.txt"))
    args = ap.parse_args(argv)
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_encode.py needs an MI355X (HIP device)")
    from sceneego_amd.preprocess import load_depth, load_image_bgr
    torch.set_num_threads(1)
    dev = torch.device("cuda")
    cfg = load_config()
    frame = torch.from_numpy(load_image_bgr(os.path.join(GOLD, "demo", "img_001000.jpg")))[None].to(dev)
    depth = torch.from_numpy(load_depth(os.path.join(GOLD, "demo", "img_001000.jpg.exr")))[None].to(dev)
    joints = torch.from_numpy(np.load(os.path.join(GOLD, "demo_exr_b1.npz"))["joints"][:1]).to(dev)
    r = SceneRenderer(resolve_calibration_path(cfg.dataset.camera_calibration_path), device=dev)
    views = {"render 720x960": r.render(depth, frame, joints).clone(), "overlay 1024x1280": r.overlay(frame, joints, depth=depth).clone()}
    png, jpg = PngEncoder(dev), JpegEncoder(dev)
    if args.kernels_only:
        view, B = args.kernels_only.rsplit(":", 1)
        batch = views[view].expand(int(B), -1, -1, -1).contiguous()
        for _ in range(args.warmup + args.iters):
            png.launch(batch)
        torch.cuda.synchronize()
        return
    lines = [f"PNG encoder cost, {torch.cuda.get_device_name(0)}; rendered views of the demo frame; device calls: HIP events, "
             f"{args.warmup} warm-up + {args.iters} timed calls; encode(): wall clock of a synchronised call, same counts; PIL "
             f"{__import__('PIL').__version__} on one host core, 1 warm-up + {args.host_iters} timed calls; median (minimum); library "
             f"{_lib.built_fingerprint()}", "",
             f"{'view':<18} {'B':>2} {'path':<44} {'us/call':>11} {'(min)':>11} {'us/frame':>11} {'bytes/frame':>12}"]
    ql, qc = quant_tables(90)
    for name, img in views.items():
        host = img[0].cpu().numpy()
        H, W = host.shape[:2]
        for B in (1, 8):
            batch = img.expand(B, -1, -1, -1).contiguous()
            rows = []
            files = png.encode(batch)
            size = len(files[0])
            idat = [f[41:-16] for f in files]                     # signature 8 + IHDR 25 + IDAT header 8 ... CRC 4 + IEND 12
            rows.append(("se_png_encode_u8 (4 kernels)",) + timed_events(lambda: png.launch(batch), args.warmup, args.iters) + (size,))
            rows.append(("PngEncoder.encode (read-back, CRC, file)",) + timed_wall(lambda: png.encode(batch), args.warmup, args.iters) + (size,))
            rows.append(("  host part: zlib.crc32 of the IDAT",) + timed_wall(lambda: [zlib.crc32(d) for d in idat], args.warmup, args.iters) + (size,))
            rows.append(("  host part: chunks around it (with CRC)",) + timed_wall(lambda: [png_file(H, W, 3, d) for d in idat], args.warmup, args.iters) + (size,))
            jsize = len(jpg.encode(batch)[0])
            rows.append(("se_jpeg_encode_u8 444 q90",) + timed_events(lambda: jpg.launch(batch, ql, qc, "444"), args.warmup, args.iters) + (jsize,))
            rows.append(("JpegEncoder.encode 444 q90 (read-back)",) + timed_wall(lambda: jpg.encode(batch), args.warmup, args.iters) + (jsize,))
            rows.append(("raw frames to the host (.cpu())",) + timed_wall(lambda: batch.cpu(), 1, args.host_iters) + (host.nbytes,))
            for label, med, lo, nbytes in rows:
                lines.append(f"{name:<18} {B:>2} {label:<44} {med:11.1f} {lo:11.1f} {med / B:11.1f} {nbytes:12d}")
            lines.append(f"{name:<18} {B:>2} the host CRC is {100 * rows[2][1] / rows[1][1]:.0f} % of encode(), the kernels {100 * rows[0][1] / rows[1][1]:.0f} %")
        size = pil_save(host, "PNG")
        med, lo = timed_wall(lambda: pil_save(host, "PNG"), 1, args.host_iters)
        lines.append(f"{name:<18} {1:>2} {'PIL save PNG (host, one core)':<44} {med:11.1f} {lo:11.1f} {med:11.1f} {size:12d}")
        print("\n".join(lines[-15:]), flush=True)
    # file sizes, the volume views included
    vol = blob_volumes(cfg.model.volume_size if hasattr(cfg.model, "volume_size") else 64, dev)
    pictures = dict(views)
    pictures["volumes.render 720x960"] = r.render_volumes(depth, frame, joints, vol, 2.0).clone()
    pictures["volumes.overlay 1024x1280"] = r.overlay_volumes(frame, joints, vol, 2.0, depth=depth).clone()
    lines += ["", f"{'file sizes':<28} {'device PNG':>12} {'PIL PNG':>12} {'ratio':>7} {'raw':>12}"]
    for name, img in pictures.items():
        host = img[0].cpu().numpy()
        mine, pil = len(png.encode(img.contiguous())[0]), pil_save(host, "PNG")
        lines.append(f"{name:<28} {mine:12d} {pil:12d} {mine / pil:7.3f} {host.nbytes:12d}")
    print("\n".join(lines[-5:]), flush=True)
    if not args.no_trace:
        lines += ["", f"the kernels one by one: rocprofv3 --kernel-trace --stats over {args.warmup + args.iters} calls of se_png_encode_u8 "
                      f"(the first, cold call included), one child process per row group; durations in ns"]
        for name in views:
            for B in (1, 8):
                head, rows = kernel_trace(name, B, args.warmup, args.iters)
                lines.append(f"{name}, B = {B}:" + ("" if head is None else "  " + head))
                lines += ["  " + r for r in rows]
                print("\n".join(lines[-1 - len(rows):]), flush=True)
    if args.sequence_frames > 0:
        import run_sequence
        n = args.sequence_frames
        depths = [os.path.join(GOLD, "demo", f) for f in ("img_001000.jpg.exr", "img_001796.jpg.exr", "img_002376.jpg.exr")]
        lines += ["", f"run_sequence.py on a synthetic sequence of {n} frames (batch {cfg.test.batch_size}, --weights synthetic, one stream), "
                      f"--render_every 1, frames/s:"]
        with tempfile.TemporaryDirectory() as tmp:
            synth.make_sequence(os.path.join(tmp, "seq"), "bench", n, depths, estimated_depth_name="est_depth", seed=5)
            common = ["--root_dir", os.path.join(tmp, "seq"), "--seq_name", "bench", "--estimated_depth_name", "est_depth", "--weights", "synthetic"]
            forms = (("no rendering", []),
                     ("--render_dir, --png_encoder host (PIL)", ["--render_dir", os.path.join(tmp, "host")]),
                     ("--render_dir, --png_encoder device", ["--render_dir", os.path.join(tmp, "device"), "--png_encoder", "device"]),
                     ("--render_dir, --render_format jpg", ["--render_dir", os.path.join(tmp, "jpg"), "--render_format", "jpg"]))
            with contextlib.redirect_stdout(io.StringIO()):
                run_sequence.main(common)               # once untimed: the first call of a process pays library load and graph capture
            for label, extra in forms:
                with contextlib.redirect_stdout(io.StringIO()):
                    res = run_sequence.main(common + extra)
                lines.append(f"  {label:<44} {res['fps']:8.2f}")
                print(lines[-1], flush=True)
            mb = {d: sum(os.path.getsize(os.path.join(tmp, d, f)) for f in os.listdir(os.path.join(tmp, d))) / 1e6 for d in ("host", "device", "jpg")}
            lines.append(f"  directories of {n} frame pairs: PIL PNG {mb['host']:.1f} MB, device PNG {mb['device']:.1f} MB, JPEG {mb['jpg']:.1f} MB")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
