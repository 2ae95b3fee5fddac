#!/usr/bin/env python3
"""Image decode, host (preprocess.load_image_bgr, PIL) against device (jpeg_device.decode_jpeg_batch), on the committed demo frame
(tests/golden/demo/img_001000.jpg, 1280x1024 4:2:0), and the end-to-end frames/s of run_sequence.py with either image decoder.

    python tools/bench_jpeg_decode.py [--batches 1 8 32] [--reps 20] [--sequence 256] [--out result.json]

host:       wall clock of load_image_bgr per frame, one core, after one warm-up pass.
device:     HIP events around one call on already parsed files (pack + one H2D copy + the kernels + the status read-back), after
            warm-up; ``device_ms_with_parse`` is the same call from file bytes.
host parse: wall clock of the host side per frame (marker parse, tables, unstuffing, packing into the pinned buffer layout).
end-to-end: run_sequence.py on a generated sequence of --sequence frames (synthetic weights, config batch size, depth decoded on the
            device), once per image decoder after a short warm-up run.  --sequence 0 skips it (e.g. under rocprofv3
            --kernel-trace --stats).
Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sceneego_amd import jpeg_device  # noqa: E402
from sceneego_amd.preprocess import load_image_bgr  # noqa: E402

FRAME = os.path.join(ROOT, "tests", "golden", "demo", "img_001000.jpg")
DEPTHS = [os.path.join(ROOT, "tests", "golden", "demo", n + ".jpg.exr") for n in ("img_001000", "img_001796", "img_002376")]


def host_ms_per_frame(reps):
    load_image_bgr(FRAME)
    t0 = time.perf_counter()
    for _ in range(reps):
        load_image_bgr(FRAME)
    return (time.perf_counter() - t0) * 1e3 / reps


def parse_ms_per_frame(data, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        f = jpeg_device.JpegFile(data)
        pk = jpeg_device.Packed([f])
        host = np.empty(pk.size(), dtype=np.uint8)
        pk.fill(host, 0)
    return (time.perf_counter() - t0) * 1e3 / reps


def device_ms(sources, reps):
    out = torch.empty((len(sources), 1024, 1280, 3), device="cuda", dtype=torch.uint8)
    for _ in range(3):
        jpeg_device.decode_jpeg_batch(sources, "cuda", out=out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        jpeg_device.decode_jpeg_batch(sources, "cuda", out=out)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sequence", type=int, default=256, help="frames of the end-to-end run (0: skip)")
    ap.add_argument("--out", default=None, help="also write the results as a JSON list")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode.py needs a HIP device")
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    with open(FRAME, "rb") as f:
        data = f.read()
    h = host_ms_per_frame(args.reps)
    p = parse_ms_per_frame(data, args.reps)
    emit({"what": "host", "load_image_bgr_ms_per_frame": round(h, 3), "device_path_host_parse_ms_per_frame": round(p, 3)})
    for B in args.batches:
        parsed = [jpeg_device.JpegFile(data, i) for i in range(B)]
        med, best = device_ms(parsed, args.reps)
        med_raw, _ = device_ms([data] * B, args.reps)
        emit({"what": "decode", "batch": B, "device_ms_median": round(med, 3), "device_ms_min": round(best, 3),
              "device_ms_with_parse": round(med_raw, 3), "host_ms": round(h * B, 3), "speedup": round(h * B / med, 1)})
    if args.sequence > 0:
        import run_sequence
        from sceneego_amd import synth
        with tempfile.TemporaryDirectory() as tmp:
            synth.make_sequence(tmp, "seq", args.sequence, DEPTHS, estimated_depth_name="est_depth")
            synth.make_sequence(tmp, "warm", 16, DEPTHS, estimated_depth_name="est_depth")
            for decode in ("host", "device"):
                common = ["--root_dir", tmp, "--estimated_depth_name", "est_depth", "--weights", "synthetic", "--image_decode", decode]
                run_sequence.main(common + ["--seq_name", "warm"])
                r = run_sequence.main(common + ["--seq_name", "seq"])
                emit({"what": "run_sequence", "image_decode": decode, "frames": r["frames"], "fps": round(r["fps"], 2)})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
