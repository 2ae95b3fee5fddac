#!/usr/bin/env python3
"""Depth-map decode, host (sceneego_amd/exr.py) against device (exr_device.decode_depth_exr_batch), on the three demo maps
(tests/golden/demo, 640x512 HALF PIZ), and the end-to-end frames/s of run_sequence.py with either decoder.

    python tools/bench_exr_decode.py [--compression piz zip zips none] [--batches 1 8 32] [--reps 20] [--sequence 256]
                                     [--out result.json]

--compression: the demo maps as they are (piz, the default) and/or re-encoded at run time by the test-side writer
(tests/exr_zip_cases.py: zlib level 6, 16-line ZIP / 1-line ZIPS chunks, or NONE); lines of a re-encoded set carry "compression".

host:    wall clock of read_depth_exr over the batch's files, one core, one pass per file after one warm-up pass.
device:  HIP events around one call (pack + one H2D copy + both kernels + the status read-back), after warm-up; the host-side
         share of a call (parse, validate, pack) is timed separately on the wall clock with the launch stubbed out.
end-to-end: run_sequence.py on a generated sequence of --sequence frames (synthetic weights, config batch size), once per decoder
         after a short warm-up run.  --sequence 0 skips it (e.g. under rocprofv3 --kernel-trace --stats).
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

from sceneego_amd import _lib, exr, exr_device  # noqa: E402

DEMO = [os.path.join(ROOT, "tests", "golden", "demo", n + ".jpg.exr") for n in ("img_001000", "img_001796", "img_002376")]


def _read(src):
    return exr.read_depth_exr(src) if isinstance(src, str) else exr.depth_channel(exr.read_exr_buffer(src))


def host_ms(files):
    for p in files[:3]:
        _read(p)
    t0 = time.perf_counter()
    for p in files:
        _read(p)
    return (time.perf_counter() - t0) * 1e3


def device_ms(files, reps):
    out = torch.empty((len(files), 512, 640), device="cuda")
    for _ in range(3):
        exr_device.decode_depth_exr_batch(files, "cuda", out=out, clamp=None)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        exr_device.decode_depth_exr_batch(files, "cuda", out=out, clamp=None)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def host_side_ms(files, reps):
    real = _lib.exr_piz_decode, _lib.exr_zip_decode
    _lib.exr_piz_decode = _lib.exr_zip_decode = lambda *a, **k: None
    try:
        out = torch.empty((len(files), 512, 640), device="cuda")
        exr_device.decode_depth_exr_batch(files, "cuda", out=out, check=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            exr_device.decode_depth_exr_batch(files, "cuda", out=out, check=False)
        return (time.perf_counter() - t0) * 1e3 / reps
    finally:
        _lib.exr_piz_decode, _lib.exr_zip_decode = real


def sources(comp):
    """The three demo maps in compression `comp` (paths for piz, file bytes otherwise)."""
    if comp == "piz":
        return DEMO
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import exr_zip_cases
    return [exr_zip_cases.reencode(p, comp) for p in DEMO]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--compression", nargs="+", default=["piz"], choices=("piz", "zip", "zips", "none"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sequence", type=int, default=256, help="frames of the end-to-end run (0: skip)")
    ap.add_argument("--out", default=None, help="also write the results as a JSON list")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_exr_decode.py needs a HIP device")
    results = []

    def emit(r):
        results.append(r)
        print(json.dumps(r), flush=True)

    for comp in args.compression:
        demo = sources(comp)
        tag = {} if comp == "piz" else {"compression": comp}
        for B in args.batches:
            files = [demo[i % 3] for i in range(B)]
            h = host_ms(files)
            med, best = device_ms(files, args.reps)
            hs = host_side_ms(files, args.reps)
            emit({"what": "decode", **tag, "batch": B, "host_ms": round(h, 3), "host_ms_per_frame": round(h / B, 3),
                  "device_ms_median": round(med, 3), "device_ms_min": round(best, 3),
                  "device_host_side_ms_per_frame": round(hs / B, 4), "speedup": round(h / med, 1)})
        if args.sequence > 0:
            import run_sequence
            from sceneego_amd import synth
            with tempfile.TemporaryDirectory() as tmp:
                paths = []
                for i, d in enumerate(demo):
                    if isinstance(d, str):
                        paths.append(d)
                        continue
                    paths.append(os.path.join(tmp, f"demo{i}.exr"))
                    with open(paths[-1], "wb") as f:
                        f.write(d)
                synth.make_sequence(tmp, "seq", args.sequence, paths, estimated_depth_name="est_depth")
                synth.make_sequence(tmp, "warm", 16, paths, estimated_depth_name="est_depth")
                for decode in ("host", "device"):
                    common = ["--root_dir", tmp, "--estimated_depth_name", "est_depth", "--weights", "synthetic", "--depth_decode",
                              decode]
                    run_sequence.main(common + ["--seq_name", "warm"])
                    r = run_sequence.main(common + ["--seq_name", "seq"])
                    emit({"what": "run_sequence", **tag, "depth_decode": decode, "frames": r["frames"], "fps": round(r["fps"], 2)})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
