#!/usr/bin/env python3
"""Headline benchmark: frames/s of the full VoxelNetwork_depth forward (256x256 image + 1024x1280 depth -> 15x3 joints).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`.  For N > 1 the driver launches it under
torch.distributed.run, one rank per GPU (RCCL); when it is typed WITHOUT a launcher (`python bench.py --gpus 8`) the
script starts that launcher itself as a CHILD process — before anything touches the GPU — and exits with the child's
return code.  A rank whose WORLD_SIZE differs from --gpus exits non-zero: a 1-GPU number is never printed as an N-GPU line.

W untimed warm-up steps, then EXACTLY K steps bracketed by barrier + synchronize on both sides, MAX over ranks, rank 0
prints ONE JSON line.  A step = one forward over one batch of synthetic input already resident in HBM (+ the all-gather
of the joints when N > 1).  Weak scaling: every rank runs --batch frames (BASELINE.json configs[1]: batch 8, fp32, 64^3).
Nothing is recorded inside the timed region; per-launch and per-stage durations come from a SEPARATE short pass with HIP
events on the launch stream (SURVEY.md §8d "Timing").
Consecutive steps are issued round-robin on `--streams` HIP streams (default 3, sceneego_amd/pipeline.py): each step is still one
complete forward of --batch frames, the K steps are all inside the timed bracket, and (with --full) `extra.single_stream` reports
the same K steps issued on one stream beside the headline; `config.streams` says which form `value` is.

A plain run does only what the headline needs: set-up, W warm-up steps, the K timed steps, --dump-outputs if given, the line.
`--dump-outputs DIR` writes what the timed path handed back in its LAST timed step as float32 .npy files (dump_outputs below).
Everything else moves behind `--full` (off by default); the --no-* switches, --profile-steps, --dump-kernel-events and
--dump-launch-order refine a --full run.  With --full the line also carries step_ms, repeat_values, latency_ms, single_stream_value,
shard_check / allgather_us (N > 1) and the objects below:
  roofline     — dominant V2V kernel (3x3x3 conv 32->32 at 64^3, 9 launches/step), bound "mfma":
                 achieved = EXECUTED matrix-core FLOP per launch / mean launch duration, frac = achieved / 157.3 TFLOP/s
                 (<= 1); the Winograd saving over the direct convolution is reported separately as algorithmic_speedup.
                 "hbm" compares the algorithmic bytes of the launch with the rocprofv3 FETCH_SIZE/WRITE_SIZE counters of
                 the committed PMC pass (profiles/r04_pmc.json; counters cannot be read from inside this process).  The
                 record carries the ABI version and a hash of sceneego_amd/csrc it was taken on; when either differs from
                 this checkout `traffic` is null (a stale record is never printed).
                 "stage_ms" = backbone / gather / voxelise / v2v / softargmax (median over the profiling pass).
  cpu_baseline — the CPU oracle (oracle/sceneego_oracle.py: the reference's own ATen CPU ops) on this box's host cores,
                 B=1 and B=8, 1 warm-up + 3 timed forwards each, median (N = 1 only), on the SAME seeded frames the GPU ran.
  parity       — max |joint difference| (metres) between the output of the LAST timed step and the oracle's forward on the
                 same frames (rank 0's frames; float64 evaluation of the reference's soft-argmax formula as the
                 platform-stable gate, its float32 value beside it); the process exits with code 3 above `tol` = 1e-3.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense f32 MFMA peak = vector f32 peak
HBM_PEAK_GBS = 8000.0
# algorithmic work of V2V + soft-argmax per frame at 64^3 / 128^3, fp32
V2V_GFLOP_PER_FRAME = {64: 299.1, 128: 2393.0}
V2V_GB_PER_FRAME = {64: 1.372, 128: 10.98}
PMC_FILE = os.path.join(ROOT, "profiles", "r06_pmc.json")
JOINT_TOL = 1e-3               # BASELINE.json north_star: joints within 1e-3 m of the reference's CPU forward
# se_conv3d_f32_algo() -> (kernel name, executed MFMA FLOP / direct-convolution FLOP)
K3_ALGOS = {
    0: ("conv3d_tiled_kernel / conv3d_direct_kernel: direct implicit GEMM", 1.0),
    1: ("conv3d_k3_wino43pp_kernel: 1-D Winograd F(4,3) along z, ping-pong wave groups", 0.5),
    2: ("conv3d_k3_wino2d_kernel: 2-D Winograd F(4,3) x F(2,3) along z, y; register accumulators over all input channels", 1.0 / 3.0),
    3: ("conv3d_k3_wino44pp_kernel: 2-D Winograd F(4,3) x F(4,3) along z, y, ping-pong wave groups, LDS-DMA weight stream; register "
        "accumulators over all input channels", 0.25),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="frames per GPU per step (BASELINE configs[1]: 8)")
    ap.add_argument("--volume-size", type=int, default=64)
    ap.add_argument("--depth-kind", default="uniform", choices=["uniform", "floor"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-events", action="store_true", help="skip the separate per-launch / per-stage timing pass")
    ap.add_argument("--profile-steps", type=int, default=5, help="steps of the separate timing pass")
    ap.add_argument("--v2v-dtype", default="fp32", choices=["fp32", "bf16"],
                    help="fp32: BASELINE configs[1] (default, the headline); bf16: configs[2] (bf16 storage, f32 accumulate)")
    ap.add_argument("--backbone-dtype", default="fp32", choices=["fp32", "bf16"], help="MIOpen backbone precision (config 3: bf16)")
    ap.add_argument("--no-extras", action="store_true", help="skip the side measurement of BASELINE configs[2] (bf16, B=32)")
    ap.add_argument("--dump-kernel-events", action="store_true", help="per-shape launch times to stderr")
    ap.add_argument("--dump-launch-order", default="", help="write the launch keys of one profiled step, in issue order, to this JSON file")
    ap.add_argument("--graphs", action="store_true", help="replay the forward as a captured hipGraph")
    ap.add_argument("--streams", type=int, default=3,
                    help="consecutive steps are issued round-robin on this many HIP streams (sceneego_amd/pipeline.py: the 2-D backbone of "
                         "step i+1 runs in the gaps of step i); 1 = every step behind the previous one")
    ap.add_argument("--master-port", type=int, default=0, help="rendezvous port of the self-started launcher (0: torchrun --standalone binds a free one itself)")
    ap.add_argument("--no-repeats", action="store_true", help="skip the two repeat brackets that show the spread of the headline")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle comparison of the timed output (profiling runs)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline as well: repeat brackets, the single-stream run, per-step device times, the per-launch "
                         "timing pass and roofline, the oracle parity gate, the CPU baseline, the cross-rank shard check and the side "
                         "configurations (the --no-* switches above trim a --full run)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the outputs of the last timed step to DIR/<name>.npy (float32; outputs above DUMP_SAMPLE elements as a fixed sample)")
    args = ap.parse_args()
    if not args.full and (args.dump_kernel_events or args.dump_launch_order):
        ap.error("--dump-kernel-events and --dump-launch-order come from the per-launch timing pass: add --full")
    return args


def self_launch(args):
    """`python bench.py --gpus N` typed without a launcher: run N ranks as a child job and hand back its exit code.
    The parent has not imported torch and never touches the GPU; it does not exec."""
    # no pre-picked port (another process could take it between the probe and the bind): --standalone lets torchrun's own c10d
    # rendezvous bind port 0 and publish MASTER_PORT to the ranks; --master-port N keeps the explicit form
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}"]
    if args.master_port:
        cmd += ["--master-addr", "127.0.0.1", "--master-port", str(args.master_port)]
    else:
        cmd += ["--standalone", "--local-addr", "127.0.0.1"]
    cmd += [os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def build_network(volume_size, device):
    from sceneego_amd import load_config, synth
    from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
    cfg = load_config()
    cfg.model.volume_size = volume_size
    net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
    sd = synth.make_state_dict(net.state_dict(), seed=0)
    net.load_state_dict(sd, strict=True)
    return net.to(device).eval(), sd


def host_inputs(batch, rank, kind):
    """The seeded synthetic batch of this rank (BASELINE configs[1]: N(0,1) image, U(0.3,3) / floor-plane depth) from the portable
    counter-based generator (sceneego_amd/synth.py): the SAME frames are given to the GPU and, on rank 0, to the CPU oracle."""
    from sceneego_amd import synth
    return synth.make_inputs(1234 + rank, batch, kind)


def device_inputs(batch, rank, device, kind):
    img, depth = host_inputs(batch, rank, kind)
    return img.to(device), depth.to(device)


def effective_cores():
    """Host cores this process may really use: affinity mask, capped by the cgroup CPU quota if one is set."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period))))
    except (OSError, ValueError):
        pass
    return n


def pmc_record(batch, G, algo):
    """Counters of the dominant kernel from the committed rocprofv3 PMC passes (tools/pmc_round.py), or (None, why) when the
    record was taken for another shape / kernel family, on another ABI version or on other kernel sources than this checkout."""
    from sceneego_amd import _lib
    try:
        with open(PMC_FILE) as f:
            d = json.load(f)
    except (OSError, ValueError) as e:
        return None, f"{os.path.relpath(PMC_FILE, ROOT)} unreadable ({type(e).__name__})"
    if not (d.get("batch") == batch and d.get("volume_size") == G and d.get("algo") == algo):
        return None, "the committed counter record is for another batch / grid / kernel family"
    fp, built = _lib.source_fingerprint(), _lib.built_fingerprint()
    if built != fp:
        return None, f"libsceneego_hip.so was built from other sources (csrc {built}) than this checkout (csrc {fp}): rebuild"
    if d.get("abi_version") != _lib.ABI_VERSION or d.get("csrc_sha256_16") != fp:
        return None, (f"stale counter record: taken on ABI {d.get('abi_version')} / csrc {d.get('csrc_sha256_16')}, this build is "
                      f"ABI {_lib.ABI_VERSION} / csrc {fp}; re-run tools/pmc_round.py on the GPU box")
    return d, None


class _KeepLogits(dict):
    """taps sink for the oracle that retains only the V2V logits (the full tap set of a B=8 forward is several GB)."""

    def __setitem__(self, k, v):
        if k == "logits":
            super().__setitem__(k, v)


def oracle_reference(sd, volume_size, img, depth, timed):
    """The CPU oracle on the frames the GPU ran: joints of its forward (the reference's float32 soft-argmax, and the float64
    evaluation of the same formula from the same logits) and, when ``timed``, SURVEY.md §8d's CPU timing: B=1 and the whole batch,
    1 warm-up + 3 timed forwards each, median."""
    import torch
    from oracle import sceneego_oracle as O
    torch.set_num_threads(effective_cores())
    const = O.Constants(os.path.join(ROOT, "sceneego_amd", "calibration", "fisheye.calibration_05_08.json"), G=volume_size)
    taps = _KeepLogits()
    j32 = O.forward(sd, const, img, depth, taps=taps)[0]     # also the warm-up at the timed shape (oneDNN primitive creation)
    j64 = O.integrate(taps["logits"], const.coord, softmax=True, accumulate64=True)[0]
    taps.clear()
    if not timed:
        return j32, j64, None
    frames_all = img.shape[0]
    per_batch = {}
    stage = {}
    for frames in sorted({1, frames_all}):
        i, d = img[:frames], depth[:frames]
        if frames != frames_all:
            O.forward(sd, const, i, d)
        ts = []
        for _ in range(3):
            times = {}
            t0 = time.perf_counter()
            O.forward(sd, const, i, d, times=times)
            ts.append(time.perf_counter() - t0)
            stage = times
        med = statistics.median(ts)
        per_batch[f"b{frames}"] = {"frames_per_s": round(frames / med, 4), "median_s": round(med, 3),
                                   "runs_s": [round(t, 3) for t in ts]}
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            model = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), "")
    except OSError:
        pass
    top = per_batch[f"b{frames_all}"]
    base = {"value": top["frames_per_s"], "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle/sceneego_oracle.py forward at B=1 and B={frames_all} ({volume_size}^3, fp32) on the same seeded frames the GPU "
                      f"ran, 1 warm-up + 3 timed each, median; value = the B={frames_all} rate",
            "cpu": model, f"stage_seconds_b{frames_all}": {k: round(v, 3) for k, v in stage.items()}}
    base.update(per_batch)
    return j32, j64, base


K7_RATIO = {True: 12.0 / 42.0, False: 10.0 / 28.0}      # F(6,7) when dim % 16 == 0, else F(4,7): products per output and tap column
LAYOUT_BITS = 32 | 64 | 128 | 256 | 1024 | 2048 | 4096       # SE_IN_/OUT_/RES_OCTET | SE_EPI_SKIPCONV16 | SE_IN_/OUT_/RES_QUAD


def launch_flops(lib, key, flags, batch):
    """(direct-convolution FLOP, FLOP the matrix cores EXECUTE, kernel variant) of one profiled float32 V2V launch.
    Variant of a 3x3x3 launch = se_conv3d_f32_variant(batch, shape, the launch's own layout flags): every launch is priced at the
    ratio of the kernel it really ran on (position 62, channels-last 32 -> 32, runs on the 1/3 kernel)."""
    kind, k, cin, cout, dim = key
    vox = float(batch) * dim ** 3
    if kind == "conv3d":
        if k == 7:
            cin_real = 33 if cin == 48 else cin            # the V2V input buffer is padded to 48; the kernels walk 11 three-channel chunks
            direct = 2.0 * vox * 343 * cin_real * cout
            return direct, direct * K7_RATIO[dim % 16 == 0], 7
        if k == 3:
            fl = (flags or 0) & LAYOUT_BITS
            var = int(lib.se_conv3d_f32_variant(batch, dim, cin, cout, 3, fl))
            direct = 2.0 * vox * 27 * cin * cout
            ex = direct * K3_ALGOS.get(var, K3_ALGOS[0])[1]
            if fl & 256:                                    # fused 16-channel 1x1x1 skip convolution: executed as is
                direct += 2.0 * vox * 16 * cout
                ex += 2.0 * vox * 16 * cout
            return direct, ex, var
        direct = 2.0 * vox * cin * cout
        return direct, direct, 0
    if kind == "conv3d_fft":                                # the 7^3 front layer in the frequency domain (csrc/conv3d_fft7.hip): what the
        direct = 2.0 * vox * 343 * cin * cout               # matrix cores execute is pass 2, a real GEMM [M x 68] . [68 x 32] per frequency
        return direct, 2.0 * batch * (dim // 16) ** 3 * 68 * 32 * 7488, 70
    if kind == "deconv":                                    # k2s2 transposed convolution: 8 output voxels per input voxel
        direct = 2.0 * vox * 8 * cin * cout
        return direct, direct, 0
    if kind == "tail":                                      # back_layers.1, .2 (32 -> 32) + output_layer (32 -> 16 executed columns)
        direct = 2.0 * vox * (32 * 32 * 2 + 32 * cout)
        return direct, 2.0 * vox * (32 * 32 * 2 + 32 * 16), 0
    return 0.0, 0.0, -1


def timing_pass(step, steps):
    """Separate, untimed-for-the-headline pass: HIP events on the launch stream around every conv launch and every stage."""
    import torch
    from sceneego_amd import _lib
    with torch.no_grad():
        _lib.start_profile()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    return _lib.stop_profile()


def headline_line(args, world, G, bf16, n_streams, dt, rank_ms, world_backend):
    """The fields of the result line that a plain run prints: the headline bracket (K steps in dt seconds, max over ranks)."""
    frames = args.batch * world * args.steps
    line = {
        "metric": "frames/sec VoxelNetDepth forward (256x256 img+depth, 64^3 grid)" if G == 64 else
                  f"frames/sec VoxelNetDepth forward (256x256 img+depth, {G}^3 grid)",
        "value": round(frames / dt, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": ("bf16 storage + f32 accumulate (V2V), " + args.backbone_dtype + " backbone") if bf16 else
                 ("f32" if args.backbone_dtype == "fp32" else "f32 V2V, bf16 backbone"), "data": "synthetic",
        "config": {"workload": f"batch={args.batch}/GPU synthetic 256x256 image N(0,1) + {args.depth_kind} depth 1024x1280, "
                               f"{G}^3 grid, 15 joints, " + ("bf16 V2V (BASELINE configs[2])" if bf16 else "fp32 (BASELINE configs[1])"),
                   "batch_per_gpu": args.batch, "global_batch": args.batch * world, "volume_size": G,
                   "parallelism": f"dp{world}" + (" + RCCL all_gather of [B,15,3] joints" if world > 1 else ""),
                   "hipgraph": bool(args.graphs), "streams": n_streams},
    }
    if world > 1:
        line["rccl_ranks"] = world_backend
        line["rank_ms_per_step"] = [round(v, 4) for v in rank_ms]
    return line


DUMP_SAMPLE = 1 << 22      # elements written of a larger output: 16 MB of float32 per array, 48 MB for the three at most


def dump_outputs(path, outputs):
    """--dump-outputs: what a caller of the timed path receives from its last step, as float32 .npy files under ``path``:
    joints.npy [B*N,15,3] (all ranks' frames, gathered), features.npy [B,32,64,64] and volumes.npy (this rank's frames; the forward's
    second and third return values).  An output of more than DUMP_SAMPLE elements is written as a fixed sample, flattened: its flat
    range is cut into DUMP_SAMPLE equal strata and one element is taken from each at an offset drawn by numpy's default_rng(0), so
    the same arguments give the same positions in every run and every build."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    for name, t in zip(("joints", "features", "volumes"), outputs):
        t = t.detach()
        n = t.numel()
        if n > DUMP_SAMPLE:
            stride = n // DUMP_SAMPLE
            idx = np.arange(DUMP_SAMPLE, dtype=np.int64) * stride + np.random.default_rng(0).integers(0, stride, DUMP_SAMPLE)
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:               # checked before anything touches the GPU
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env}: refusing to print a {world_env}-GPU number as a "
              f"{args.gpus}-GPU line", file=sys.stderr)
        sys.exit(2)
    import torch
    from sceneego_amd import _lib, dist as sdist
    rank, world, device = sdist.init_from_env()
    assert world == args.gpus
    lib = _lib.load()
    net, sd = build_network(args.volume_size, device)
    img_h, depth_h = host_inputs(args.batch, rank, args.depth_kind)
    img, depth = img_h.to(device), depth_h.to(device)
    G = args.volume_size
    bf16 = args.v2v_dtype == "bf16"
    if bf16:
        net.set_v2v_dtype("bf16")
    if args.backbone_dtype == "bf16":
        net.set_backbone_dtype("bf16")
    if args.graphs:
        net.enable_graphs(True)

    n_streams = 1 if args.graphs else max(1, args.streams)
    pipe = None
    from sceneego_amd.pipeline import PipelinedForward
    if n_streams > 1:
        try:
            pipe = PipelinedForward(net, n_streams)
        except Exception as e:           # never lose the measurement to the throughput mode: fall back to one stream, say so
            print(f"bench.py: pipelined mode unavailable ({type(e).__name__}: {e}); running --streams 1", file=sys.stderr)
            pipe, n_streams = None, 1

    # a step returns (joints of every rank, this rank's features, this rank's volumes): what its caller receives (--dump-outputs)
    def step_single():
        out = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)
        return sdist.all_gather_joints(out[0]), out[1], out[2]

    def step():
        if pipe is None:
            return step_single()
        # the forward runs on one of the pipeline's streams; the (only) collective stays on the main stream, behind the forward's
        # event, so every rank issues its all-gathers in step order on one stream
        # inputs_ready=False: the resident inputs were complete before the loop; waiting for the main stream here would put step i+1
        # behind step i's all-gather, i.e. behind step i
        out, done = pipe(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth, inputs_ready=False)
        if world == 1:
            return out[0], out[1], out[2]    # nothing to gather; the caller synchronises the device before reading them
        PipelinedForward.hand_over(out[0], done)     # main stream waits for the forward; joints recorded on it for the collective
        return sdist.all_gather_joints(out[0]), out[1], out[2]

    with torch.no_grad():
        if pipe is not None:
            # set-up, not warm-up: every replica packs its kernels and lets MIOpen pick its solvers on its own stream once, so that
            # the W warm-up steps (which alternate between the replicas) never meet a cold one, whatever W is
            for _ in range(len(pipe)):
                pipe(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth, inputs_ready=False)
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            out = step()

        def timed(fn):
            """EXACTLY K steps between barrier + synchronize on both sides; max over ranks (and this rank's own wall time)."""
            torch.cuda.synchronize()
            sdist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                o = fn()
            torch.cuda.synchronize()
            sdist.barrier()
            torch.cuda.synchronize()
            mine = time.perf_counter() - t0
            return o, sdist.max_over_ranks(mine, device), mine

        last, dt, dt_mine = timed(step)                 # <- the headline
    out = last[0]
    rank_ms = sdist.gather_values(dt_mine / args.steps * 1e3, device)
    assert tuple(out.shape) == (args.batch * world, 15, 3) and bool(torch.isfinite(out).all())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)           # before any later forward (a replayed graph's outputs are static) overwrites them
    del last
    timed_joints = out[rank * args.batch:(rank + 1) * args.batch].detach().cpu()     # this rank's frames of the LAST timed step
    if not args.full:
        sdist.barrier()
        if rank == 0:
            print(json.dumps(headline_line(args, world, G, bf16, n_streams, dt, rank_ms, sdist.describe() if world > 1 else None)))
        return
    # spread: the same timed bracket twice more (reported beside the headline, never instead of it)
    repeats = []
    with torch.no_grad():
        for _ in range(0 if args.no_repeats else 2):
            repeats.append(timed(step)[1])
    # the same K steps with every step behind the previous one on ONE stream (reported beside the headline when it is pipelined)
    dt_single = None
    step_ms = None
    with torch.no_grad():
        if pipe is not None:
            step_single()
            dt_single = timed(step_single)[1]
        # per-step device time on the issuing stream (HIP events around each of K more single-stream steps; outside every timed bracket)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        torch.cuda.synchronize()
        for a, b in evs:
            a.record()
            step_single()
            b.record()
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in evs)
        step_ms = {"min": round(ts[0], 4), "median": round(statistics.median(ts), 4), "max": round(ts[-1], 4), "n": len(ts),
                   "what": "device time of K single-stream steps, HIP events on the issuing stream, separate pass behind the timed region"}

    # ---- N > 1: the gathered tensor really holds every rank's shard (frames are independent: a rank recomputes its right-hand
    # neighbour's frames locally and compares them with that neighbour's slice of the last timed all-gather) ----------------------
    shard_check = None
    if world > 1:
        peer = (rank + 1) % world
        pi, pd = device_inputs(args.batch, peer, device, args.depth_kind)
        with torch.no_grad():
            kp_peer = net(pi, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=pd)[0]
        torch.cuda.synchronize()
        d_peer = float((kp_peer - out[peer * args.batch:(peer + 1) * args.batch]).abs().max())
        d_peer = sdist.max_over_ranks(d_peer, device)
        shard_check = {"max_abs_diff_m": round(d_peer, 9), "tol": 2e-4 if not bf16 else 1e-1,
                       "checked": "every rank recomputed rank+1's frames and compared them with that rank's slice of the last timed "
                                  "all-gather (max over ranks; run-to-run noise of the MIOpen backbone is ~1e-5 m)"}
        del pi, pd, kp_peer
    prof = {}
    if not args.no_kernel_events:
        if args.graphs:
            net.enable_graphs(False)             # events cannot be recorded inside a replayed graph
        prof = timing_pass(step_single, args.profile_steps)
        if args.graphs:
            net.enable_graphs(True)
    sdist.barrier()
    world_backend = sdist.describe()
    if rank != 0:
        return
    psteps = args.profile_steps
    frames = args.batch * world * args.steps
    line = headline_line(args, world, G, bf16, n_streams, dt, rank_ms, world_backend)
    line["step_ms"] = step_ms
    if repeats:
        vals = [line["value"]] + [round(frames / r, 3) for r in repeats]
        line["repeat_values"] = {"values": vals, "min": min(vals), "max": max(vals),
                                 "what": "the headline bracket (first entry = `value`) and two more identical K-step brackets in the same process"}
    if world > 1:
        ag = [v for k, v in prof.items() if k[0] == "allgather"]
        if ag:
            line["allgather_us"] = {"median": round(statistics.median(ag[0]) * 1e3, 1), "max": round(max(ag[0]) * 1e3, 1), "n": len(ag[0]),
                                    "what": "HIP events on the issuing stream around all_gather_into_tensor([B/N,15,3]) in the separate "
                                            "timing pass, rank 0 (includes the wait for the slowest rank's forward)"}
    stage_ms = {k[1]: round(statistics.median(v), 4) for k, v in prof.items() if k[0] == "stage"}
    launches = {k: v for k, v in prof.items() if k[0] not in ("stage", "allgather")}
    conv_ms_per_step = sum(sum(v) for k, v in launches.items() if k[0].startswith("conv3d")) / psteps if launches else 0.0

    # ---- roofline of the dominant kernel (fp32 program) --------------------------------------------
    key = ("conv3d", 3, 32, 32, G)
    detail = [d for d in _lib.last_launch_detail if len(d[0]) == 5]
    if key in launches and not bf16:
        # every launch priced at the kernel it really ran on (its own layout flags)
        per_var = {}
        for k_, fl_, ms_ in detail:
            if k_ == key:
                d_, e_, v_ = launch_flops(lib, k_, fl_, args.batch)
                pv = per_var.setdefault(v_, {"launches": 0, "ms": 0.0, "direct": 0.0, "executed": 0.0})
                pv["launches"] += 1; pv["ms"] += ms_; pv["direct"] += d_; pv["executed"] += e_
        n_l = sum(v["launches"] for v in per_var.values())
        tot_ms = sum(v["ms"] for v in per_var.values())
        avg_ms = tot_ms / n_l
        direct_flop = sum(v["direct"] for v in per_var.values()) / n_l      # per launch (mean)
        exec_flop = sum(v["executed"] for v in per_var.values()) / n_l
        algo = max(per_var, key=lambda v: per_var[v]["launches"])           # the kernel most launches of the shape run on
        kname = "; ".join(f"{per_var[v]['launches'] // psteps} on {K3_ALGOS.get(v, K3_ALGOS[0])[0].split(':')[0]} "
                          f"({per_var[v]['ms'] / per_var[v]['launches']:.4f} ms, executed/direct {K3_ALGOS.get(v, K3_ALGOS[0])[1]:.3f})"
                          for v in sorted(per_var, key=lambda v: -per_var[v]["launches"]))
        ach = exec_flop / (avg_ms * 1e-3) / 1e12
        k7 = [v for k, v in launches.items() if k[0] in ("conv3d", "conv3d_fft") and k[1] == 7]
        k7_fft = [k for k in launches if k[0] == "conv3d_fft"]
        # algorithmic bytes of a launch: input read + output written once + the skip tensor where the launch has one (its own flags:
        # SE_EPI_RES_PRE_RELU = 2; the fused 16-channel skip convolution, 256, reads half a tensor), mean over the launches of the shape
        per_launch_bytes = [4.0 * args.batch * G ** 3 * (32 + 32 + (16 if (fl_ or 0) & 256 else 32 if (fl_ or 0) & 2 else 0))
                            for k_, fl_, _ in detail if k_ == key]
        alg_bytes = sum(per_launch_bytes) / len(per_launch_bytes)
        pmc, pmc_why = pmc_record(args.batch, G, algo)
        counter_bytes = pmc["hbm_bytes_per_launch"] if pmc else None
        # stage level: executed matrix-core FLOP of EVERY V2V launch of the pass (3^3, 7^3, 1^3, transposed, fused tail) / the stage time
        v2v_exec = sum(launch_flops(lib, k_, fl_, args.batch)[1] for k_, fl_, _ in detail) / psteps
        v2v_direct = sum(launch_flops(lib, k_, fl_, args.batch)[0] for k_, fl_, _ in detail) / psteps
        line["roofline"] = {
            "bound": "mfma", "achieved": round(ach, 2), "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / F32_MFMA_PEAK_TFLOPS, 4), "traffic": counter_bytes,
            # what this kernel STRUCTURE can reach (DESIGN.md section 4, round-5 finding 3): the float32 MFMA issues on
            # the vector ALUs, so a 4-channel step costs the SUM of its MFMA issue (6.9 k cycles per SIMD) and of the transform / epilogue
            # vector instructions beside it (~1.8 k) = 8.7 k cycles; the measured step takes 10.5 k at frac 0.557 -> 0.557 x 10.5 / 8.7
            "structural_frac": 0.67,
            "structural_frac_what": "ceiling of the F(4,3)xF(4,3) ping-pong structure on this pipe: the measured fraction scaled from the 10.5 k "
                                    "cycles a 4-channel step takes to the 8.7 k of its MFMA + vector-ALU issue (the float32 MFMA shares the "
                                    "vector ALUs: the two add up; 6.9 k of it is MFMA): 0.557 x 10.5 / 8.7.  Two rounds of issue-side experiments "
                                    "moved the kernel by layout only (profiles/r04_*, r05_*); round 6 left it alone (DESIGN.md section 6)",
            "kernel": f"conv3d 3x3x3 32->32 @{G}^3 f32, {n_l // psteps} launches/step on v_mfma_f32_16x16x4_f32: {kname}",
            "note": "achieved = EXECUTED matrix-core FLOP per launch / mean launch duration (HIP events on the launch stream, "
                    f"separate {psteps}-step pass outside the timed region), every launch priced at the kernel it ran on "
                    "(se_conv3d_f32_variant with the launch's layout flags); algorithmic_speedup = direct-convolution FLOP / executed FLOP",
            "algorithmic_speedup": round(direct_flop / exec_flop, 3),
            "algorithmic_tflops": round(direct_flop / (avg_ms * 1e-3) / 1e12, 2),
            "avg_launch_ms": round(avg_ms, 4), "executed_flop_per_launch": exec_flop, "direct_flop_per_launch": direct_flop,
            "per_kernel": {K3_ALGOS.get(v, K3_ALGOS[0])[0].split(":")[0]: {
                "launches_per_step": pv["launches"] // psteps, "avg_launch_ms": round(pv["ms"] / pv["launches"], 4),
                "executed_over_direct": round(pv["executed"] / pv["direct"], 4),
                "frac": round(pv["executed"] / (pv["ms"] * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4)} for v, pv in per_var.items()},
            "hbm": {"algorithmic_bytes": alg_bytes, "algorithmic_bytes_what": "mean over the launches of the shape: input + output, + the skip tensor "
                                                                                "for the launches that read one", "counter_bytes": counter_bytes,
                    "ratio": round(counter_bytes / alg_bytes, 3) if counter_bytes else None,
                    "algorithmic_gbs": round(alg_bytes / (avg_ms * 1e-3) / 1e9, 1),
                    "source": ("builder-side rocprofv3 pass, NOT measured in this run: " + os.path.relpath(PMC_FILE, ROOT) +
                               ": separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) on these kernel "
                               f"sources (csrc {pmc.get('csrc_sha256_16')}), " + pmc.get("correction", "")) if pmc else pmc_why,
                    "counters": {k: pmc.get(k) for k in ("fetch_kib_raw", "write_kib", "mfma_busy_cycles_per_launch", "mfma_pipe_busy_frac_of_launch",
                                                         "lds_bank_conflict_cycles", "lds_active_cycles")} if pmc else None},
            "stage": {"v2v_conv_ms_per_step": round(conv_ms_per_step, 3),
                      "v2v_tflops_algorithmic": round(V2V_GFLOP_PER_FRAME.get(G, 0) * args.batch / (conv_ms_per_step * 1e-3) / 1e3, 2)
                      if conv_ms_per_step else None,
                      "v2v_executed_gflop_per_step": round(v2v_exec / 1e9, 2), "v2v_direct_gflop_per_step": round(v2v_direct / 1e9, 2),
                      "v2v_executed_frac": round(v2v_exec / (stage_ms["v2v"] * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4)
                      if stage_ms.get("v2v") else None,
                      "v2v_executed_frac_what": "executed matrix-core FLOP of every V2V launch of the timing pass (3^3 at their kernels' ratios, "
                                                "7^3: the per-frequency GEMM of the frequency-domain form, or 12/42 on the Winograd kernel; 1^3 / transposed / fused tail "
                                                "as is) / stage_ms.v2v / the f32 MFMA peak",
                      "v2v_hbm_frac": round(V2V_GB_PER_FRAME.get(G, 0) * args.batch / (stage_ms["v2v"] * 1e-3) / HBM_PEAK_GBS, 4)
                      if stage_ms.get("v2v") else None,
                      "conv7_avg_ms": round(sum(k7[0]) / len(k7[0]), 4) if k7 else None},
        }
        if k7_fft and k7:
            # the frequency-domain front layer is three HBM-bound passes: bytes = input + spectra X (written, read) + Y (written, read) +
            # weight spectra + output (csrc/conv3d_fft7.hip header; tools/fft7_model.py prints the same model)
            m_tiles = args.batch * (G // 16) ** 3
            fbytes = 4.0 * args.batch * G ** 3 * (33 + 16) + 2.0 * m_tiles * (33 + 16) * 7488 * 8 + 7488 * 17 * 128 * 4.0
            f_ms = sum(k7[0]) / len(k7[0])
            line["roofline"]["front_layer"] = {
                "kernel": "7x7x7 33->16 in the frequency domain: fft7_fwd_kernel + fft7_gemm_kernel<33> + fft7_inv_kernel (one se_conv3d_k7_fft_f32 call)",
                "bound": "hbm", "avg_call_ms": round(f_ms, 4), "bytes_per_call": fbytes,
                "achieved_gbs": round(fbytes / (f_ms * 1e-3) / 1e9, 1), "frac": round(fbytes / (f_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "executed_gflop_per_call": round(2.0 * m_tiles * 68 * 32 * 7488 / 1e9, 2),
                "direct_gflop_per_call": round(2.0 * args.batch * G ** 3 * 343 * 33 * 16 / 1e9, 1),
                "what": "bytes = input + output + the float32 complex spectra X (33 ch) and Y (16 ch) of every 24^3 tile written once and read "
                        "once + the weight spectra; the F(6,7) Winograd kernel it replaces (SCENEEGO_FFT7=0) executed 217 GFLOP at B=8",
                "traffic": (pmc or {}).get("front_layer_fft", {}).get("hbm_bytes_per_call"),
                "traffic_what": "(2 * FETCH_SIZE + WRITE_SIZE) * 1024 summed over the three passes, from the same committed counter record as "
                                "roofline.traffic (null when the record is missing or was taken on other kernel sources)"}
    keyb = ("conv3d_bf16", 3, 32, 32, G)
    if keyb in launches:
        ms = launches[keyb]
        avg_ms = sum(ms) / len(ms)
        nbytes = 2.0 * args.batch * G ** 3 * (32 + 32)           # bf16 input + output records of one launch (skip reads excluded)
        flop = 2.0 * args.batch * G ** 3 * 27 * 32 * 32
        k7 = [v for k, v in launches.items() if k[1] == 7]
        line["roofline"] = {
            "bound": "hbm", "achieved": round(nbytes / (avg_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(nbytes / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "traffic": None,
            "kernel": f"conv3d 3x3x3 32->32 @{G}^3 bf16 storage (v_mfma_f32_16x16x32_bf16), {len(ms) // psteps} launches/step",
            "avg_launch_ms": round(avg_ms, 4), "bytes_per_launch": nbytes,
            "mfma_tflops": round(flop / (avg_ms * 1e-3) / 1e12, 1), "mfma_frac_of_2500": round(flop / (avg_ms * 1e-3) / 2.5e15, 4),
            "stage": {"v2v_conv_ms_per_step": round(conv_ms_per_step, 3),
                      "v2v_hbm_frac": round(0.5 * V2V_GB_PER_FRAME.get(G, 0) * args.batch / (conv_ms_per_step * 1e-3) / HBM_PEAK_GBS, 4),
                      "conv7_avg_ms": round(sum(k7[0]) / len(k7[0]), 4) if k7 else None},
        }
    if stage_ms:
        line.setdefault("roofline", {})["stage_ms"] = stage_ms
    if args.dump_launch_order and prof:
        order = _lib.last_launch_order[:len(_lib.last_launch_order) // psteps]
        with open(args.dump_launch_order, "w") as f:
            json.dump([list(k_) + [launch_flops(lib, k_, fl_, args.batch)[2] if k_[0] == "conv3d" else -1]
                       for k_, fl_, _ in _lib.last_launch_detail[:len(order)]], f)
    if args.dump_kernel_events:
        for k in sorted(launches, key=lambda k: -sum(launches[k])):
            v = launches[k]
            print(f"{str(k):44s} {len(v) // psteps:3d}/step avg {sum(v) / len(v):8.4f} ms  per-step {sum(v) / psteps:8.4f} ms",
                  file=sys.stderr)
    # ---- parity gate on the timed output + CPU baseline, same frames (rank 0's) -----------------------
    want_cpu = world == 1 and not args.no_cpu_baseline
    parity_ok = True
    j64 = None
    if not args.no_parity or want_cpu:
        nref = args.batch if G <= 64 else 1          # the oracle takes ~1 s per frame at 64^3 and ~10 s at 128^3
        j32, j64, base = oracle_reference(sd, G, img_h[:nref], depth_h[:nref], timed=want_cpu)
        if want_cpu:
            line["cpu_baseline"] = base
        if not args.no_parity:
            err64 = float((timed_joints[:nref] - j64).abs().max())
            err32 = float((timed_joints[:nref] - j32).abs().max())
            # the bf16-storage mode (BASELINE configs[2]) is specified to 4e-2 m, not to the reference tolerance
            tol = JOINT_TOL if not bf16 and args.backbone_dtype == "fp32" else 4e-2
            parity_ok = err64 <= tol and err32 <= tol
            line["parity"] = {
                "max_joint_err_m": round(err64, 9), "tol": tol, "pass": parity_ok, "frames": nref,
                "max_joint_err_vs_f32_softargmax_m": round(err32, 9),
                "oracle_f32_vs_f64_m": round(float((j32 - j64).abs().max()), 9),       # the CPU oracle's OWN float32 einsum noise on this host
                "checked": "joints of the LAST timed step (rank 0's frames) against oracle/sceneego_oracle.py on the same seeded frames; "
                           "BOTH comparisons are gated at tol: the oracle's own float32 output (the reference's CPU forward; its float32 "
                           "einsum over 262 144 voxels is reduction-order dependent across hosts, DESIGN.md 2) and the float64 evaluation "
                           "of the same soft-argmax formula on the oracle's logits (max_joint_err_m, the platform-stable figure); "
                           "oracle_f32_vs_f64_m = distance between those two evaluations of the SAME oracle logits, i.e. the part of "
                           "max_joint_err_vs_f32_softargmax_m that is the host's float32 summation order, not the HIP path"}
    if shard_check is not None:
        line["shard_check"] = shard_check
        parity_ok = parity_ok and shard_check["max_abs_diff_m"] <= shard_check["tol"]
    if world == 1 and not bf16 and args.backbone_dtype == "fp32" and G == 64 and not args.no_extras:
        line["extra"] = {"b1_f32": batch_extra(net, pipe, 1, rank, device, args.depth_kind, graphs=True),
                         "b32_f32": batch_extra(net, pipe, 32, rank, device, args.depth_kind, graphs=False),
                         "split_bf16_v2v_b8": split_extra(net, img, depth, timed_joints, j64),
                         "config3_bf16_b32": config3_extra(net, rank, device, args.depth_kind),
                         "config2_floor_depth_b8": floor_depth_extra(net, rank, device, args.batch),
                         "no_scene_v2v32_b8": no_scene_extra(device),
                         "config5_g128_b8": config5_extra(device, args.depth_kind)}
    if dt_single is not None:
        single = {
            "value": round(frames / dt_single, 3), "unit": "frames/s", "ms_per_step": round(dt_single / args.steps * 1e3, 4),
            "note": "the same K steps issued on ONE stream, every step behind the previous one (bench.py --streams 1); the headline "
                    "issues consecutive steps round-robin on `config.streams` streams (sceneego_amd/pipeline.py), each step still one "
                    "forward of `batch_per_gpu` frames"}
        line.setdefault("extra", {})["single_stream"] = single
        line["single_stream_value"] = single["value"]
        line["latency_ms"] = single["ms_per_step"]      # one forward alone on the chip; ms_per_step = timed wall / K with `streams` in flight
    else:
        line["latency_ms"] = line["ms_per_step"]
    print(json.dumps(line))
    if not parity_ok:
        print(f"bench.py: PARITY FAILED: parity {line.get('parity')} shard_check {line.get('shard_check')}", file=sys.stderr)
        sys.exit(3)


def config3_extra(net, rank, device, depth_kind):
    """BASELINE configs[2] measured beside the headline (never part of `value`): batch 32, bf16-storage V2V + bf16 backbone, with
    its own roofline (HBM bound: the bf16 3x3x3 kernel moves 2 B per element) and the measured joint distance to the float32 program
    on the same 32 frames."""
    import torch
    from sceneego_amd import _lib
    try:
        img, depth = device_inputs(32, rank, device, depth_kind)
        with torch.no_grad():
            kp32 = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)[0].float().cpu()
        net.set_v2v_dtype("bf16")
        net.set_backbone_dtype("bf16")
        with torch.no_grad():
            for _ in range(2):
                net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                kp = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)[0]
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 5
            diff = (kp.float().cpu() - kp32).abs().amax(dim=2).flatten()           # per joint: max over x, y, z
            _lib.start_profile()
            for _ in range(3):
                net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)
            torch.cuda.synchronize()
            prof = _lib.stop_profile()
        r = {"value": round(32 / dt, 1), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "batch": 32,
             "dtype": "bf16 storage + f32 accumulate (V2V), bf16 backbone",
             "joint_diff_to_f32_program_m": {"median": round(float(diff.median()), 6), "p95": round(float(diff.kthvalue(int(0.95 * diff.numel()))[0]), 6),
                                             "max": round(float(diff.max()), 6), "joints": int(diff.numel()),
                                             "spec": "over the 480 joints of a B=32 batch: median <= 1.5e-2 m, p95 <= 4e-2 m, max <= 0.15 m (what "
                                                     "tests/test_gpu_configs.py::test_config3_b32_bf16_accuracy gates; the 4e-2 m of DESIGN.md 4b is the bound on "
                                                     "the 45 golden joints, tests/test_gpu_bf16.py); bf16 storage does not meet the 1e-3 m parity tolerance",
                                             "pass": bool(float(diff.median()) <= 1.5e-2 and float(diff.kthvalue(int(0.95 * diff.numel()))[0]) <= 4e-2
                                                          and float(diff.max()) <= 0.15)},
             "note": "lower precision than the reference: reported beside the float32 headline, never in `value`"}
        ms = prof.get(("conv3d_bf16", 3, 32, 32, 64))
        if ms:
            avg = sum(ms) / len(ms)
            # bf16 input + output records of a launch, + the skip tensor for the launches that read one (flags of the profiled pass)
            det = [f for k, f, _ in _lib.last_launch_detail if k == ("conv3d_bf16", 3, 32, 32, 64)]
            skip = sum(1 for f in det if f is not None and f & (_lib.EPI_RES_PRE_RELU | _lib.EPI_RES_POST_RELU)) / max(1, len(det))
            nbytes = 2.0 * 32 * 64 ** 3 * (32 + 32 + 32 * skip)
            flop = 2.0 * 32 * 64 ** 3 * 27 * 32 * 32
            st = {k[1]: statistics.median(v) for k, v in prof.items() if k[0] == "stage"}
            r["roofline"] = {"bound": "hbm", "achieved": round(nbytes / (avg * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(nbytes / (avg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                             "kernel": f"conv3d 3x3x3 32->32 @64^3 bf16 storage (v_mfma_f32_16x16x32_bf16), B=32, {len(ms) // 3} launches/step",
                             "avg_launch_ms": round(avg, 4), "bytes_per_launch": nbytes, "launches_with_skip_tensor_frac": round(skip, 3),
                             "mfma_frac_of_2500": round(flop / (avg * 1e-3) / 2.5e15, 4),
                             "stage_ms": {k: round(v, 3) for k, v in st.items()},
                             "v2v_hbm_frac": round(0.5 * V2V_GB_PER_FRAME[64] * 32 / (st["v2v"] * 1e-3) / HBM_PEAK_GBS, 4) if st.get("v2v") else None}
        return r
    except Exception as e:      # never let the side measurement break the headline line
        return {"error": repr(e)[:200]}
    finally:
        net.set_v2v_dtype("fp32")
        net.set_backbone_dtype("fp32")


def _time_forward(net, img, depth, steps=5, warm=2):
    import torch
    with torch.no_grad():
        for _ in range(warm):
            net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
    assert bool(torch.isfinite(out[0]).all())
    return dt


def floor_depth_extra(net, rank, device, batch):
    """BASELINE configs[1]'s second variant (Config 2): the analytic floor-plane depth (realistic sparsity: ~4.6 k occupied voxels
    against ~137 k for iid-uniform depth) at the headline batch, one stream; joints against the uniform-depth forward are NOT comparable
    (different scene): parity of this input kind is tests/test_gpu_forward.py::test_forward_b1_floor_vs_golden."""
    import torch
    try:
        img, depth = device_inputs(batch, rank, device, "floor")
        dt = _time_forward(net, img, depth, steps=10)
        with torch.no_grad():
            occ = net.depth_map_to_voxel(depth)
        return {"value": round(batch / dt, 2), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "batch": batch, "dtype": "f32", "streams": 1,
                "occupied_voxels_per_frame": round(float(occ.sum()) / batch, 1),
                "note": "depth = 1.4 / ray_z clamped to 10 m (synth.make_inputs kind 'floor'), one stream, eager; compare extra.single_stream"}
    except Exception as e:
        return {"error": repr(e)[:200]}


def batch_extra(net, pipe, batch, rank, device, depth_kind, graphs):
    """north-star "batch 1/8/32": the float32 forward at another batch size beside the B=8 headline - one stream (eager), the same
    with hipGraph replay (B=1: the demo.py case, /root/reference/demo.py:23) and pipelined over the headline's streams."""
    import torch
    try:
        img, depth = device_inputs(batch, rank, device, depth_kind)
        steps = 20 if batch == 1 else 5
        dt = _time_forward(net, img, depth, steps=steps)
        r = {"value": round(batch / dt, 2), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "batch": batch, "dtype": "f32",
             "streams": 1, "note": "one stream, eager launches; `pipelined` = the headline's mode at this batch"}
        if graphs:
            net.enable_graphs(True)
            try:
                dtg = _time_forward(net, img, depth, steps=steps)
                r["hipgraph"] = {"value": round(batch / dtg, 2), "ms_per_step": round(dtg * 1e3, 3)}
            finally:
                net.enable_graphs(False)
        if pipe is not None:
            with torch.no_grad():
                for _ in range(2 * len(pipe)):
                    pipe(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth, inputs_ready=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps * 2):
                    pipe(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth, inputs_ready=False)
                torch.cuda.synchronize()
                dtp = (time.perf_counter() - t0) / (steps * 2)
            r["pipelined"] = {"value": round(batch / dtp, 2), "ms_per_step": round(dtp * 1e3, 3), "streams": len(pipe)}
            if graphs:
                # ... and with every replica's forward replayed as a captured hipGraph: at batch 1 the eager pipeline is bound by the
                # host's launch rate (~175 launches per frame from one Python thread), a replay is one call per frame
                for n in pipe.nets:
                    n.enable_graphs(True)
                try:
                    with torch.no_grad():
                        for _ in range(2 * len(pipe)):
                            pipe(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth, inputs_ready=False)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(steps * 3):
                            out_g, _ = pipe(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth, inputs_ready=False)
                        torch.cuda.synchronize()
                        dtg = (time.perf_counter() - t0) / (steps * 3)
                    kp_g = out_g[0].clone()
                    pipe.nets[0].enable_graphs(False)
                    with torch.no_grad():
                        kp_e = pipe.nets[0](img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)[0]
                    torch.cuda.synchronize()
                    r["pipelined_hipgraph"] = {"value": round(batch / dtg, 2), "ms_per_step": round(dtg * 1e3, 3), "streams": len(pipe),
                                               "max_joint_diff_to_eager_m": round(float((kp_g - kp_e).abs().max()), 9)}
                finally:
                    for n in pipe.nets:
                        n.enable_graphs(False)
        return r
    except Exception as e:      # never let the side measurement break the headline line
        return {"error": repr(e)[:200]}
    finally:
        torch.cuda.empty_cache()


def split_extra(net, img, depth, f32_joints, oracle_j64):
    """EXPERIMENTAL split-bf16 arithmetic for the 3x3x3 layers (float32 tensors; csrc/conv3d_split.hip), beside the headline: the same
    frames, one stream; joints against the float32 program of this run and against the oracle."""
    import torch
    try:
        net.set_v2v_dtype("split_bf16")
        dt = _time_forward(net, img, depth)
        with torch.no_grad():
            kp = net(img, net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth)[0].cpu()
        r = {"value": round(img.shape[0] / dt, 2), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "batch": int(img.shape[0]),
             "dtype": "f32 tensors, 3x3x3 layers as split-bf16 products (hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16, f32 accumulate)",
             "streams": 1, "max_joint_diff_to_f32_program_m": round(float((kp - f32_joints).abs().max()), 9),
             "note": "experimental; not the float32 headline.  tol 1e-3 m"}
        if oracle_j64 is not None:
            n = oracle_j64.shape[0]
            r["max_joint_err_vs_oracle_m"] = round(float((kp[:n] - oracle_j64).abs().max()), 9)
        return r
    except Exception as e:
        return {"error": repr(e)[:200]}
    finally:
        net.set_v2v_dtype("fp32")


def config5_extra(device, depth_kind):
    """BASELINE configs[4] measured beside the headline (never part of `value`): 128^3 grid, batch 8, float32, one stream."""
    import torch
    net = None
    try:
        net, _ = build_network(128, device)
        img, depth = device_inputs(8, 0, device, depth_kind)
        dt = _time_forward(net, img, depth)
        return {"value": round(8 / dt, 2), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "batch": 8, "volume_size": 128,
                "dtype": "f32", "streams": 1,
                "note": "same forward at volume_size 128 (8x the voxels); parity at this size: tests/test_gpu_configs.py::test_config5_g128_b8"}
    except Exception as e:      # never let the side measurement break the headline line
        return {"error": repr(e)[:200]}
    finally:
        del net
        torch.cuda.empty_cache()


def no_scene_extra(device):
    """The reference author's own micro-benchmark shape (network/v2v.py:259-270: V2VModel(32, 15) on [8,32,64,64,64]) as it occurs
    on this path: the `with_scene: False` network (network/voxel_net_depth.py:65-77), batch 8, float32, whole forward."""
    import torch
    net = None
    try:
        from sceneego_amd import load_config, synth
        from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
        cfg = load_config()
        cfg.model.with_scene = False
        net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
        net.load_state_dict(synth.make_state_dict(net.state_dict(), seed=0), strict=True)
        net = net.to(device).eval()
        img, _ = device_inputs(8, 0, device, "uniform")
        dt = _time_forward(net, img, None)
        return {"value": round(8 / dt, 2), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "batch": 8, "dtype": "f32",
                "streams": 1, "note": "with_scene False: V2VModel(32, 15) on the gathered [8,32,64^3] feature volume, no depth input"}
    except Exception as e:
        return {"error": repr(e)[:200]}
    finally:
        del net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
