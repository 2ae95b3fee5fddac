"""Per-block float64 parity of the whole V2V program over the batch / grid routes it can take.

``v2v_route`` picks, block by block, the kernel (``conv3d_variant``: 0 direct / split-K, 1 1-D F(4,3), 2 F(4,3) x F(2,3),
3 F(4,3) x F(4,3) ping-pong) and the hand-over layout (channels-last, quad-planar, octet-planar) from the batch and the level size.
The kernel tests check each kernel alone; this module checks what the program composes from them.  A recorder wraps
``_front0_fft`` / ``_conv`` (front layer), ``_res``, ``_up`` and ``run`` with ``monkeypatch`` and keeps, for the checked samples,
every block output (reference network/v2v.py ``front0..3``, ``skip1..5``, ``enc1..5``, ``mid``, ``dec1..5``, ``back0``, logits)
together with the layout the call wrote it in and the pooled tensor of the blocks that pool from their epilogue.  Each tap is
compared with a float64 evaluation of its block (the oracle's ``_basic3d`` / ``_res3d`` / ``_up3d`` on a float64 state dict) fed
the HIP's own input tap, at the kernel tests' bar 2e-5 * max|ref|; the pooled tensors must equal ``max_pool3d`` of their block's
output bit for bit; the logits of the whole chain are compared with a float64 oracle run on the same input at 1e-4 * max.
"""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import sceneego_oracle as O
from sceneego_amd import _lib, load_config, synth
from sceneego_amd.v2v import V2VProgram

from conftest import synthetic_state_dict

DEV = "cuda:0"
TAP_TOL = 2e-5          # max|hip - ref| <= TAP_TOL * max|ref| per block (the bar of tests/test_gpu_kernels.py)
# Regression gates per kernel family, of max|ref| (5x the largest value measured on MI355X over the matrix, rounded up to one digit):
GATE_WINO44 = 2e-5      # blocks with a convolution on the F(4,3) x F(4,3) kernel (variant 3): measured 3.6e-6 (enc1 at 64^3, G=128)
GATE_OTHER = 5e-6       # the other 3x3x3 blocks (variants 0 / 1 / 2) and the decoder taps: measured 8.1e-7 (enc2, octet, 32^3)
GATE_POINTWISE = 2e-6   # the frequency-domain front layer and the fused 1x1x1 tail: measured 2.9e-7 / 3.0e-7
LOGIT_TOL = 1e-4        # whole chain against the float64 oracle (the bar of test_v2v_stagewise_vs_oracle)
P = "volume_net"
E = P + ".encoder_decoder"

torch.set_num_threads(min(16, torch.get_num_threads()))


# ------------------------------------------------------------------------------------------------
# float64 references (CPU)
# ------------------------------------------------------------------------------------------------
_IM2COL_BYTES = 1 << 30


def _conv3d_slabs(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
    """F.conv3d in output z-slabs when the float64 im2col of the whole volume would exceed 1 GiB (7^3 x 33 channels at 64^3: 24 GB).
    Same operator on each slab; below the limit it IS F.conv3d."""
    k = w.shape[2]
    D = x.shape[2]
    per_plane = x.shape[1] * k ** 3 * x.shape[3] * x.shape[4] * x.element_size()
    if stride != 1 or groups != 1 or dilation != 1 or per_plane * D <= _IM2COL_BYTES:
        return F.conv3d(x, w, b, stride, padding, dilation, groups)
    p = padding if isinstance(padding, int) else padding[0]
    xp = F.pad(x, (0, 0, 0, 0, p, p))
    S = max(1, _IM2COL_BYTES // per_plane)
    return torch.cat([F.conv3d(xp[:, :, z:z + S + 2 * p], w, b, padding=(0, p, p)) for z in range(0, D, S)], dim=2)


# the oracle's block functions with the slab convolution (every other operator unchanged)
_F64 = types.SimpleNamespace(**{n: getattr(F, n) for n in dir(F) if not n.startswith("__")})
_F64.conv3d = _conv3d_slabs


@pytest.fixture()
def oracle64(monkeypatch):
    monkeypatch.setattr(O, "F", _F64)
    return O


_SD64 = {}


def _sd64():
    if not _SD64:
        _SD64.update({k: (v.double() if v.is_floating_point() else v) for k, v in synthetic_state_dict(False).items()})
    return _SD64


def _crop(t, box, halo, D):
    """t [n,C,D,D,D]; box ((z0,z1),(y0,y1),(x0,x1)) or None (whole volume).  Returns the box grown by ``halo`` and clipped to the
    volume - the volume's own boundary keeps the zero padding of the reference - and the box's offsets inside it."""
    if box is None:
        return t, None
    lo = [max(0, a - halo) for a, _ in box]
    hi = [min(D, b + halo) for _, b in box]
    c = t[:, :, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    return c, tuple((a - l, b - l) for (a, b), l in zip(box, lo))


def _inner(t, off):
    if off is None:
        return t
    (z0, z1), (y0, y1), (x0, x1) = off
    return t[:, :, z0:z1, y0:y1, x0:x1]


def _half(box):
    return None if box is None else tuple((a // 2, b // 2) for a, b in box)


TOP = ("front0", "front1", "front2", "front3", "skip1", "dec1", "back0", "logits")      # the taps at the G^3 level


def block_refs(sd, tap, x, G, box=None, lower=True, scale=1.0):
    """float64 reference of every tap, each block computed from the HIP's own input tap.  ``tap(name, box=None)``: the HIP tap as
    float64 NCDHW, cropped to ``box`` when one is given.  ``box``: output region of the G^3-level taps (None: all of it), computed on
    the box plus the block's receptive-field halo; ``lower``: also the levels below G^3, always whole.  ``scale``: the logits'
    volume_multiplier."""
    ref = {}

    def top(name, fn, src, halo):
        c, off = _crop(src, box, halo, G)
        ref[name] = _inner(fn(c), off)

    top("front0", lambda c: O._basic3d(sd, P + ".front_layers.0", c), x, 3)
    for i in (1, 2, 3):
        top(f"front{i}", lambda c, i=i: O._res3d(sd, f"{P}.front_layers.{i}", c), tap(f"front{i - 1}"), 2)
    top("skip1", lambda c: O._res3d(sd, E + ".skip_res1", c), tap("front3"), 2)
    if lower:
        prev = tap("front3")
        for k in range(1, 6):
            ref[f"enc{k}"] = O._res3d(sd, f"{E}.encoder_res{k}", F.max_pool3d(prev, 2, 2))
            if k < 5:
                ref[f"skip{k + 1}"] = O._res3d(sd, f"{E}.skip_res{k + 1}", tap(f"enc{k}"))
            prev = tap(f"enc{k}")
        ref["mid"] = O._res3d(sd, E + ".mid_res", tap("enc5"))
        for k in range(5, 1, -1):
            src = tap("mid") if k == 5 else tap(f"dec{k + 1}")
            ref[f"dec{k}"] = O._up3d(sd, f"{E}.decoder_upsample{k}", O._res3d(sd, f"{E}.decoder_res{k}", src)) + tap(f"skip{k}")
    # dec1 on the box: the 2x upsample of the half-size region of decoder_res1(dec2), which needs a 2-voxel halo at G/2
    c, off = _crop(tap("dec2"), _half(box), 2, G // 2)
    r = _inner(O._res3d(sd, E + ".decoder_res1", c), off)
    ref["dec1"] = O._up3d(sd, E + ".decoder_upsample1", r) + tap("skip1", box)
    top("back0", lambda c: O._res3d(sd, P + ".back_layers.0", c), tap("dec1"), 2)
    ref["logits"] = tail_ref(sd, tap("back0", box)) * scale
    return ref


def tail_ref(sd, back0):
    """back_layers.1 / .2 and output_layer (three 1x1x1 layers, reference network/v2v.py:155-161)."""
    x = O._basic3d(sd, P + ".back_layers.1", back0)
    x = O._basic3d(sd, P + ".back_layers.2", x)
    return F.conv3d(x, sd[P + ".output_layer.weight"], sd[P + ".output_layer.bias"])


# ------------------------------------------------------------------------------------------------
# the recorder (test side only: monkeypatch on V2VProgram)
# ------------------------------------------------------------------------------------------------
def _to_ncdhw(t, lay, D, C):
    """A tap of n samples in its hand-over layout -> [n, C, D, D, D].  The planar layouts live in [B,D,D,D,C]-shaped tensors too."""
    n = t.shape[0]
    if lay in ("quad", "oct"):
        w = 4 if lay == "quad" else 8
        return t.reshape(n, C // w, D, D, D, w).permute(0, 1, 5, 2, 3, 4).reshape(n, C, D, D, D)
    return t.reshape(n, D, D, D, C).permute(0, 4, 1, 2, 3)


class Recorder:
    def __init__(self, monkeypatch, sel):
        self.sel = list(sel)
        self.taps = {}          # name -> (tensor [n,C,D,D,D] float32 on the device, layout, variants)
        self.x = None
        self.scaled = None
        self.names = {}
        rec = self
        orig_res, orig_up, orig_fft, orig_conv, orig_run = (V2VProgram._res, V2VProgram._up, V2VProgram._front0_fft,
                                                            V2VProgram._conv, V2VProgram.run)

        def _res(prog, x, blk, r, B, pool_out=None):
            out = orig_res(prog, x, blk, r, B, pool_out=pool_out)
            name = rec._name(prog, blk)
            rec._put(name, out, r.lay_out, r.dim, r.cout, r.variants)       # layout and kernels: the route entry the executor was given
            if pool_out is not None:
                rec._put(name + ".pool", pool_out, None, r.dim // 2, r.cout, r.variants)
            return out

        def _up(prog, x, pc, skip, B, dim, flags):
            out = orig_up(prog, x, pc, skip, B, dim, flags)
            rec._put(rec._name(prog, pc), out, "quad" if flags & _lib.OUT_QUAD else None, 2 * dim, pc.cout, ())
            return out

        def _front0_fft(prog, x, B, G, flags):
            out = orig_fft(prog, x, B, G, flags)
            rec._put("front0", out, "quad" if flags & _lib.OUT_QUAD else None, G, prog.front0.cout, ("fft",))
            return out

        def _conv(prog, x, pc, B, dim, flags, residual=None, out=None, pool_out=None):
            out = orig_conv(prog, x, pc, B, dim, flags, residual=residual, out=out, pool_out=pool_out)
            if pc is prog.front0:
                rec._put("front0", out, None, dim, pc.cout, (_lib.conv3d_variant(B, dim, pc.cin_pad, pc.cout, pc.k, 0),))
            return out

        def run(prog, x, B, G, out=None, softargmax=None, scaled=False, planar1=False):
            rec.x_raw, rec.scaled, rec.fused = x, scaled, softargmax is not None
            if planar1:
                xin = x[rec.sel]
            elif x.dim() == 6:      # triplet-planar [B, ceil(cin/3), G, G, G, 3]
                xin = x[rec.sel].permute(0, 1, 5, 2, 3, 4).reshape(len(rec.sel), -1, G, G, G)[:, :prog.cin]
            else:
                xin = x[rec.sel].permute(0, 4, 1, 2, 3)[:, :prog.cin]
            rec.x = xin.clone()
            lg = orig_run(prog, x, B, G, out=out, softargmax=softargmax, scaled=scaled, planar1=planar1)
            rec._put("logits", lg, "planar", G, prog.cout, ())
            return lg

        for n, f in (("_res", _res), ("_up", _up), ("_front0_fft", _front0_fft), ("_conv", _conv), ("run", run)):
            monkeypatch.setattr(V2VProgram, n, f)

    def _name(self, prog, obj):
        if not self.names:
            m = {id(b): f"front{i + 1}" for i, b in enumerate(prog.front_res)}
            for k in range(5):
                m[id(prog.skip[k])] = f"skip{k + 1}"
                m[id(prog.enc[k])] = f"enc{k + 1}"
                m[id(prog.dec[k])] = f"decres{k + 1}"       # decoder_res{k}: its output goes straight into the deconvolution
                m[id(prog.up[k])] = f"dec{k + 1}"
            m[id(prog.mid)] = "mid"
            m[id(prog.back_res)] = "back0"
            self.names = m
        return self.names[id(obj)]

    def _put(self, name, t, lay, D, C, var):
        if name.startswith("decres"):
            self.taps[name] = (None, lay, var)        # layout and kernel only: the reference chains it into dec{k}
            return
        s = t[self.sel]
        if lay == "planar":
            s = s.reshape(len(self.sel), C, D, D, D)
        else:
            s = _to_ncdhw(s, lay, D, C)
        self.taps[name] = (s.clone(), lay or "cl", var)


# ------------------------------------------------------------------------------------------------
# one matrix point
# ------------------------------------------------------------------------------------------------
_NETS = {}
SEEN = {"variants": set(), "layouts": set(), "points": set()}


def _net(G):
    if G not in _NETS:
        from sceneego_amd.voxel_net_depth import VoxelNetwork_depth
        _NETS.clear()
        cfg = load_config()
        cfg.model.volume_size = G
        net = VoxelNetwork_depth(cfg, device="cpu", verbose=False)
        net.load_state_dict(synthetic_state_dict(False), strict=True)
        _NETS[G] = net.to(DEV).eval()
    return _NETS[G]


def _boxes(G):
    """Four 16^3 output boxes of a G^3 level: a corner, an edge, a face and the centre (z, y, x ranges)."""
    e, c = G - 16, G // 2 - 8
    r = lambda a: (a, a + 16)
    return {"corner": (r(e), r(e), r(e)), "edge": (r(0), r(0), r(c)), "face": (r(c), r(c), r(0)), "centre": (r(c), r(c), r(c))}


def check_point(rec, G, B, label, oracle, box_top=False, chained=True):
    """Compare every recorded tap of ``rec`` (filled by one forward) with its block-isolated float64 reference."""
    sd = _sd64()
    scale = float(_NETS[G].volume_net.program.output_scale) if rec.scaled else 1.0
    torch.cuda.synchronize()
    lines, fails = [], []
    for name, (t, lay, var) in rec.taps.items():
        if t is not None:
            assert not bool(torch.isnan(t).any()), f"{label}: NaN in tap {name} ({lay}, variants {var})"
        SEEN["layouts"].add(lay)
        SEEN["variants"].update(v for v in var if isinstance(v, int))
    # pooled tensors: bit for bit max_pool3d of the block's own full-resolution output (float32, on the device)
    for name, (t, lay, var) in list(rec.taps.items()):
        if name.endswith(".pool"):
            want = F.max_pool3d(rec.taps[name[:-5]][0], 2, 2)
            assert torch.equal(t, want), f"{label}: pooled tensor of {name[:-5]} ({var}) differs from max_pool3d of its output: " \
                                         f"{float((t - want).abs().max()):.3e}"
    for s in range(len(rec.sel)):
        def tap(name, box=None):
            t = rec.taps[name][0][s:s + 1]
            if box is not None and box != "full":
                (z0, z1), (y0, y1), (x0, x1) = box
                t = t[:, :, z0:z1, y0:y1, x0:x1]
            return t.double().cpu()
        x = rec.x[s:s + 1].double().cpu()
        boxes = list(_boxes(G).items()) if box_top else [(None, None)]
        for bi, (bname, box) in enumerate(boxes):
            refs = block_refs(sd, tap, x, G, box=box, lower=bi == 0, scale=scale)
            for name, ref in refs.items():
                got = tap(name, box if name in TOP else None)
                err = float((got - ref).abs().max())
                mx = float(ref.abs().max())
                lay, var = rec.taps[name][1], rec.taps[name][2]
                where = f"sample {rec.sel[s]}" + (f" {bname}" if box is not None and name in TOP else "")
                lines.append(f"{name:7s} {where:16s} {lay:6s} {str(var):8s} {err:.2e} / {mx:.2e} = {err / max(mx, 1e-30):.1e}")
                if not err <= min(TAP_TOL, _gate(name, rec.taps)) * mx:
                    fails.append(f"{label} tap {name} ({where}, layout {lay}, conv3d_variant {var}): max|d| {err:.3e} > "
                                 f"{min(TAP_TOL, _gate(name, rec.taps))} * {mx:.3e}")
        if chained:
            want = oracle.v2v(sd, x) * scale
            got = tap("logits")
            err, mx = float((got - want).abs().max()), float(want.abs().max())
            lines.append(f"chained logits sample {rec.sel[s]}: {err:.2e} / {mx:.2e} = {err / mx:.1e}")
            if not err <= LOGIT_TOL * mx:
                fails.append(f"{label} chained logits sample {rec.sel[s]}: {err:.3e} > {LOGIT_TOL} * {mx:.3e}")
    print(f"\n[{label}]\n" + "\n".join(lines))
    SEEN["points"].add(label)
    assert not fails, "\n".join(fails)


def _gate(name, taps):
    if name in ("front0", "logits"):
        return GATE_POINTWISE
    var = taps[name][2] + (taps["decres" + name[3:]][2] if name.startswith("dec") else ())
    return GATE_WINO44 if 3 in var else GATE_OTHER


def _forward_point(monkeypatch, G, B, sel, seed):
    net = _net(G)
    img, depth = synth.make_inputs(seed, B, "floor" if seed % 2 else "uniform")
    rec = Recorder(monkeypatch, sel)
    with torch.no_grad():
        net(img.to(DEV), net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth.to(DEV))
    torch.cuda.synchronize()
    xb = [t for k, t in net._xbuf.items() if k[0] == B]
    assert xb and rec.x_raw is xb[0] and rec.x_raw.dim() == 5, "the forward did not take the planar1 production input"
    assert rec.fused, "the forward did not take the fused soft-argmax tail"
    return rec


# Route matrix (G, B, checked samples).  Which kernel / layout each level takes follows se_conv3d_f32_variant,
# se_conv3d_wino44pp_shape (units = B * (D/16) * (D/8)^2 * cout/32 against the CU count, or D >= 64), se_conv3d_small_volume
# (B * D^3 <= 4096), the 2048..8192-voxel window of the split-K kernels and sceneego_amd.v2v.v2v_route.
ROUTES = [
    # G=64: 64^3 quad everywhere; 32^3 octet (64 units < 256 CUs); 16^3 channels-last split-K (4096 voxels) + halo; 8^3 grid split-K
    pytest.param(64, 1, (0,), id="G64-B1"),
    # 32^3 octet (128 units); 16^3 octet (8192 voxels > 4096); 8^3 in-workgroup split-K (1024 voxels)
    pytest.param(64, 2, (1,), id="G64-B2"),
    # 32^3 quad (4 * 2*4*4 * 2 = 256 units = CU count: the first batch on the ping-pong kernel); 8^3 LDS-halo tiles (2048 voxels)
    pytest.param(64, 4, (3,), id="G64-B4"),
    # the headline batch: 32^3 quad, 16^3 octet, 8^3 halo (4096 voxels), 4^3 / 2^3 split-K
    pytest.param(64, 8, (0, 7), id="G64-B8"),
    # more than 32 samples: the persistent kernels slice the batch into launches of 32, the FFT front layer walks 8+8+8+8+2
    pytest.param(64, 34, (33,), id="G64-B34"),
    # G=32: the middle block at 1^3; 32^3 top level octet at B=1 (64 units)
    pytest.param(32, 1, (0,), id="G32-B1"),
    # ... and quad at B=8 (512 units); 16^3 octet, 8^3 halo, 2^3 and 1^3 split-K / direct
    pytest.param(32, 8, (0, 7), id="G32-B8"),
    # G=96: 48 / 24 / 12 / 6 / 3; 24^3 is the production route onto the 1-D F(4,3) kernel (algo 1); 3^3 is odd for conv, deconv, pool
    pytest.param(96, 1, (0,), id="G96-B1"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("G,B,sel", ROUTES)
def test_v2v_blocks_vs_float64(G, B, sel, monkeypatch, oracle64):
    rec = _forward_point(monkeypatch, G, B, sel, seed=1000 + 10 * G + B)
    check_point(rec, G, B, f"G{G} B{B}", oracle64)


@pytest.mark.gpu
def test_v2v_blocks_vs_float64_g128_boxes(monkeypatch, oracle64):
    """BASELINE configs[4]'s 128^3 grid, B=1: the 128^3-level taps on four 16^3 output boxes (each against a float64 reference on the
    box plus its receptive-field halo cropped from the input tap), every level below whole.  No chained float64 run: it would need
    the full 128^3 network in float64 on the host (the golden case b1_g128_floor checks the whole forward)."""
    rec = _forward_point(monkeypatch, 128, 1, (0,), seed=1128)
    check_point(rec, 128, 1, "G128 B1", oracle64, box_top=True, chained=False)


@pytest.mark.gpu
def test_v2v_model_forward_dense_input_vs_float64(monkeypatch, oracle64):
    """The drop-in path: ``V2VModel.forward`` on a dense NCDHW input (planar front layer input as it stands, un-fused tail with
    unscaled logits), B=2 at 64^3, the last sample."""
    net = _net(64)
    x = torch.randn(2, 33, 64, 64, 64, generator=torch.Generator().manual_seed(77))
    x[:, 32] = (x[:, 32] > 1.0).float()         # an occupancy-like channel
    rec = Recorder(monkeypatch, (1,))
    with torch.no_grad():
        lg = net.volume_net(x.to(DEV))
    assert not rec.fused and not rec.scaled
    assert torch.equal(rec.x.cpu(), x[1:2])
    assert torch.equal(lg[1:2].cpu(), rec.taps["logits"][0].cpu())
    check_point(rec, 64, 2, "V2VModel.forward G64 B2", oracle64)


@pytest.mark.gpu
def test_route_matrix_coverage():
    """The matrix above must reach every kernel family and every hand-over layout: a routing change that empties a route fails here
    instead of silently shrinking what the module checks."""
    want = {f"G{p.values[0]} B{p.values[1]}" for p in ROUTES} | {"G128 B1", "V2VModel.forward G64 B2"}
    if not want <= SEEN["points"]:
        pytest.skip("coverage is asserted over the whole matrix; run the module without a selection")
    assert {0, 1, 2, 3} <= SEEN["variants"], SEEN["variants"]
    assert {"quad", "oct", "cl"} <= SEEN["layouts"], SEEN["layouts"]


# ------------------------------------------------------------------------------------------------
# CPU self-check of the reference side
# ------------------------------------------------------------------------------------------------
def test_block_references_reproduce_oracle_taps(oracle64):
    """At G=32, B=1: the block-isolated references, fed the oracle's own float64 taps, reproduce ``O.v2v(..., taps=)`` exactly on the
    whole volume and to rounding on the four 16^3 boxes (same operators on a smaller region); the slab convolution equals F.conv3d."""
    sd = _sd64()
    G = 32
    x = torch.randn(1, 33, G, G, G, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    taps = {}
    O.v2v(sd, x, taps=taps)

    def tap(name, box=None):
        t = taps[name]
        if box is not None:
            (z0, z1), (y0, y1), (x0, x1) = box
            t = t[:, :, z0:z1, y0:y1, x0:x1]
        return t

    names = {f"front{i}" for i in range(4)} | {f"{n}{k}" for n in ("skip", "enc", "dec") for k in range(1, 6)} | {"mid", "back0", "logits"}
    refs = block_refs(sd, tap, x, G)
    assert set(refs) == names
    for name, ref in refs.items():
        assert torch.equal(ref, taps[name]), (name, float((ref - taps[name]).abs().max()))
    for bname, box in _boxes(G).items():
        refs = block_refs(sd, tap, x, G, box=box, lower=False)
        assert set(refs) == set(TOP)
        for name, ref in refs.items():
            want = tap(name, box)
            assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max()), (name, bname)
    # the slab form of the convolution (the 7^3 layer at 64^3 and above) against the plain operator
    w = sd[P + ".front_layers.0.block.0.weight"]
    xs = torch.randn(1, 33, 24, 20, 20, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    global _IM2COL_BYTES
    keep = _IM2COL_BYTES
    try:
        _IM2COL_BYTES = 1 << 22
        got = _conv3d_slabs(xs, w, None, padding=3)
    finally:
        _IM2COL_BYTES = keep
    want = F.conv3d(xs, w, None, padding=3)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
