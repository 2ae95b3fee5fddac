"""GPU: what ``V2VProgram.run`` composes in bf16 storage - octet-planar input, pad channels, strides, flag words - launch by launch.

A recorder (``monkeypatch`` on ``_lib.conv3d`` / ``deconv3d_k2s2`` / ``maxpool3d_2`` / ``pointwise_chain3``) keeps every launch of a bf16
forward of the whole network with the synthetic state dict: its input, skip and output tensors, the packed layer and the flag word
the program passed.  Each launch is then held to the float64 interval model (tests/bf16_launch_model.py) fed the launch's OWN input
tensors: reference weights are the program's own packed tensors read back through the kernels and held to the float64 fold of the
layer's modules (test_gpu_bf16_launches.check_packed), the bias is the packed layer's.  Pools must be exact.

Grids: G = 32 at B = 1 and B = 3 (the 32^3 launches on one sample at B = 3, everything below whole) and G = 96 at B = 1 (levels up
to 24^3 whole; the 48^3 and 96^3 launches on two 16^3 output boxes, one at the far corner and one interior across tile borders, each
against a reference on the box plus its halo, the volume's own border keeping its zero padding).  Each point runs with the fused
soft-argmax tail (the production forward) and without it (``run`` alone).  The bf16 forward is also held to the mode's
specification against the float32 program on the same inputs.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from sceneego_amd import _lib, load_config, synth
from sceneego_amd.v2v import V2VProgram

import bf16_launch_cases as C
import bf16_launch_model as M
from conftest import synthetic_state_dict
from test_gpu_bf16_launches import check_packed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
torch.set_num_threads(min(16, torch.get_num_threads()))
BOX_FROM = 48           # levels from this size on are checked on boxes
_NETS = {}
SEEN = {"kernels": set(), "points": set()}


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


def _boxes(D):
    if D < BOX_FROM:
        return [None]
    r = lambda a: (a, a + 16)
    return [(r(D - 16),) * 3, (r(D // 2 - 4), r(D // 2 - 12), r(D // 2 + 2))]


# ------------------------------------------------------------------------------------------------
# the recorder
# ------------------------------------------------------------------------------------------------
class Launches:
    def __init__(self, monkeypatch):
        self.items = []
        self.logits = []
        self.on = True          # off while the checks run: they launch kernels of their own (the weight read-back)
        rec = self
        conv3d, deconv, pool, chain, run = _lib.conv3d, _lib.deconv3d_k2s2, _lib.maxpool3d_2, _lib.pointwise_chain3, V2VProgram.run

        def w_conv3d(inp, wpack, bpack, residual, out, batch, dim, cin, cin_pad, cout, ksize, flags, workspace=None, pool_out=None):
            conv3d(inp, wpack, bpack, residual, out, batch, dim, cin, cin_pad, cout, ksize, flags, workspace, pool_out=pool_out)
            if rec.on and inp.dtype == BF:
                assert pool_out is None and workspace is None
                rec.items.append(dict(kind="conv", x=inp, w=wpack, b=bpack, res=residual, out=out, B=batch, dim=dim, cin=cin,
                                      cin_pad=cin_pad, cout=cout, k=ksize, flags=flags))

        def w_deconv(inp, wpack, bpack, residual, out, batch, dim, cin, cout, flags):
            deconv(inp, wpack, bpack, residual, out, batch, dim, cin, cout, flags)
            if rec.on and inp.dtype == BF:
                rec.items.append(dict(kind="deconv", x=inp, w=wpack, b=bpack, res=residual, out=out, B=batch, dim=dim, cin=cin,
                                      cin_pad=cin, cout=cout, k=2, flags=flags))

        def w_pool(inp, out, batch, dim, channels, in_octet=False):
            pool(inp, out, batch, dim, channels, in_octet=in_octet)
            if rec.on and inp.dtype == BF:
                rec.items.append(dict(kind="pool", x=inp, out=out, B=batch, dim=dim, cin_pad=channels, cout=channels, k=2))

        def w_chain(inp, pc1, pc2, pc3, out, batch, dim, softargmax=None, in_quad=False):
            chain(inp, pc1, pc2, pc3, out, batch, dim, softargmax=softargmax, in_quad=in_quad)
            if rec.on and inp.dtype == BF:
                rec.items.append(dict(kind="chain_sa" if softargmax is not None else "chain", x=inp, pcs=(pc1, pc2, pc3), out=out,
                                      B=batch, dim=dim, cin_pad=32, cout=pc3.cout, k=1))

        def w_run(prog, x, *a, **k):
            lg = run(prog, x, *a, **k)
            rec.logits.append((prog.dtype, lg))
            return lg

        for n, f in (("conv3d", w_conv3d), ("deconv3d_k2s2", w_deconv), ("maxpool3d_2", w_pool), ("pointwise_chain3", w_chain)):
            monkeypatch.setattr(_lib, n, f)
        monkeypatch.setattr(V2VProgram, "run", w_run)


def _layers(net):
    """data_ptr of a packed weight tensor (the tail: id of the packed layer) -> (conv, bn, scale, packed layer)."""
    vn, prog = net.volume_net, net.volume_net.program
    fl, ed, bl = vn.front_layers, vn.encoder_decoder, vn.back_layers
    m = {}

    def put(pc, conv, bn, scale=1.0):
        m[pc.w.data_ptr()] = m[id(pc)] = (conv, bn, scale, pc)

    def res(pcs, blk):
        put(pcs[0], blk.res_branch[0], blk.res_branch[1])
        put(pcs[1], blk.res_branch[3], blk.res_branch[4])
        if pcs[2] is not None:
            put(pcs[2], blk.skip_con[0], blk.skip_con[1])

    put(prog.front0, fl[0].block[0], fl[0].block[1])
    for i, pcs in enumerate(prog.front_res):
        res(pcs, fl[i + 1])
    for k in range(5):
        res(prog.enc[k], getattr(ed, f"encoder_res{k + 1}"))
        res(prog.skip[k], getattr(ed, f"skip_res{k + 1}"))
        res(prog.dec[k], getattr(ed, f"decoder_res{k + 1}"))
        up = getattr(ed, f"decoder_upsample{k + 1}")
        put(prog.up[k], up.block[0], up.block[1])
    res(prog.mid, ed.mid_res)
    res(prog.back_res, bl[0])
    put(prog.back1, bl[1].block[0], bl[1].block[1])
    put(prog.back2, bl[2].block[0], bl[2].block[1])
    put(prog.out, vn.output_layer, None)
    if prog.out_scaled is not prog.out:
        put(prog.out_scaled, vn.output_layer, None, prog.output_scale)
    return m


_FOLDS = {}


def _fold(entry):
    """The layer's weights as the program packed them, and the bias it passes."""
    conv, bn, scale, pc = entry
    key = (pc.w.data_ptr(), scale)
    if key not in _FOLDS:
        conv, bn = copy.deepcopy(conv).cpu(), copy.deepcopy(bn).cpu() if bn is not None else None
        if scale != 1.0:
            with torch.no_grad():
                conv.weight.mul_(float(scale))          # as _PackedConv: float32 weights and bias times the scale, then packed
                conv.bias.mul_(float(scale))
        # the program's own packed tensor, read back through the kernels and held to the float64 fold of the layer's modules
        _FOLDS[key] = (check_packed(pc, conv, bn, f"{pc.cin}->{pc.cout} k{pc.k}")[0], pc.b[:pc.cout].cpu())
    return _FOLDS[key]


def _ncdhw(t, C_):
    """channels-last [B,D,D,D,C] or octet-planar [B,C/8,D,D,D,8] device tensor -> [B,C,D,D,D] view"""
    if t.dim() == 6:
        B, o, D = t.shape[0], t.shape[1], t.shape[2]
        return t.permute(0, 1, 5, 2, 3, 4).reshape(B, o * 8, D, D, D)[:, :C_]
    return t.permute(0, 4, 1, 2, 3)[:, :C_]


def _host(t):
    return t.float().cpu().double()


def check_launches(rec, net, G, B, label):
    rec.on = False
    try:
        _check_launches(rec, net, G, B, label)
    finally:
        rec.on = True


def _check_launches(rec, net, G, B, label):
    layers = _layers(net)
    lines, fails = [], []
    for n, it in enumerate(rec.items):
        kind, D = it["kind"], it["dim"]
        kern = C.kernel_of(kind, it["B"], D, it["cin_pad"], it["cout"], it["k"], it.get("res") is not None)
        SEEN["kernels"].add(kern)
        Do = 2 * D if kind == "deconv" else D // 2 if kind == "pool" else D
        sel = [B - 1] if max(D, Do) == G and B > 1 else list(range(B))        # the G^3 launches: one sample of a batch
        what = f"{label} launch {n} {kind} k{it['k']} {it['cin_pad']}->{it['cout']} @{D}^3 ({kern})"
        if kind == "pool":
            x = it["x"][sel].float().cpu().permute(0, 4, 1, 2, 3)
            got = it["out"][sel].float().cpu().permute(0, 4, 1, 2, 3)
            if not torch.equal(got, F.max_pool3d(x, 2, 2)):
                fails.append(f"{what}: not the exact maximum")
            lines.append(f"{what}: exact")
            continue
        if kind in ("chain", "chain_sa"):
            wb = ()
            for pc in it["pcs"]:
                w, b = _fold(layers[id(pc)])
                wb += (w.reshape(w.shape[0], -1), b)
            x = _ncdhw(it["x"], 32)[sel]
            got = it["out"].view(B, it["cout"], D, D, D)[sel]
            for box in _boxes(D):
                xb, gb = M.crop(x, box, 0)[0], M.crop(got, box, 0)[0]
                cm = M.chain(C.rows(_host(xb)), *wb)
                g = C.rows(_host(gb))
                bad = M.outside(g, cm.logits)
                ratio, nd = M.device_ratio(g, cm)
                lines.append(f"{what} box {box}: outside {int(bad.sum())} of {bad.numel()}, hidden straddle "
                             f"{100 * M.straddle_share(cm.h1):.2f}% / {100 * M.straddle_share(cm.h2):.2f}%, device ratio {ratio:.2f} over {nd} voxels")
                if bool(bad.any()):
                    fails.append(lines[-1])
            continue
        transposed = kind == "deconv"
        assert (it["res"] is not None) == bool(it["flags"] & (M.EPI_RES_PRE_RELU | M.EPI_RES_POST_RELU)), what
        assert it["flags"] & ~7 == 0, f"{what}: a layout flag in a bf16 launch ({it['flags']})"
        w, b = _fold(layers[it["w"].data_ptr()])
        assert tuple(w.shape[:2]) == ((it["cin"], it["cout"]) if transposed else (it["cout"], it["cin"])), what
        x = _ncdhw(it["x"], it["cin"])[sel]
        res = None if it["res"] is None else _ncdhw(it["res"], it["cout"])[sel]
        got = _ncdhw(it["out"], it["cout"])[sel]
        K = it["cin"] * (1 if transposed else it["k"] ** 3)
        for box in _boxes(Do):
            if transposed:
                xb, off = M.crop(x, None if box is None else tuple((a // 2, e // 2) for a, e in box), 0)
                off = None if off is None else tuple((2 * a, 2 * e) for a, e in off)
            else:
                xb, off = M.crop(x, box, it["k"] // 2)
            y, S = M.exact(_host(xb), w, b, it["k"], transposed)
            y, S = M.inner(y, off), M.inner(S, off)
            iv = M.interval(y, S, None if res is None else _host(M.crop(res, box, 0)[0]), it["flags"], M.g_of(K))
            g = _host(M.crop(got, box, 0)[0])
            bad = M.outside(g, iv)
            share = M.straddle_share(iv)
            lo_n, hi_n = M.on_edge(g, iv)
            lines.append(f"{what} flags {it['flags']} box {box}: outside {int(bad.sum())} of {bad.numel()}, straddle {100 * share:.2f}% "
                         f"(on lo {lo_n}, on hi {hi_n})")
            if bool(bad.any()) or share > M.STRADDLE_CAP:
                fails.append(lines[-1])
    print(f"\n[{label}]\n" + "\n".join(lines))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------
# the points
# ------------------------------------------------------------------------------------------------
def _forward(net, img, depth):
    with torch.no_grad():
        kp, _, vols, _ = net(img.to(DEV), net.grid_coord_proj_batch, net.coord_volumes, depth_map_batch=depth.to(DEV))
    torch.cuda.synchronize()
    return kp, vols


POINTS = [pytest.param(32, 1, id="G32-B1"), pytest.param(32, 3, id="G32-B3"), pytest.param(96, 1, id="G96-B1")]


@pytest.mark.parametrize("G,B", POINTS)
def test_bf16_program_launches_vs_float64(G, B, monkeypatch):
    from test_gpu_bf16 import BF16_JOINT_TOL, BF16_LOGIT_RMS_TOL
    net = _net(G)
    net.set_v2v_dtype("bf16")
    _FOLDS.clear()          # keyed by the packed tensors' addresses: one program at a time
    img, depth = synth.make_inputs(2000 + 10 * G + B, B, "floor" if B % 2 else "uniform")
    rec = Launches(monkeypatch)
    kp, vols = _forward(net, img, depth)
    prog = net.volume_net.program
    assert prog.dtype == BF and len(rec.logits) == 1
    assert rec.items[-1]["kind"] == "chain_sa", "the forward did not take the fused soft-argmax tail"
    assert rec.items[0]["x"].dim() == 6 and rec.items[0]["k"] == 7, "the front layer did not read the octet-planar input"
    assert bool(torch.isfinite(kp).all()) and bool(torch.isfinite(vols).all())
    check_launches(rec, net, G, B, f"G{G} B{B} fused")
    # without the fused soft-argmax: run() alone on the forward's own input buffer; only the tail is another launch
    fused = rec.items
    x = rec.items[0]["x"]
    rec.items, rec.logits = [], []
    with torch.no_grad():
        lg = prog.run(x, B, G, scaled=True)
    torch.cuda.synchronize()
    assert [it["kind"] for it in rec.items[:-1]] == [it["kind"] for it in fused[:-1]] and rec.items[-1]["kind"] == "chain"
    for a, b in zip(rec.items, fused):
        assert torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32)), "the two forwards differ"
    rec.items = rec.items[-1:]
    check_launches(rec, net, G, B, f"G{G} B{B} plain tail")
    lg_b = lg.double()
    # the mode's specification against the float32 program on the same inputs
    try:
        net.set_v2v_dtype("fp32")
        rec.logits = []
        kp32, _ = _forward(net, img, depth)
        (dt, lg_f), = rec.logits
        assert dt == torch.float32
        lg_f = lg_f.double().view_as(lg_b)
    finally:
        net.set_v2v_dtype("bf16")
    rel = float((lg_b - lg_f).pow(2).mean().sqrt() / lg_f.std())
    err = float((kp - kp32).abs().max())
    print(f"G{G} B{B}: bf16 against the float32 program: logits rms {rel:.2e} x std, joints {err:.2e} m")
    SEEN["points"].add((G, B))
    assert rel <= BF16_LOGIT_RMS_TOL, rel
    assert err <= BF16_JOINT_TOL, err


def test_bf16_route_matrix_coverage():
    """The points above must reach every bf16 kernel the program can reach: a routing change that empties a route fails here instead
    of silently shrinking what the module checks.  conv_bf16_k7_kernel is out of the program's reach (the grid is a multiple of 32,
    so the front layer always takes the row-reuse kernel); tests/test_gpu_bf16_launches.py runs it."""
    if SEEN["points"] != {(p.values[0], p.values[1]) for p in POINTS}:
        pytest.skip("coverage is asserted over the whole matrix; run the module without a selection")
    fam = {C.family(k) for k in SEEN["kernels"]}
    assert set(C.KERNEL_FAMILIES) - {"conv_bf16_k7_kernel"} <= fam, set(C.KERNEL_FAMILIES) - fam
    assert {"conv_bf16_k3_splitk_kernel<1,4>", "conv_bf16_k3_splitk_kernel<2,4>", "conv_bf16_direct_kernel<1>", "conv_bf16_k3_kernel<8>",
            "deconv_bf16_kernel<2>", "deconv_bf16_kernel<4>"} <= SEEN["kernels"], SEEN["kernels"]
