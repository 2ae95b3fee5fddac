"""GPU: every launch form of the bf16-storage V2V program through the C ABI, held to float64 within ONE rounding.

The criterion is tests/bf16_launch_model.py: with the exact float64 value y and the magnitude S of a launch's dot products,
delta = g 2^-24 S, every output element must lie in [bf16_rne(epi(y - delta)), bf16_rne(epi(y + delta))] - the exact bit pattern
wherever the two ends agree (over 90 % of every case, asserted on the host).  The cases (tests/bf16_launch_cases.py) are the
smallest shapes that reach each branch of the dispatchers: partial 16-voxel tiles, an odd tile count on the two-tile split-K
kernel, the 32768-voxel boundary between split-K and direct, the levels of G = 32 and G = 96, every transposed-convolution
instantiation, the fused tail with idle waves and a partial last chunk.

Harness: outputs are NaN-filled and sit inside a larger NaN-filled allocation whose margins must stay untouched; inputs and skip
tensors sit inside NaN-filled allocations too, so a read outside the tensor shows in the result; pad channels hold finite garbage.
Every launch runs twice and must give identical bits.  The model is fed the launch's own operands: the packed weights read back
through the kernels themselves (packed_weights) and the packed float32 bias, both held to the float64 BatchNorm fold
(check_packed).  They are NOT taken from torch-CPU's float32 fold in the packer's order: on the device about one weight in 10^5
differs from it by one bf16 ulp (test_packer_roundtrip_through_the_kernels).
"""
import copy
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from sceneego_amd import _lib
from sceneego_amd.v2v import V2VModel, _PackedConv, channels_last_to_octet_planar

import bf16_launch_cases as C
import bf16_launch_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
MARGIN = 1 << 14            # elements of NaN in front of and behind every tensor
NAN = float("nan")
torch.set_num_threads(min(16, torch.get_num_threads()))


class Embedded:
    """A tensor inside a larger NaN-filled allocation."""

    def __init__(self, shape, dtype=BF, value=None):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((n + 2 * MARGIN,), NAN, device=DEV, dtype=dtype)
        self.t = self.buf[MARGIN:MARGIN + n].view(shape)
        if value is not None:
            self.t.copy_(value)

    def margins_untouched(self):
        return bool(torch.isnan(self.buf[:MARGIN]).all()) and bool(torch.isnan(self.buf[MARGIN + self.n:]).all())


def _ndhwc(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _ncdhw(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _pack(conv, bn, cin_pad=None):
    return _PackedConv(copy.deepcopy(conv).to(DEV), copy.deepcopy(bn).to(DEV) if bn is not None else None, cin_pad, BF)


def _input(x, cin_pad, octet):
    """[B,cin,D,D,D] float32 (bf16 values) -> the launch's input layout, pad channels = finite garbage, NaN around the tensor."""
    B, cin, D = x.shape[0], x.shape[1], x.shape[2]
    cl = torch.full((B, D, D, D, cin_pad), 3.0, dtype=BF)
    cl[..., :cin] = _ndhwc(x).to(BF)
    if octet:
        cl = channels_last_to_octet_planar(cl)
    return Embedded(tuple(cl.shape), value=cl)


def _launch(c, pc, xin, res, out):
    if c.transposed:
        _lib.deconv3d_k2s2(xin.t, pc.w, pc.b, res.t if res else None, out.t, c.B, c.dim, c.cin, c.cout, c.flags)
    else:
        _lib.conv3d(xin.t, pc.w, pc.b, res.t if res else None, out.t, c.B, c.dim, c.cin, c.cin_pad, c.cout, c.k, c.flags)


SEEN = set()
RAN = set()


# ------------------------------------------------------------------------------------------------
# the packer, read back through the kernels
# ------------------------------------------------------------------------------------------------
_EYE = []


def packed_weights(pc):
    """The weights of a packed layer as the KERNELS see them, in torch's layout (float32 holding bf16 values).  One-hot inputs: sample
    b holds a single 1 at the centre voxel of channel b and the launch gets a zero bias, so the output IS the packed weight:
    w[co, b, tap] lands on voxel (k - 1 - tap) of sample b (transposed: on output parity tap).  A layer with neither 16 nor a
    multiple of 32 couts (output_layer) is read through the plain chain behind two identity layers."""
    cin, cout, k = pc.cin, pc.cout, pc.k
    zero = torch.zeros_like(pc.b)
    dim = 1 if pc.transposed else k
    x = torch.zeros((cin, cin) + (dim,) * 3)
    x[torch.arange(cin), torch.arange(cin), dim // 2, dim // 2, dim // 2] = 1.0
    xin = _input(x, pc.cin_pad, octet=k == 7)
    if not pc.transposed and cout % 32 and cout != 16:
        assert k == 1 and cin == 32
        if not _EYE:
            eye = nn.Conv3d(32, 32, 1)
            with torch.no_grad():
                eye.weight.copy_(torch.eye(32).view(32, 32, 1, 1, 1))
                eye.bias.zero_()
            _EYE.append(_pack(eye, None))
        out = Embedded((32, cout, 1), dtype=torch.float32)
        _lib.pointwise_chain3(xin.t, _EYE[0], _EYE[0], types.SimpleNamespace(w=pc.w, b=zero, cout=cout), out.t, 32, 1)
        torch.cuda.synchronize()
        assert out.margins_untouched()
        return out.t.cpu().view(32, cout).T.reshape(cout, 32, 1, 1, 1).contiguous()
    out = Embedded((cin,) + ((2 * dim if pc.transposed else dim),) * 3 + (cout,))
    if pc.transposed:
        _lib.deconv3d_k2s2(xin.t, pc.w, zero, None, out.t, cin, dim, cin, cout, 0)
    else:
        _lib.conv3d(xin.t, pc.w, zero, None, out.t, cin, dim, cin, pc.cin_pad, cout, k, 0)
    torch.cuda.synchronize()
    assert out.margins_untouched()
    got = _ncdhw(out.t.cpu()).float()                       # [ci, co, taps...]
    return (got if pc.transposed else got.flip(2, 3, 4).transpose(0, 1)).contiguous()


def fold64(conv, bn):
    """The BatchNorm fold in float64: (w, b, and the magnitude |(b - mean) sc| + |beta| the bias's float32 roundings scale with)."""
    w, b = conv.weight.detach().double(), conv.bias.detach().double()
    if bn is None:
        return w, b, b.abs()
    sc = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    w = w * (sc.view(1, -1, 1, 1, 1) if isinstance(conv, nn.ConvTranspose3d) else sc.view(-1, 1, 1, 1, 1))
    t = (b - bn.running_mean.double()) * sc
    return w, t + bn.bias.detach().double(), t.abs() + bn.bias.detach().double().abs()


def check_packed(pc, conv, bn, what):
    """Every weight within half a bf16 ulp plus three float32 roundings (square root, division, multiply) of the float64 fold; every
    bias within six float32 roundings of it (add, square root, division, subtract, multiply, add).  Returns the read-back weights and
    in how many places they differ from the CPU float32 fold in the packer's order."""
    got = packed_weights(pc)
    w64, b64, bmag = fold64(conv, bn)
    assert bool(((got.double() - w64).abs() <= 0.5 * M.bf16_ulp(w64) + 3 * M.U24 * w64.abs()).all()), f"{what}: packed weights off the fold"
    assert bool(((pc.b[:pc.cout].cpu().double() - b64).abs() <= 6 * M.U24 * bmag).all()), f"{what}: packed bias off the fold"
    if pc.b.numel() > pc.cout:
        assert float(pc.b[pc.cout:].abs().max()) == 0.0
    return got, int((got != C.fold(conv, bn)[0]).sum())


# every (cin, cin_pad, cout, k, transposed) of the program (sceneego_amd/v2v.py: front layer, Res3DBlocks and their skip
# convolutions, decoder_upsample1..5, back_layers.1 / .2, output_layer)
PACKED_LAYERS = [(33, 40, 16, 7, False)] + \
    [(ci, ci, co, 3, False) for ci, co in ((16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128))] + \
    [(ci, ci, co, 1, False) for ci, co in ((16, 32), (32, 64), (64, 128), (32, 32))] + \
    [(ci, ci, co, 2, True) for ci, co in ((64, 32), (128, 64), (128, 128))]
FOLD_DIFFERENCES = []


@pytest.mark.parametrize("cin,cin_pad,cout,k,transposed", PACKED_LAYERS)
def test_packer_roundtrip_through_the_kernels(cin, cin_pad, cout, k, transposed):
    """Random BatchNorm statistics; the packed weights are read back through the kernels (packed_weights) and held to the float64
    fold.  Measured on MI355X: the device's fold differs from torch-CPU's float32 fold in the packer's order in about one weight of
    10^5 (the BatchNorm scale gamma / sqrt(var + eps) differs in its last float32 bit on some channels, which moves a product across a
    bf16 rounding boundary with probability 2^-16); both are within the bound.  The launch and program tests therefore take their
    reference weights from this read-back, never from the CPU fold."""
    gen = torch.Generator().manual_seed(cin * 1000 + cout * 10 + k)
    conv, bn = C._layer(cin, cout, k, transposed, gen)
    pc = _pack(conv, bn, cin_pad)
    got, ndiff = check_packed(pc, conv, bn, f"{cin}->{cout} k{k}")
    FOLD_DIFFERENCES.append((ndiff, got.numel()))
    print(f"packer {cin}->{cout} k{k}{' transposed' if transposed else ''}: {ndiff} of {got.numel()} weights differ from the CPU float32 fold")
    assert float((got - C.fold(conv, bn)[0]).abs().max()) <= float(M.bf16_ulp(got).max())      # a neighbouring bf16 value at most
    # the same layer with the folded bias made exactly zero (bias = running mean, beta = 0): the weights do not move
    with torch.no_grad():
        conv.bias.copy_(bn.running_mean)
        bn.bias.zero_()
    pc0 = _pack(conv, bn, cin_pad)
    assert float(pc0.b.abs().max()) == 0.0
    assert torch.equal(pc0.w.view(torch.int16), pc.w.view(torch.int16))


def test_packer_plain_output_layer():
    """output_layer: no BatchNorm, so the packed weights ARE the float32 weights rounded to nearest even, bit for bit; 15 couts in one
    16-row tile, read back through the plain chain; with its bias the logit is one product and a single float32 addition."""
    gen = torch.Generator().manual_seed(15)
    for cout3 in (15, 16):
        last, _ = C._layer(32, cout3, 1, False, gen, bn=False)
        p3 = _pack(last, None)
        w, b = C.fold(last, None)
        assert torch.equal(packed_weights(p3), w)
        assert torch.equal(p3.b[:cout3].cpu(), b)
        x = torch.zeros((32, 32, 1, 1, 1))
        x[torch.arange(32), torch.arange(32)] = 1.0
        xin = _input(x, 32, False)
        out = Embedded((32, cout3, 1), dtype=torch.float32)
        _lib.pointwise_chain3(xin.t, _EYE[0], _EYE[0], p3, out.t, 32, 1)
        torch.cuda.synchronize()
        assert out.margins_untouched()
        assert torch.equal(out.t.cpu().view(32, cout3), w.view(cout3, 32).T + b)


# ------------------------------------------------------------------------------------------------
# one launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.LAUNCH_CASES, ids=[c.id for c in C.LAUNCH_CASES])
def test_launch_vs_float64_interval(c):
    o = C.operands(c)
    pc = _pack(o.conv, o.bn, c.cin_pad)
    w, ndiff = check_packed(pc, o.conv, o.bn, c.id)
    ref = C.reference(c, w, pc.b[:c.cout].cpu())        # the weights the kernel multiplies by and the bias it adds
    xin = _input(o.x, c.cin_pad, octet=c.k == 7)
    res = Embedded((c.B,) + (c.dim_out,) * 3 + (c.cout,), value=_ndhwc(o.res).to(BF)) if o.res is not None else None
    outs = [Embedded((c.B,) + (c.dim_out,) * 3 + (c.cout,)) for _ in range(2)]
    for out in outs:
        _launch(c, pc, xin, res, out)
    torch.cuda.synchronize()
    for out in outs:
        assert out.margins_untouched(), f"{c.id}: wrote outside the output tensor"
    assert xin.margins_untouched() and (res is None or res.margins_untouched())
    assert torch.equal(outs[0].t.view(torch.int16), outs[1].t.view(torch.int16)), f"{c.id}: two launches differ"
    got = _ncdhw(outs[0].t.cpu())
    iv = ref.interval
    bad = M.outside(got, iv)
    lo_n, hi_n = M.on_edge(got, iv)
    kern = C.case_kernel(c)
    print(f"{c.id}: {kern} g_ref={ref.g_ref:.2f} g={ref.g:g} straddle={100 * M.straddle_share(iv):.2f}% on_lo={lo_n} on_hi={hi_n} "
          f"outside={int(bad.sum())} of {bad.numel()} nan={int(torch.isnan(got).sum())} weights off the CPU fold: {ndiff} "
          f"reference {ref.seconds:.2f}s")
    SEEN.add(kern)
    RAN.add(c)
    assert M.straddle_share(iv) <= M.STRADDLE_CAP
    assert not bool(bad.any()), f"{c.id} ({kern}): {int(bad.sum())} of {bad.numel()} elements outside [lo, hi], first at " \
                                f"{tuple(int(i) for i in bad.nonzero()[0])}: got {float(got[tuple(bad.nonzero()[0])])}"


# ------------------------------------------------------------------------------------------------
# max-pool: exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,dim,ch", C.POOL_CASES)
def test_maxpool_exact(B, dim, ch):
    x = torch.randn((B, ch, dim, dim, dim), generator=torch.Generator().manual_seed(dim + ch)).to(BF)
    xin = Embedded((B, dim, dim, dim, ch), value=_ndhwc(x))
    outs = [Embedded((B,) + (dim // 2,) * 3 + (ch,)) for _ in range(2)]
    for out in outs:
        _lib.maxpool3d_2(xin.t, out.t, B, dim, ch)
    torch.cuda.synchronize()
    assert outs[0].margins_untouched() and outs[1].margins_untouched()
    assert torch.equal(outs[0].t.view(torch.int16), outs[1].t.view(torch.int16))
    assert torch.equal(_ncdhw(outs[0].t.cpu()).float(), F.max_pool3d(x.float(), 2, 2))
    SEEN.add(C.kernel_of("pool", B, dim, ch, ch, 2))
    RAN.add(("pool", B, dim, ch))


# ------------------------------------------------------------------------------------------------
# the tail
# ------------------------------------------------------------------------------------------------
def _chain_weights(o):
    """(w1, b1, w2, b2, w3, b3) as the device holds them: read-back weights, packed biases"""
    wb = ()
    for conv, bn in o.layers:
        pc = _pack(conv, bn)
        w, _ = check_packed(pc, conv, bn, "chain")
        wb += (w.reshape(w.shape[0], -1), pc.b[:pc.cout].cpu())
    return wb


def _chain_launch(o, B, dim, cout3, softargmax=None, x=None):
    pcs = [_pack(conv, bn) for conv, bn in o.layers]
    xin = _input(o.x if x is None else x, 32, False)
    out = Embedded((B, cout3, dim ** 3), dtype=torch.float32)
    _lib.pointwise_chain3(xin.t, pcs[0], pcs[1], pcs[2], out.t, B, dim, softargmax=softargmax)
    torch.cuda.synchronize()
    assert out.margins_untouched() and xin.margins_untouched()
    return out.t


DEVICE_RATIO = []


@pytest.mark.parametrize("c", C.CHAIN_CASES, ids=[c.id for c in C.CHAIN_CASES])
def test_chain_vs_float64_interval(c):
    o = C.chain_operands(c.cout, c.B, c.dim)
    cm = M.chain(C.rows(o.x), *_chain_weights(o))
    assert M.straddle_share(cm.h1) <= M.STRADDLE_CAP and M.straddle_share(cm.h2) <= M.STRADDLE_CAP
    a, b = _chain_launch(o, c.B, c.dim, c.cout), _chain_launch(o, c.B, c.dim, c.cout)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    got = a.cpu().permute(0, 2, 1).reshape(-1, c.cout)
    bad = M.outside(got, cm.logits)
    ratio, n = M.device_ratio(got, cm)
    DEVICE_RATIO.append(ratio)
    print(f"{c.id}: outside={int(bad.sum())} of {bad.numel()}; device |logit - y| / (2^-24 S) = {ratio:.2f} over {n} determined voxels "
          f"(g / 4 = {M.G_FACTOR / 4:g})")
    SEEN.add(C.kernel_of("chain", c.B, c.dim, 32, c.cout, 1))
    RAN.add(c)
    assert not bool(bad.any()), (c.id, int(bad.sum()))
    # the device's own ratio: above g / 4 the margin of 4 over the reference's order would be used up - find out why, do not raise g
    assert not ratio > M.G_FACTOR / 4, ratio


@pytest.mark.parametrize("B,dim", C.FUSED_TAIL_CASES)
def test_fused_softargmax_tail(B, dim):
    """se_pointwise_chain3_softargmax_bf16: logits bit-equal to the plain bf16 chain (itself held to float64 above); joints and
    volumes through se_softargmax3d_finish_f32 within the float32 twin's bars of the two-pass soft-argmax on those logits; a NaN
    input voxel makes exactly its own sample's joints NaN."""
    o = C.chain_operands(15, B, dim, seed=1000 * B + dim)
    N = dim ** 3
    coord = ((torch.rand((N, 3), generator=torch.Generator().manual_seed(dim)) - 0.5) * 2.0).to(DEV)
    rows = B * 15

    def fused(x=None):
        scratch = torch.full((_lib.softargmax3d_scratch_elems(rows),), NAN, device=DEV)
        lg = _chain_launch(o, B, dim, 15, softargmax=(coord, scratch), x=x)
        vol, j = torch.full((B, 15, N), NAN, device=DEV), torch.full((B, 15, 3), NAN, device=DEV)
        _lib.softargmax3d_finish(lg, scratch, vol, j, rows, N, 1)
        return lg, vol, j

    plain = _chain_launch(o, B, dim, 15)
    lg, vol, j = fused()
    lg2, vol2, j2 = fused()
    assert torch.equal(lg, plain)
    assert torch.equal(lg2, lg) and torch.equal(vol2, vol) and torch.equal(j2, j)
    cm = M.chain(C.rows(o.x), *_chain_weights(o))
    assert not bool(M.outside(lg.cpu().permute(0, 2, 1).reshape(-1, 15), cm.logits).any())
    vol_ref, j_ref = torch.empty_like(vol), torch.empty_like(j)
    _lib.softargmax3d(plain.contiguous(), coord, vol_ref, j_ref, rows, N, 1)
    ej, ev = float((j - j_ref).abs().max()), float((vol - vol_ref).abs().max() / vol_ref.max())
    print(f"fused tail B={B} D={dim}: joints {ej:.2e} m, volumes {ev:.2e} relative, sum {float(vol.sum()):.6f}")
    assert ej < 2e-6
    assert ev <= 1e-5
    assert abs(float(vol.sum()) - rows) < 1e-3
    SEEN.add(C.kernel_of("chain_sa", B, dim, 32, 15, 1))
    RAN.add(("fused", B, dim))
    # one NaN voxel in the last sample
    x = o.x.clone()
    x[B - 1, 3, dim // 2, dim - 1, dim - 1] = NAN
    _, _, jn = fused(x)
    assert bool(torch.isnan(jn[B - 1]).all()), "the NaN input voxel did not reach every joint of its sample"
    assert torch.equal(jn[:B - 1], j[:B - 1]), "the NaN input voxel changed another sample"


@pytest.mark.parametrize("B,dim", C.FUSED_TAIL_REFUSED)
def test_fused_softargmax_tail_refuses_partial_tiles(B, dim):
    """chunk & 15: a chunk that is not whole 16-voxel tiles is an argument error, before anything is launched."""
    o = C.chain_operands(15, B, dim, seed=1)
    pcs = [_pack(conv, bn) for conv, bn in o.layers]
    x = _ndhwc(o.x).to(BF).to(DEV)
    out = torch.full((B, 15, dim ** 3), NAN, device=DEV)
    coord = torch.zeros((dim ** 3, 3), device=DEV)
    scratch = torch.full((_lib.softargmax3d_scratch_elems(B * 15),), NAN, device=DEV)
    lib = _lib.load()
    code = lib.se_pointwise_chain3_softargmax_bf16(_lib._ptr(x), _lib._ptr(pcs[0].w), _lib._ptr(pcs[0].b), _lib._ptr(pcs[1].w),
                                                   _lib._ptr(pcs[1].b), _lib._ptr(pcs[2].w), _lib._ptr(pcs[2].b), _lib._ptr(out),
                                                   _lib._ptr(coord), _lib._ptr(scratch), B, dim, 15, _lib._stream())
    torch.cuda.synchronize()
    assert code == -1                                       # SE_ERR_BAD_ARG
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(scratch).all())
    with pytest.raises(_lib.HipExtensionError):
        _lib.pointwise_chain3(x, pcs[0], pcs[1], pcs[2], out, B, dim, softargmax=(coord, scratch))


def test_17_joints_fail_when_the_program_is_compiled():
    """cout 17 has no bf16 packing (<= 16 or a multiple of 32): the error comes from compile(), not from inside a forward."""
    model = V2VModel(33, 17).eval().to(DEV)
    with pytest.raises(_lib.HipExtensionError):
        model.compile(torch.bfloat16)


def test_launch_cases_reached_every_kernel():
    """Every __global__ convolution, transposed convolution, pool and tail kernel of the two bf16 files ran in this module."""
    fam = {C.family(k) for k in SEEN}
    whole = set(C.LAUNCH_CASES) | set(C.CHAIN_CASES) | {("pool",) + p for p in C.POOL_CASES} | {("fused",) + p for p in C.FUSED_TAIL_CASES}
    if RAN != whole:
        pytest.skip("coverage is asserted over the whole module; run it without a selection")
    assert set(C.KERNEL_FAMILIES) <= fam, set(C.KERNEL_FAMILIES) - fam
    if DEVICE_RATIO:
        print(f"device logit ratio: max {max(DEVICE_RATIO):.2f} (g = {M.G_FACTOR:g}, g / 4 = {M.G_FACTOR / 4:g})")
