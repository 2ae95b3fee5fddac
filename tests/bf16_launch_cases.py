"""The case matrix of the bf16-storage launch tests: the smallest shapes that reach each branch of se_conv3d_bf16,
se_deconv3d_k2s2_bf16 and the fused tail, their operands (seeded, CPU) and their float64 references (computed once per session and
shared by tests/test_bf16_launch_model_host.py and tests/test_gpu_bf16_launches.py).

The kernel a shape runs on follows from the shape alone; ``kernel_of`` restates the dispatcher's rules (csrc/conv3d_bf16.hip
se_conv3d_bf16, csrc/conv3d_bf16_tiled.hip se_conv3d_bf16_tiled_try) so that the tests can assert which kernels they reach.
"""
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

import bf16_launch_model as M

BF = torch.bfloat16
R, PRE, POST = M.EPI_RELU, M.EPI_RES_PRE_RELU, M.EPI_RES_POST_RELU


class Case(NamedTuple):
    kind: str           # "conv" | "deconv" | "chain"
    B: int
    dim: int            # input level size
    cin: int
    cout: int
    k: int
    flags: int          # EPI_* word; a residual / skip tensor is passed exactly when it carries PRE or POST

    @property
    def id(self):
        f = "".join(n for n, b in (("R", R), ("pre", PRE), ("post", POST)) if self.flags & b) or "plain"
        return f"{self.kind}-k{self.k}-B{self.B}-D{self.dim}-{self.cin}to{self.cout}-{f}"

    @property
    def cin_pad(self):
        return (self.cin + 7) // 8 * 8

    @property
    def transposed(self):
        return self.kind == "deconv"

    @property
    def dim_out(self):
        return 2 * self.dim if self.transposed else self.dim

    @property
    def K(self):
        """terms of one output's dot product"""
        return self.cin * (1 if self.transposed else self.k ** 3)

    @property
    def seed(self):
        return (self.B * 1000003 + self.dim * 10007 + self.cin * 101 + self.cout * 7 + self.k * 3 + self.flags) % (1 << 31)


def _conv(B, dim, cin, cout, flags, k=3):
    return Case("conv", B, dim, cin, cout, k, flags)


CONV_CASES = [
    # 3^3, conv_bf16_k3_splitk_kernel<1,4>: fewer than 128 voxel tiles
    _conv(1, 1, 128, 128, R | PRE),         # one voxel: only the centre tap is inside
    _conv(5, 1, 128, 128, R),
    _conv(1, 2, 128, 128, R | PRE),
    _conv(2, 3, 128, 128, R | PRE),         # 54 voxels: a partial fourth tile
    _conv(3, 6, 128, 128, R | PRE),         # 40.5 tiles
    _conv(1, 12, 64, 128, R),
    # 3^3, conv_bf16_k3_splitk_kernel<2,4>: from 128 tiles to 32768 voxels
    _conv(2, 12, 128, 128, R | PRE),
    _conv(10, 6, 128, 128, R | PRE),        # 135 tiles, odd: the second tile of the last workgroup is wholly out of range (G=96, batch 10)
    _conv(64, 8, 16, 32, R),                # exactly 32768 voxels
    # 3^3, conv_bf16_direct_kernel
    _conv(65, 8, 16, 32, R),                # just past the boundary
    _conv(3, 24, 64, 128, R | PRE),
    _conv(5, 20, 16, 32, R),                # 2500 tiles on workgroups of 8: a ragged last workgroup (through the ABI only)
    # 3^3, conv_bf16_k3_kernel (LDS tiles, dim % 16 == 0)
    _conv(1, 48, 32, 64, R),
    _conv(1, 48, 64, 64, R | PRE),
    _conv(3, 16, 16, 32, R),
    _conv(1, 16, 32, 32, R | POST),         # EPI_RES_POST_RELU on a convolution
] + [
    # 1x1x1 (the skip convolutions: no ReLU), conv_bf16_direct_kernel<1, ...>
    _conv(B, dim, cin, cout, 0, k=1) for cin, cout in ((16, 32), (32, 64), (64, 128)) for B, dim in ((1, 1), (3, 6), (1, 12), (5, 20))
] + [
    # 7^3, 33 channels (cin_pad 40) -> 16
    _conv(1, 48, 33, 16, R, k=7),           # conv_bf16_k7r_kernel, 3 tiles in z
    _conv(3, 16, 33, 16, R, k=7),
    _conv(1, 24, 33, 16, R, k=7),           # conv_bf16_k7_kernel<false>, 27 tiles
    _conv(1, 12, 33, 16, R, k=7),           # conv_bf16_direct_kernel<7, ...>
]
DECONV_CASES = [Case("deconv", B, dim, cin, cout, 2, R | (POST if skip else 0))
                for B, dim, cin, cout in ((2, 1, 128, 128), (1, 3, 128, 128), (3, 6, 128, 128), (2, 12, 128, 64), (1, 24, 64, 32),
                                          (1, 16, 32, 32), (2, 8, 96, 64))
                for skip in (True, False)]
CHAIN_CASES = [Case("chain", B, dim, 32, cout3, 1, 0) for cout3 in (15, 16) for B, dim in ((1, 16), (2, 6), (3, 1))]
LAUNCH_CASES = CONV_CASES + DECONV_CASES
POOL_CASES = [(3, 2, 128), (2, 6, 128), (1, 48, 64), (2, 6, 8), (2, 6, 40)]            # (B, dim, channels): exact
# fused soft-argmax tail (B, dim): chunk 16 with fifteen idle waves; a last chunk of 8 voxels; 256 / 128 / 128 chunks per sample
FUSED_TAIL_CASES = [(8, 8), (8, 10), (1, 16), (3, 16), (2, 32)]
FUSED_TAIL_REFUSED = [(1, 8), (8, 12)]          # chunk & 15


# ------------------------------------------------------------------------------------------------
# the dispatcher's rules, restated
# ------------------------------------------------------------------------------------------------
def kernel_of(kind, B, dim, cin_pad, cout, k, has_res=False):
    """The __global__ kernel (with its template arguments where the dispatcher chooses them) a launch runs on."""
    vox = B * dim ** 3
    if kind == "deconv":
        return f"deconv_bf16_kernel<{cin_pad // 32}>"
    if kind == "pool":
        return "maxpool2_bf16_kernel"
    if kind == "chain":
        return "pointwise_chain3_bf16_kernel"
    if kind == "chain_sa":
        return "pointwise_chain3_sa_bf16_kernel"
    octs = cin_pad // 8
    oc = 1 if k == 7 else (2 if octs % 2 == 0 else 1) if k == 3 else (4 if octs % 4 == 0 else 2 if octs % 2 == 0 else 1)
    pair = cout % 32 == 0
    if k == 3 and dim % 16 == 0 and cin_pad % 16 == 0 and pair and vox < 2 ** 31:
        return "conv_bf16_k3_kernel<8>"
    if k == 7 and dim % 8 == 0 and cout == 16 and not has_res and dim ** 3 * 8 < 2 ** 31:
        return "conv_bf16_k7r_kernel" if dim % 16 == 0 else "conv_bf16_k7_kernel<false>"
    if k == 3 and pair and oc == 2 and vox <= 32768:
        return "conv_bf16_k3_splitk_kernel<2,4>" if (vox + 15) // 16 >= 128 else "conv_bf16_k3_splitk_kernel<1,4>"
    return f"conv_bf16_direct_kernel<{k}>"


def case_kernel(c):
    return kernel_of(c.kind, c.B, c.dim, c.cin_pad, c.cout, c.k, bool(c.flags & (PRE | POST)))


# every __global__ convolution / transposed convolution / pool / tail kernel of conv3d_bf16.hip and conv3d_bf16_tiled.hip
# (conv_bf16_k7_kernel<true> is selected by the development library's A/B switch only)
KERNEL_FAMILIES = ("conv_bf16_direct_kernel", "conv_bf16_k3_splitk_kernel", "conv_bf16_k3_kernel", "conv_bf16_k7_kernel",
                   "conv_bf16_k7r_kernel", "deconv_bf16_kernel", "maxpool2_bf16_kernel", "pointwise_chain3_bf16_kernel",
                   "pointwise_chain3_sa_bf16_kernel")


def family(kernel):
    return kernel.split("<")[0]


# ------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------
def rand_bn(c, gen):
    bn = nn.BatchNorm3d(c).eval()
    u = lambda lo, hi: torch.rand(c, generator=gen) * (hi - lo) + lo
    with torch.no_grad():
        bn.weight.copy_(u(0.5, 1.5))
        bn.bias.copy_(u(-0.3, 0.3))
        bn.running_mean.copy_(u(-0.3, 0.3))
        bn.running_var.copy_(u(0.5, 1.5))
    return bn


def fold(conv, bn):
    """CPU float32 fold in the packer's order (pack_bf16_kernel): sc = gamma / sqrt(var + eps), ONE multiply, round to nearest even;
    bias (b - mean) * sc + beta.  Returns (w as float32 holding bf16 values, b float32)."""
    w, b = conv.weight.detach().float(), conv.bias.detach().float()
    if bn is not None:
        sc = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
        w = w * (sc.view(1, -1, 1, 1, 1) if isinstance(conv, nn.ConvTranspose3d) else sc.view(-1, 1, 1, 1, 1))
        b = (b - bn.running_mean) * sc + bn.bias.detach()
    return w.to(BF).float(), b


class Operands(NamedTuple):
    conv: nn.Module
    bn: Optional[nn.Module]
    x: torch.Tensor             # [B,cin,D,D,D] float32 holding bf16 values
    res: Optional[torch.Tensor]
    w: torch.Tensor             # folded, bf16 values
    b: torch.Tensor             # folded float32 bias


def _layer(cin, cout, k, transposed, gen, bn=True):
    conv = nn.ConvTranspose3d(cin, cout, 2, stride=2) if transposed else nn.Conv3d(cin, cout, k, padding=k // 2)
    fan = cin * (1 if transposed else k ** 3)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / fan) ** 0.5)
        conv.bias.copy_(torch.rand(cout, generator=gen) * 0.4 - 0.2)
    return conv, (rand_bn(cout, gen) if bn else None)


_OPS = {}


def operands(c):
    if c not in _OPS:
        gen = torch.Generator().manual_seed(c.seed)
        conv, bn = _layer(c.cin, c.cout, c.k, c.transposed, gen)
        x = torch.randn((c.B, c.cin) + (c.dim,) * 3, generator=gen).to(BF).float()
        res = None
        if c.flags & (PRE | POST):
            res = torch.randn((c.B, c.cout) + (c.dim_out,) * 3, generator=gen).to(BF).float()
        _OPS[c] = Operands(conv, bn, x, res, *fold(conv, bn))
    return _OPS[c]


class ChainOperands(NamedTuple):
    layers: tuple               # three (conv, bn)
    x: torch.Tensor             # [B,32,D,D,D]
    wb: tuple                   # (w1 [32,32], b1, w2, b2, w3 [cout3,32], b3)


def chain_operands(cout3, B, dim, seed=None):
    key = ("chain", cout3, B, dim, seed)
    if key not in _OPS:
        gen = torch.Generator().manual_seed(7919 * cout3 + 31 * B + dim if seed is None else seed)
        layers = (_layer(32, 32, 1, False, gen), _layer(32, 32, 1, False, gen), _layer(32, cout3, 1, False, gen, bn=False))
        x = torch.randn((B, 32) + (dim,) * 3, generator=gen).abs().to(BF).float()       # the tail reads a ReLU output
        wb = ()
        for conv, bn in layers:
            w, b = fold(conv, bn)
            wb += (w.reshape(w.shape[0], -1), b)
        _OPS[key] = ChainOperands(layers, x, wb)
    return _OPS[key]


def rows(t):
    """[B,C,D,D,D] -> [B*D^3, C]"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------------------
# references: once per session
# ------------------------------------------------------------------------------------------------
class Reference(NamedTuple):
    lo: torch.Tensor            # bf16 tensors [B,cout,Do,Do,Do]
    hi: torch.Tensor
    acc32: torch.Tensor         # torch-CPU float32 accumulator (convolution + bias), before the epilogue
    g_ref: float
    g: float
    seconds: float

    @property
    def interval(self):
        return M.Interval(self.lo.double(), self.hi.double())


_REF = {}


def reference(c, w=None, b=None):
    """``w``, ``b``: the weights and the bias of the launch when they are not the CPU fold - the GPU tests pass what the device packed
    (weights read back through the kernels, the packed bias), so the model is fed the launch's own operands and needs no slack."""
    o = operands(c)
    same = (w is None or torch.equal(w, o.w)) and (b is None or torch.equal(b, o.b))
    key = c if same else (c, "device")
    if key not in _REF:
        import time
        t0 = time.perf_counter()
        w, b = (o.w, o.b) if same else (o.w if w is None else w, o.b if b is None else b)
        y, S = M.exact(o.x, w, b, c.k, c.transposed)
        acc32 = M.float32_reference(o.x, w, b, c.k, c.transposed)
        g = M.g_of(c.K)
        iv = M.interval(y, S, o.res, c.flags, g)
        # bf16 holds the bounds exactly: kept in two bytes each
        _REF[key] = Reference(iv.lo.to(BF), iv.hi.to(BF), acc32, M.g_ref(acc32, y, S), g, time.perf_counter() - t0)
    return _REF[key]


_CHAIN_REF = {}


def chain_reference(cout3, B, dim, seed=None):
    key = (cout3, B, dim, seed)
    if key not in _CHAIN_REF:
        o = chain_operands(cout3, B, dim, seed)
        _CHAIN_REF[key] = M.chain(rows(o.x), *o.wb)
    return _CHAIN_REF[key]
