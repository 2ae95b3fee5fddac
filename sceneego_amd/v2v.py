"""V2V-PoseNet 3D encoder-decoder on hand-written HIP kernels.

Stands in for the reference's ``network/v2v.py`` (``V2VModel`` ``:142-181``, ``EncoderDecorder`` ``:70-139``,
``Res3DBlock`` ``:21-43``, ``Basic3DBlock`` ``:8-18``, ``Pool3DBlock`` ``:46-52``, ``Upsample3DBlock`` ``:55-67``).

Two layers:

* The ``nn.Module`` tree below is a *parameter container*: same sub-module names, parameter shapes and
  initialisation as the reference, so ``state_dict()`` has the reference's keys and the
  published checkpoint loads strictly.  The modules own no arithmetic.
* ``V2VProgram`` is what runs: built once from the tree (``V2VModel.compile``), it folds every eval-mode
  BatchNorm3d into its convolution, re-orders the weights into MFMA fragment order on the device
  (``se_conv3d_pack_f32``: csrc/conv3d_pack.hip, once per layer, here and never in a timed step) and walks the network's fixed structure, one kernel per Conv3d+BN(+ReLU)(+residual) /
  ConvTranspose3d+BN+ReLU(+skip) / max-pool.  What each launch looks like - tensor layouts (channels-last, quad- or
  octet-planar), flag words, fused skip / pooled / tail forms - is decided once per (batch, grid, input form, fused
  soft-argmax, fork set) by the pure function ``v2v_route`` and cached; ``run()`` only reads that table and launches.
  There is no ATen fallback: without ``libsceneego_hip.so`` or off a HIP device it raises.
"""
from __future__ import annotations

import os
from types import MappingProxyType
from typing import Mapping, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib


# A level's skip block is forked onto the side stream when batch x voxels of the level is at most this.  0 = never: measured in
# round 5 (tools/diag/fork_sweep.py, tools/diag/splitk_ab.py; profiles/r05_fork_and_splitk_ab.txt) every fork set is SLOWER than the
# single-stream order on this platform - batch 1: 2.83 -> 3.0-3.2 ms eager, 2.82 -> 3.02 ms as a replayed hipGraph; batch 8: +0.1-0.2 ms -
# a cross-queue dependency costs more than the overlap of the under-filled launches returns.  The capability stays (fork_levels).
FORK_MAX_VOXELS = 0


def _round16(c):
    return (c + 15) // 16 * 16


def _round8(c):
    return (c + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------
# parameter containers (reference key names)
# ------------------------------------------------------------------------------------------------
class Basic3DBlock(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_size):
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv3d(in_planes, out_planes, kernel_size=kernel_size, stride=1, padding=(kernel_size - 1) // 2),
            nn.BatchNorm3d(out_planes), nn.ReLU(True))


class Res3DBlock(nn.Module):
    def __init__(self, in_planes, out_planes):
        super().__init__()
        self.res_branch = nn.Sequential(
            nn.Conv3d(in_planes, out_planes, kernel_size=3, stride=1, padding=1), nn.BatchNorm3d(out_planes),
            nn.ReLU(True),
            nn.Conv3d(out_planes, out_planes, kernel_size=3, stride=1, padding=1), nn.BatchNorm3d(out_planes))
        if in_planes == out_planes:
            self.skip_con = nn.Sequential()
        else:
            self.skip_con = nn.Sequential(nn.Conv3d(in_planes, out_planes, kernel_size=1, stride=1, padding=0),
                                          nn.BatchNorm3d(out_planes))


class Pool3DBlock(nn.Module):
    def __init__(self, pool_size):
        super().__init__()
        assert pool_size == 2
        self.pool_size = pool_size


class Upsample3DBlock(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_size, stride):
        super().__init__()
        assert kernel_size == 2 and stride == 2
        self.block = nn.Sequential(
            nn.ConvTranspose3d(in_planes, out_planes, kernel_size=2, stride=2, padding=0, output_padding=0),
            nn.BatchNorm3d(out_planes), nn.ReLU(True))


# (name, in, out) of the encoder/decoder pyramid: level k works at G / 2^k
_ENC = ((32, 64), (64, 128), (128, 128), (128, 128), (128, 128))
_SKIP = (32, 64, 128, 128, 128)
_DEC_UP = ((64, 32), (128, 64), (128, 128), (128, 128), (128, 128))  # decoder_upsample1..5 (in, out)
_DEC_RES = (64, 128, 128, 128, 128)                                  # decoder_res1..5


class EncoderDecorder(nn.Module):  # (sic) the reference's spelling is part of the checkpoint key names
    def __init__(self):
        super().__init__()
        for k in range(5):
            setattr(self, f"encoder_pool{k + 1}", Pool3DBlock(2))
            setattr(self, f"encoder_res{k + 1}", Res3DBlock(*_ENC[k]))
            setattr(self, f"skip_res{k + 1}", Res3DBlock(_SKIP[k], _SKIP[k]))
            setattr(self, f"decoder_res{k + 1}", Res3DBlock(_DEC_RES[k], _DEC_RES[k]))
            setattr(self, f"decoder_upsample{k + 1}", Upsample3DBlock(_DEC_UP[k][0], _DEC_UP[k][1], 2, 2))
        self.mid_res = Res3DBlock(128, 128)


class V2VModel(nn.Module):
    def __init__(self, input_channels, output_channels):
        super().__init__()
        self.input_channels = input_channels
        self.output_channels = output_channels
        self.front_layers = nn.Sequential(Basic3DBlock(input_channels, 16, 7), Res3DBlock(16, 32),
                                          Res3DBlock(32, 32), Res3DBlock(32, 32))
        self.encoder_decoder = EncoderDecorder()
        self.back_layers = nn.Sequential(Res3DBlock(32, 32), Basic3DBlock(32, 32, 1), Basic3DBlock(32, 32, 1))
        self.output_layer = nn.Conv3d(32, output_channels, kernel_size=1, stride=1, padding=0)
        self._program = None
        self._initialize_weights()

    def _initialize_weights(self):
        # reference v2v.py:172-181
        for m in self.modules():
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                nn.init.xavier_normal_(m.weight)
                nn.init.constant_(m.bias, 0)

    # -- execution ---------------------------------------------------------------------------
    def compile(self, dtype=None, output_scale=1.0, split3=False) -> "V2VProgram":
        """(Re)build the HIP launch program from the current parameters (call after loading weights).
        ``dtype``: torch.float32 (default; parity path) or torch.bfloat16 (bf16 storage, float32 accumulation).
        ``output_scale``: ``run(..., scaled=True)`` returns output_scale * logits (the caller's ``volume_multiplier``,
        reference network/voxel_net_depth.py:271, folded into the output layer); ``forward`` / ``run()`` return the plain logits."""
        self._program = V2VProgram(self, dtype or getattr(self, "program_dtype", torch.float32), output_scale, split3)
        return self._program

    @property
    def program(self) -> "V2VProgram":
        if self._program is None:
            self.compile()
        return self._program

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._program = None

    def _apply(self, fn, *a, **k):
        self._program = None  # .to(device) / .float() invalidate packed weights
        return super()._apply(fn, *a, **k)

    def forward(self, x):
        """Reference signature: ``[B,Cin,G,G,G] -> [B,Cout,G,G,G]`` logits (NCDHW in and out)."""
        _lib.require_hip(x)
        B, C, G = x.shape[0], x.shape[1], x.shape[2]
        prog = self.program
        if prog.fft7_ready(G) and C == prog.cin and G % 32 == 0:
            # NCDHW is the planar input of the frequency-domain front layer as it stands
            return prog.run(x.float().contiguous(), B, G, planar1=True).view(B, self.output_channels, G, G, G)
        buf = torch.zeros((B, G, G, G, prog.cin_pad), device=x.device, dtype=prog.dtype)
        buf[..., :C] = x.permute(0, 2, 3, 4, 1)
        if prog.dtype == torch.bfloat16:
            buf = channels_last_to_octet_planar(buf)
        logits = prog.run(buf, B, G)
        return logits.view(B, self.output_channels, G, G, G)


def channels_last_to_octet_planar(x):
    """[B,G,G,G,C] -> [B,C/8,G,G,G,8]: the input layout of the bf16 7^3 front layer (include/sceneego_hip.h)."""
    B, G, C = x.shape[0], x.shape[1], x.shape[-1]
    return x.view(B, G, G, G, C // 8, 8).permute(0, 4, 1, 2, 3, 5).contiguous()


# ------------------------------------------------------------------------------------------------
# the route: every layout and fused-form decision of one forward, made before anything is launched
# ------------------------------------------------------------------------------------------------
class FrontRoute(NamedTuple):
    fft: bool                   # front_layers.0 in the frequency domain (se_conv3d_k7_fft_f32) or on se_conv3d_f32
    flags: int
    lay_out: Optional[str]      # "quad" / None = channels-last


class BlockRoute(NamedTuple):
    """One Res3DBlock.  Layouts: "quad" [B][C/4][D][D][D][4], "oct" [B][C/8][D][D][D][8], None = channels-last."""
    dim: int
    cin: int
    cout: int
    lay_in: Optional[str]
    lay_out: Optional[str]
    flags1: int                 # complete flag words of the two 3x3x3 launches
    flags2: int
    skip: str                   # "identity" | "conv" (1x1x1 launch) | "skip16" (inside the second launch: se_conv3d_skip16_f32)
    pools: bool                 # the second launch also writes the block's 2x max-pool (se_conv3d_pool_f32)
    variants: Tuple[Optional[int], Optional[int]]   # se_conv3d_f32_variant of both launches (None: bf16 / split-bf16 kernel)


class TailRoute(NamedTuple):
    fused: bool                 # back_layers.1 / .2 / output_layer in one launch, else three se_conv3d_f32 launches
    in_quad: bool
    softargmax: bool            # pass 1 of the soft-argmax rides in the fused launch


class V2VRoute(NamedTuple):
    front0: FrontRoute
    blocks: Mapping[str, BlockRoute]    # front1..3, skip1..5, enc1..5, mid, decres1..5, back0 (the reference's names)
    up: Tuple[int, ...]                 # flag words of decoder_upsample1..5
    fork: frozenset                     # levels (0 = G^3) whose skip block runs on the side stream
    tail: TailRoute
    split6: frozenset = frozenset()     # blocks with a 3x3x3 launch on a six-product bf16 form (csrc/split6.h; se_conv3d_f32_split6)


_BLOCKS = {"front1": (16, 32), "front2": (32, 32), "front3": (32, 32), "mid": (128, 128), "back0": (32, 32)}
for _k in range(5):
    _BLOCKS[f"skip{_k + 1}"] = (_SKIP[_k], _SKIP[_k])
    _BLOCKS[f"enc{_k + 1}"] = _ENC[_k]
    _BLOCKS[f"decres{_k + 1}"] = (_DEC_RES[_k], _DEC_RES[_k])
_LAY = {"quad": (_lib.IN_QUAD, _lib.OUT_QUAD, _lib.RES_QUAD), "oct": (_lib.IN_OCTET, _lib.OUT_OCTET, _lib.RES_OCTET), None: (0, 0, 0)}


def v2v_route(cout, dtype, split3, B, G, input_form="cl", fused_softargmax=False, fork=frozenset(), split6=False) -> V2VRoute:
    """Layouts, flag words and fused forms of one forward of the V2V program: a pure function of these integers and of the library's
    kernel choice (``_lib.conv3d_variant``, a host function).  Nothing is allocated or launched.  ``input_form``: "planar1"
    [B,cin,G,G,G] (frequency-domain front layer), "planar3" (triplet-planar) or "cl" (channels-last; bf16: octet-planar).
    ``split6``: the float32 program packed split planes (SCENEEGO_SPLIT6, on by default): the route records which blocks the library
    then runs on a six-product bf16 form; layouts, flag words and variants are the same either way.

    Tensor layouts of the float32 program: a Res3DBlock output that is read only by 2-D Winograd convolutions of the same kernel
    family (as input or as skip tensor) and by a max-pool is kept in that family's planar layout (quad-planar at 64^3 / 32^3,
    octet-planar at 16^3); what the deconvolutions' inputs, the 1x1x1 convolutions and the unfused tail read stays channels-last.
    The invariants the walk relies on are established here: a violation raises before run() launches anything."""
    if G % 32:
        raise ValueError("volume_size must be a multiple of 32 (five 2x max-pools), got %d" % G)
    f32 = dtype == torch.float32
    split3 = bool(split3) and f32
    # bf16 storage: everything channels-last.  Split-bf16 arithmetic: octet-planar where its kernel runs (D % 16 == 0).  Neither has
    # quad-planar, pooled or fused-skip forms (`forms`); only the plain float32 program asks the library for its layouts.
    forms = f32 and not split3
    R, PRE, POST = _lib.EPI_RELU, _lib.EPI_RES_PRE_RELU, _lib.EPI_RES_POST_RELU

    def variant(ci, co, dim, flags):
        if not f32 or (split3 and dim % 16 == 0):      # a bf16 / split-bf16 kernel runs the launch: not se_conv3d_f32's choice
            return None
        return _lib.conv3d_variant(B, dim, ci, co, 3, flags)

    def kind(name, dim):
        """Planar hand-over layout of a block at this (batch, level): "quad" when both 3x3x3 convolutions run on the F(4,3) x F(4,3)
        kernel (variant 3 with quad flags), "oct" when they run on the F(4,3) x F(2,3) one or on the split-bf16 kernel, None for a
        level with so few voxels that the plain split-K kernel is faster (16^3 at batch 1) and for the levels below."""
        ci, co = _BLOCKS[name]
        if not forms:
            return "oct" if split3 and dim % 16 == 0 else None
        if variant(ci, co, dim, _lib.IN_QUAD) == 3 and variant(co, co, dim, _lib.IN_QUAD) == 3:
            return "quad"
        if variant(ci, co, dim, 0) in (2, 3) and variant(co, co, dim, 0) in (2, 3):
            return "oct"
        return None

    blocks = {}

    def block(name, dim, lay_in, out_planar, pool=False):
        """``out_planar``: the output in the block's own planar layout (if it has one); ``pool``: an encoder max-pool reads it."""
        ci, co = _BLOCKS[name]
        k = kind(name, dim)
        if lay_in not in (None, k):
            raise RuntimeError(f"{name}: {lay_in}-planar input, but its convolutions at {dim}^3, batch {B} take {k or 'channels-last'}")
        IN, OUT, RES = _LAY[k]
        lay_out = k if out_planar else None
        pools = bool(pool and k and forms)
        # the fused 16-channel skip convolution reads channels-last or, in the quad family, the quad-planar tensor the
        # frequency-domain front layer writes (SE_RES_QUAD of se_conv3d_skip16_f32)
        fuse = bool(ci == 16 and forms and k and lay_out and not pools and lay_in in (None, "quad"))
        if ci != co and lay_in and not fuse:
            raise RuntimeError(f"{name}: a 1x1x1 skip convolution reads channels-last, got {lay_in}-planar")
        flags1 = R | OUT | (IN if lay_in else 0)
        if fuse:
            flags2 = R | IN | OUT | (RES if lay_in else 0)
        else:
            flags2 = R | PRE | IN | (RES if lay_in and ci == co else 0) | (OUT if lay_out else 0)
        blocks[name] = BlockRoute(dim, ci, co, lay_in, lay_out, flags1, flags2,
                                  "skip16" if fuse else "conv" if ci != co else "identity", pools,
                                  (variant(ci, co, dim, flags1), variant(co, co, dim, flags2)))
        return blocks[name]

    if input_form == "planar1":
        # quad-planar hand-over when front_layers.1 takes it: both its 3^3 convolutions on the F(4,3) x F(4,3) kernel and the fused
        # 16-channel skip convolution (which then reads the quad-planar tensor too)
        q = kind("front1", G) == "quad"
        front0 = FrontRoute(True, R | (_lib.OUT_QUAD if q else 0), "quad" if q else None)
    else:
        front0 = FrontRoute(False, R | (_lib.IN_PLANAR3 if input_form == "planar3" else 0), None)
    # A block whose output goes to an encoder max-pool writes the pooled tensor from its last convolution's epilogue when that
    # convolution runs on a 2-D Winograd kernel; the pool kernel is then not launched.
    src = front0
    for i in (1, 2, 3):
        src = block(f"front{i}", G, src.lay_out, True, pool=i == 3)
    # Which transposed convolutions write (and read their skip tensor) quad-planar: those in front of a block whose convolutions
    # run on the F(4,3) x F(4,3) kernel (decoder_res1 at 32^3, back_layers.0 at 64^3) and whose shape has that form in
    # se_deconv3d_k2s2_f32; the skip block of that level then writes its output quad-planar as well - whole 16-byte records
    # instead of 64 of every 128 bytes of a channels-last record.
    up_quad = [kind(f"decres{k}" if k else "back0", G >> k) == "quad" and kind(f"skip{k + 1}", G >> k) == "quad"
               and (G >> (k + 1)) % 16 == 0 and _DEC_UP[k] in ((64, 32), (128, 64)) for k in range(5)]
    for k in range(5):
        block(f"skip{k + 1}", G >> k, src.lay_out, up_quad[k])
        if src.lay_out == "quad" and not src.pools:       # there is no quad-planar pool kernel (the octet one: se_maxpool3d_2_octin_f32)
            raise RuntimeError("a quad-planar block output is always pooled by its producer")
        src = block(f"enc{k + 1}", G >> (k + 1), None, True, pool=k < 4)
    if src.lay_out:    # cannot happen: the deepest levels are too small for the 2-D kernels
        raise RuntimeError("planar tensor reached the middle block")
    block("mid", G >> 5, None, False)
    # A decoder / back block whose convolutions run on the F(4,3) x F(4,3) kernel gets its input quad-planar straight from the
    # transposed convolution in front of it; a transposed convolution itself reads channels-last.
    for k in range(5, 0, -1):
        block(f"decres{k}", G >> k, "quad" if k < 5 and up_quad[k] else None, False)
    # the fused tail with the soft-argmax pass reads a quad-planar tensor as well: back_layers.0 then writes whole records
    sa = bool(cout <= 16 and fused_softargmax)
    tail = TailRoute(cout <= 16, sa and kind("back0", G) == "quad", sa)
    block("back0", G, "quad" if up_quad[0] else None, tail.in_quad)
    up = tuple(R | POST | (_lib.OUT_QUAD | _lib.RES_QUAD if q else 0) for q in up_quad)
    s6 = frozenset(n for n, e in blocks.items() if split6 and forms and any(
        _lib.conv3d_split6(B, e.dim, ci, e.cout, 3, fl) for ci, fl in ((e.cin, e.flags1), (e.cout, e.flags2))))
    return V2VRoute(front0, MappingProxyType(blocks), up, frozenset(fork), tail, s6)


# ------------------------------------------------------------------------------------------------
# the launch program
# ------------------------------------------------------------------------------------------------
class _PackedConv:
    __slots__ = ("w", "b", "cin", "cin_pad", "cout", "k", "transposed", "fused", "w_split", "w_split6")

    def __init__(self, conv, bn, cin_pad=None, dtype=torch.float32, scale=1.0, split3=False, split6=False):
        """``scale``: the packed layer computes scale * conv(x) (weights and bias multiplied before packing).
        ``split3`` (float32 3x3x3 layers, experimental): also pack the two bfloat16 halves of the BatchNorm-folded weights for
        se_conv3d_k3_split3_f32."""
        transposed = isinstance(conv, nn.ConvTranspose3d)
        w = conv.weight.detach().float().contiguous()
        if scale != 1.0:
            assert bn is None
            w = w * float(scale)
        dev = w.device
        if transposed:
            cin, cout = w.shape[0], w.shape[1]
            k = 2
        else:
            cout, cin = w.shape[0], w.shape[1]
            k = w.shape[2]
        bf16 = dtype == torch.bfloat16
        self.cin_pad = cin_pad if cin_pad is not None else (_round8(cin) if bf16 else _round16(cin))
        self.cin, self.cout, self.k, self.transposed = cin, cout, k, transposed
        self.fused = None     # 16-channel skip convolution only: (folded weights [cout][16], summed bias) for se_conv3d_skip16_f32
        n = _lib.conv3d_packed_elems(cout, self.cin_pad, k, transposed, bf16=bf16)
        self.w = torch.empty(n, device=dev, dtype=dtype)
        self.b = torch.empty(_round16(cout), device=dev, dtype=torch.float32)
        f = lambda t: None if t is None else t.detach().float().contiguous()
        if bn is not None:
            assert not bn.training, "V2VProgram folds BatchNorm3d running statistics: call .eval() first"
            g, be, mu, var, eps = f(bn.weight), f(bn.bias), f(bn.running_mean), f(bn.running_var), bn.eps
        else:
            g = be = mu = var = None
            eps = 0.0
        bias = f(conv.bias)
        if scale != 1.0 and bias is not None:
            bias = bias * float(scale)
        _lib.conv3d_pack(w, bias, g, be, mu, var, eps, self.w, self.b, cout, cin, self.cin_pad, k, transposed)
        # the six-product bf16 forms of the float32 program (csrc/split6.h): the layer's split planes, hung on self.w for _lib.conv3d
        self.w_split6 = None
        if split6 and not bf16 and not transposed and k == 3 and cout % 32 == 0:
            self.w_split6 = _lib.conv3d_split6_pack(self.w, cout, self.cin_pad, k, transposed)
        self.w_split = None
        if split3 and not bf16 and not transposed and k == 3 and cout % 32 == 0 and self.cin_pad % 8 == 0:
            wf = w if g is None else w * (g / torch.sqrt(var + eps)).view(-1, 1, 1, 1, 1)      # the folding se_conv3d_pack_f32 applies
            self.w_split = _lib.conv3d_split3_pack(wf.contiguous(), cout, cin, self.cin_pad)

class V2VProgram:
    def __init__(self, model: V2VModel, dtype=torch.float32, output_scale=1.0, split3=False):
        assert dtype in (torch.float32, torch.bfloat16)
        self.dtype = dtype
        self.output_scale = float(output_scale)
        # EXPERIMENTAL: float32 tensors, 3x3x3 layers of the 64^3 / 32^3 / 16^3 levels on split-bf16 arithmetic (csrc/conv3d_split.hip)
        self.split3 = bool(split3) and dtype == torch.float32
        # float32 program: the direct-GEMM launches that have a six-product bf16 form (csrc/split6.h) run on it; SCENEEGO_SPLIT6=0
        # packs no split planes, which keeps every launch on its float32 form (A/B)
        self.split6 = dtype == torch.float32 and not self.split3 and os.environ.get("SCENEEGO_SPLIT6", "1") != "0"
        p = next(model.parameters())
        if not p.is_cuda:
            raise _lib.HipExtensionError("V2VModel must live on a HIP device to be compiled (got %s)" % p.device)
        _lib.load()
        self.device = p.device
        self.cout = model.output_channels
        self.cin = model.input_channels
        self.cin_pad = _round8(self.cin) if dtype == torch.bfloat16 else _round16(self.cin)
        fl, ed, bl = model.front_layers, model.encoder_decoder, model.back_layers
        basic = lambda m, cin_pad=None: _PackedConv(m.block[0], m.block[1], cin_pad, dtype)
        self.front0 = basic(fl[0], self.cin_pad)
        # frequency-domain form of the 7^3 front layer (csrc/conv3d_fft7.hip, round 6): the weight spectra in MFMA fragment order.
        # Used when run() gets the planar input [B, cin, G, G, G]; SCENEEGO_FFT7=0 keeps the F(6,7) Winograd kernel (A/B).
        self.front0_fft = None
        self._fft_ws = None
        conv0, bn0 = fl[0].block[0], fl[0].block[1]
        if (dtype == torch.float32 and os.environ.get("SCENEEGO_FFT7", "1") != "0"
                and int(_lib.load().se_conv3d_k7_fft_packed_elems(self.cin, conv0.out_channels)) > 0):
            self.front0_fft = _lib.conv3d_k7_fft_pack(conv0.weight.detach().float().contiguous(), bn0.weight.detach().float().contiguous(),
                                                      bn0.running_var.detach().float().contiguous(), bn0.eps, conv0.out_channels, self.cin)
        self.front_res = [self._pack_res(fl[i]) for i in (1, 2, 3)]
        self.enc = [self._pack_res(getattr(ed, f"encoder_res{k}")) for k in range(1, 6)]
        self.skip = [self._pack_res(getattr(ed, f"skip_res{k}")) for k in range(1, 6)]
        self.dec = [self._pack_res(getattr(ed, f"decoder_res{k}")) for k in range(1, 6)]
        self.up = [basic(getattr(ed, f"decoder_upsample{k}")) for k in range(1, 6)]
        self.mid = self._pack_res(ed.mid_res)
        self.back_res = self._pack_res(bl[0])
        self.back1 = basic(bl[1])
        self.back2 = basic(bl[2])
        self.out = _PackedConv(model.output_layer, None, None, dtype)
        self.out_scaled = self.out if self.output_scale == 1.0 else _PackedConv(model.output_layer, None, None, dtype, scale=self.output_scale)
        # scratch for the split-K path of the small pyramid levels (se_conv3d_f32 workspace): 32 Mi floats.  A workspace serves ONE
        # stream at a time: the forked skip branches (run(), off by default) have their own.
        self.workspace = torch.empty(32 << 20, device=self.device, dtype=torch.float32) if dtype == torch.float32 else None
        self.workspace_side = None
        self._side_stream = None
        self._ws = self.workspace              # the workspace of the stream run() is issuing on
        # skip_res{k+1} of the levels in fork_levels run on a side stream beside the encoder chain (reference network/v2v.py:104-119:
        # skip_x_k = skip_res_k(x) is not read before decoder_upsample_k).  None = decide per batch in run().
        self.fork_levels = None
        # (B, G, input form, fused soft-argmax, fork set) -> V2VRoute.  A route holds the library's kernel choices: a development-library
        # tool that changes the kernel selector under a program that has run must clear this.
        self._routes = {}

    def _pack_res(self, m):
        c1 = _PackedConv(m.res_branch[0], m.res_branch[1], None, self.dtype, split3=self.split3, split6=self.split6)
        c2 = _PackedConv(m.res_branch[3], m.res_branch[4], None, self.dtype, split3=self.split3, split6=self.split6)
        sk = _PackedConv(m.skip_con[0], m.skip_con[1], None, self.dtype) if len(m.skip_con) else None
        if sk is not None and sk.cin == 16 and self.dtype == torch.float32:
            # 16-channel skip convolution (front_layers.1): folded weights [cout][16] + summed bias for se_conv3d_skip16_f32, which
            # computes the skip path inside the second 3x3x3 convolution's launch
            conv, bn = m.skip_con[0], m.skip_con[1]
            scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float()
            sk.fused = ((conv.weight.detach().float().reshape(sk.cout, 16) * scale[:, None]).contiguous(), (c2.b + sk.b).contiguous())
        return (c1, c2, sk)

    # -- primitive launches ------------------------------------------------------------------
    def _new(self, B, dim, c):
        return torch.empty((B, dim, dim, dim, c), device=self.device, dtype=self.dtype)

    def _conv(self, x, pc, B, dim, flags, residual=None, out=None, pool_out=None):
        if out is None:
            out = self._new(B, dim, pc.cout)
        if self.split3 and pc.w_split is not None and dim % 16 == 0 and pool_out is None:
            _lib.conv3d_k3_split3(x, pc.w_split, pc.b, residual, out, B, dim, pc.cin_pad, pc.cout, flags)
            return out
        _lib.conv3d(x, pc.w, pc.b, residual, out, B, dim, pc.cin, pc.cin_pad, pc.cout, pc.k, flags, self._ws, pool_out=pool_out)
        return out

    def _res(self, x, blk, r, B, pool_out=None):
        """Res3DBlock (v2v.py:40-43): relu(bn(conv(relu(bn(conv(x))))) + skip(x)), launched as its route entry ``r`` says.  The tensor
        between the two convolutions is in the block's planar layout whenever it has one; ``pool_out`` (``r.pools``) receives the
        block's 2x max-pool from the second launch."""
        c1, c2, sk = blk
        a = self._conv(x, c1, B, r.dim, r.flags1)
        if r.skip == "skip16":
            out = self._new(B, r.dim, c2.cout)
            _lib.conv3d_skip16(a, c2.w, sk.fused[1], x, sk.fused[0], out, B, r.dim, c2.cin, c2.cout, r.flags2)
            return out
        s = self._conv(x, sk, B, r.dim, 0) if r.skip == "conv" else x
        return self._conv(a, c2, B, r.dim, r.flags2, residual=s, pool_out=pool_out)

    def _fork_set(self, B, G):
        """Levels (0 = G^3 ... 4 = (G/16)^3) whose skip block runs on the side stream: ``fork_levels`` if set, else the levels
        with at most FORK_MAX_VOXELS voxels in the batch (default 0 = none: measured slower, see the constant)."""
        if self.dtype != torch.float32 or self.split3:
            return frozenset()
        if self.fork_levels is not None:
            return frozenset(self.fork_levels)
        env = os.environ.get("SCENEEGO_FORK_LEVELS")          # experiments (tools/diag/fork_sweep.py): "" = none, "0,1,2,3,4" = all
        if env is not None:
            return frozenset(int(t) for t in env.split(",") if t.strip())
        return frozenset(k for k in range(5) if B * (G >> k) ** 3 <= FORK_MAX_VOXELS)

    def _side(self, main):
        if self._side_stream is None:      # first use of the (off by default) fork: outside any graph capture thanks to the warm-up forwards
            self._side_stream = torch.cuda.Stream(device=self.device)
            self.workspace_side = torch.empty_like(self.workspace)
        return self._side_stream

    def _pool(self, x, B, dim, c, x_oct=False):
        out = self._new(B, dim // 2, c)
        _lib.maxpool3d_2(x, out, B, dim, c, in_octet=x_oct)
        return out

    def _up(self, x, pc, skip, B, dim, flags):
        """Upsample3DBlock + decoder add (v2v.py:64-67,124-137): relu(bn(convT(x))) + skip.  With OUT_QUAD | RES_QUAD in ``flags``
        the output is written quad-planar [B][C/4][2D][2D][2D][4] for a block behind it whose convolutions run on the
        F(4,3) x F(4,3) kernel, and ``skip`` is quad-planar too (the skip block wrote whole records)."""
        out = self._new(B, dim * 2, pc.cout)
        _lib.deconv3d_k2s2(x, pc.w, pc.b, skip, out, B, dim, pc.cin_pad, pc.cout, flags)
        return out

    # -- the network -------------------------------------------------------------------------
    def fft7_ready(self, G):
        """True when run(..., planar1=True) can take the planar input [B, cin, G, G, G] (the frequency-domain front layer covers it)."""
        return self.front0_fft is not None and G >= 16 and G % 16 == 0

    def _front0_fft(self, x, B, G, flags):
        """front_layers.0 in the frequency domain (se_conv3d_k7_fft_f32): planar x [B,cin,G,G,G] -> 16 channels, channels-last or (OUT_QUAD)
        quad-planar.  The spectra of up to 8 samples live in a workspace owned by the program (1.5 GB at 64^3; larger batches walk it in
        chunks)."""
        need = _lib.conv3d_k7_fft_workspace_elems(min(B, 8), G, self.cin)
        if self._fft_ws is None or self._fft_ws.numel() < need:
            self._fft_ws = torch.empty(need, device=self.device, dtype=torch.float32)
        out = self._new(B, G, self.front0.cout)
        _lib.conv3d_k7_fft(x, self.front0_fft, self.front0.b, out, B, G, self.cin, self.front0.cout, flags, self._fft_ws)
        return out

    def _route(self, B, G, form, fused_softargmax):
        key = (B, G, form, fused_softargmax, self._fork_set(B, G))
        route = self._routes.get(key)
        if route is None:
            route = self._routes[key] = v2v_route(self.cout, self.dtype, self.split3, *key, split6=self.split6)
        return route

    def run(self, x, B, G, out=None, softargmax=None, scaled=False, planar1=False):
        """x: [B,G,G,G,cin_pad] channels-last (channels >= cin zero; bf16: octet-planar [B,cin_pad/8,G,G,G,8]; float32 may
        also be triplet-planar [B,ceil(cin/3),G,G,G,3], which the 7^3 Winograd front layer reads with ~5x fewer cache-line requests,
        or - ``planar1`` - fully planar [B,cin,G,G,G] for the frequency-domain front layer, see fft7_ready())
        -> planar logits [B,cout,G^3] (``scaled``: times ``output_scale``).
        ``softargmax`` = (coord, scratch): pass 1 of the soft-argmax rides in the fused tail launch."""
        assert x.is_contiguous() and x.dtype == self.dtype
        outc = self.out_scaled if scaled else self.out
        planar3 = self.dtype == torch.float32 and x.dim() == 6       # float32 triplet-planar [B,ceil(cin/3),G,G,G,3]
        if planar1:
            assert self.fft7_ready(G) and tuple(x.shape) == (B, self.cin, G, G, G)
        elif planar3:
            assert tuple(x.shape) == (B, (self.cin + 2) // 3, G, G, G, 3)
        else:
            assert tuple(x.shape) == ((B, self.cin_pad // 8, G, G, G, 8) if self.dtype == torch.bfloat16 else (B, G, G, G, self.cin_pad))
        # every layout, flag word and fused form of this forward (v2v_route): below, only launches
        route = self._route(B, G, "planar1" if planar1 else "planar3" if planar3 else "cl", softargmax is not None)

        def res(name, blk, x):
            r = route.blocks[name]
            pooled = self._new(B, r.dim // 2, r.cout) if r.pools else None
            return self._res(x, blk, r, B, pool_out=pooled), pooled

        if route.front0.fft:
            x = self._front0_fft(x, B, G, route.front0.flags)
        else:
            x = self._conv(x, self.front0, B, G, route.front0.flags)
        for i, blk in enumerate(self.front_res):
            x, pooled = res(f"front{i + 1}", blk, x)
        # encoder (v2v.py:104-119).  skip_res_k(x) is not read before decoder_upsample_k: the skip blocks of the levels in `fork` are
        # issued on a side stream (event fork behind the producer of x, event join in front of the deconvolution that reads the
        # result) and run beside the encoder / middle / decoder chain, which at small batches leaves most of the chip idle
        # (16^3 at batch 1: 32 work units on 256 CUs).  Inside a hipGraph capture the fork and the joins become graph edges.
        skips = []
        joins = [None] * 5
        main = torch.cuda.current_stream(self.device) if route.fork else None
        dim = G
        lay = route.blocks["front3"].lay_out
        for k in range(5):
            if k in route.fork:
                side = self._side(main)
                ev = torch.cuda.Event()
                ev.record(main)
                side.wait_event(ev)
                x.record_stream(side)
                with torch.cuda.stream(side):
                    self._ws = self.workspace_side
                    try:
                        sk = res(f"skip{k + 1}", self.skip[k], x)[0]
                    finally:
                        self._ws = self.workspace
                    joins[k] = torch.cuda.Event()
                    joins[k].record(side)
                sk.record_stream(main)
                skips.append(sk)
            else:
                skips.append(res(f"skip{k + 1}", self.skip[k], x)[0])    # read by the decoder's deconvolution
            # the producer of x wrote its max-pool from its epilogue, or the pool kernel runs (which also reads octet-planar)
            x = pooled if pooled is not None else self._pool(x, B, dim, x.numel() // (B * dim ** 3), x_oct=lay == "oct")
            dim //= 2
            x, pooled = res(f"enc{k + 1}", self.enc[k], x)
            lay = route.blocks[f"enc{k + 1}"].lay_out
        x = res("mid", self.mid, x)[0]
        # decoder (v2v.py:121-137)
        for k in range(4, -1, -1):
            x = res(f"decres{k + 1}", self.dec[k], x)[0]
            if joins[k] is not None:
                main.wait_event(joins[k])
            x = self._up(x, self.up[k], skips[k], B, dim, route.up[k])
            skips[k] = None
            dim *= 2
        # back layers + output (v2v.py:155-161)
        x = res("back0", self.back_res, x)[0]
        if out is None:
            out = torch.empty((B, self.cout, G * G * G), device=self.device, dtype=torch.float32)
        if route.tail.fused:
            # back_layers.1 / .2 / output_layer fused: one read of x, one planar write of the logits
            _lib.pointwise_chain3(x, self.back1, self.back2, outc, out, B, G, softargmax=softargmax if route.tail.softargmax else None,
                                  in_quad=route.tail.in_quad)
            return out
        x = self._conv(x, self.back1, B, G, _lib.EPI_RELU)
        x = self._conv(x, self.back2, B, G, _lib.EPI_RELU)
        _lib.conv3d(x, outc.w, outc.b, None, out, B, G, outc.cin, outc.cin_pad, outc.cout, 1, _lib.EPI_OUT_PLANAR)
        return out
