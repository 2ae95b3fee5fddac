"""Per-layer float64 parity of the 2D backbone over the launch routes ``FoldedBackbone._call_fused`` can take.

``_call_fused`` picks, layer by layer, between the HIP kernels (``se_conv2d_1x1_f32`` with 64- / 128-channel tiles, its small-M form, the
stride-2 forms, ``se_conv2d_3x3_f32`` / ``_s2_f32``, the fused stem tail, one GEMM + ``se_deconv2d_k4s2_assemble_f32``) and MIOpen followed
by ``se_bias_act_nchw_f32``, from the batch, the map size and the channel counts.  The kernel tests check each kernel alone; this module
checks what the executor composes from them.  A recorder wraps ``_pw`` / ``_pw_s2`` / ``_c3`` / ``_deconv_gemm``, the ``_lib`` entry points
they reach and ``F.conv2d`` / ``F.conv_transpose2d`` / ``F.max_pool2d`` as ``pose_resnet`` sees them, and keeps for the checked samples
every layer's input, residual, ``in_bias``, ``relu`` flag, output and the route (entry points in call order, tile of the packed weights).
Each tap is compared with a float64 evaluation of that one layer (reference network/pose_resnet.py ``Bottleneck`` :52-90, ``PoseResNet``
:135-246, BatchNorm folded in float64 from the formula) fed the HIP run's own input tap: 1e-5 * max|ref| for a tap of a HIP kernel, a
measured gate for a tap that went through MIOpen / rocBLAS; the fused stem tail must equal its float32 expression bit for bit; the final
features are compared with a float64 run of the whole chain at 1e-4 * max + 1e-5.  The reference of a layer comes from its slot (which
convolution of which Bottleneck), never from the flags the executor passed, and the shortcut of a conv3 is the tap the block started from.
"""
import collections
import types

import pytest
import torch
import torch.nn.functional as F

from sceneego_amd import _lib, pose_resnet
from sceneego_amd.pose_resnet import FoldedBackbone

from conftest import synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAP_TOL = 1e-5          # max|hip - ref| <= TAP_TOL * max|ref| per layer (the bar of the 2-D kernel tests in tests/test_gpu_kernels.py)
# Regression gates of the taps that went through MIOpen / rocBLAS, of max|ref| (5x the largest value measured on MI355X over the matrix,
# rounded up to one digit; none may exceed GATE_CAP, the whole-backbone bar):
GATE_CAP = 1e-4
GATE_STEM = 3e-6            # the 7x7 stride-2 stem convolution on MIOpen: measured 4.6e-7 (128 x 128, B=8)
GATE_MIOPEN_1X1 = 9e-6      # 1x1 layers on MIOpen + bias_act_nchw, stride 1 (with / without the in_bias pass) and 2: measured 1.8e-6 (256 x 256, B=32)
GATE_MIOPEN_3X3 = 4e-6      # 3x3 layers on MIOpen, stride 1 and 2: measured 7.3e-7 (264 x 264, B=1)
GATE_TAIL_FALLBACK = 2e-7   # bias_act_nchw + max_pool2d after the stem (one float32 rounding): measured 3.0e-8 (264 x 264, B=1)
GATE_DECONV_GEMM = 9e-6     # rocBLAS GEMM + se_deconv2d_k4s2_assemble_f32: measured 1.7e-6 (512 x 512, B=1)
GATE_DECONV_MIOPEN = 7e-6   # conv_transpose2d on MIOpen + bias_act_nchw: measured 1.2e-6 (256 x 256, B=32)
CHAIN_TOL = 1e-4        # final features against the float64 chain: CHAIN_TOL * max|ref| + CHAIN_ABS (test_bias_act_and_fused_backbone)
CHAIN_ABS = 1e-5
BN_EPS = 1e-5           # nn.BatchNorm2d's default (reference network/pose_resnet.py builds every BatchNorm2d without an eps)

torch.set_num_threads(min(16, torch.get_num_threads()))


# ------------------------------------------------------------------------------------------------
# float64 references (CPU)
# ------------------------------------------------------------------------------------------------
_P64 = {}


def _params64():
    """Every convolution of the backbone with its BatchNorm folded in float64: w' = w * gamma / sqrt(var + eps) per output channel,
    b' = beta - mean * gamma / sqrt(var + eps).  The layer table is read off the state dict's keys."""
    if _P64:
        return _P64
    sd = {k[len("backbone."):]: v.double() for k, v in synthetic_state_dict(False).items()
          if k.startswith("backbone.") and v.is_floating_point()}

    def fold(conv, bn, transposed=False):
        scale = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + BN_EPS)
        shift = sd[bn + ".bias"] - sd[bn + ".running_mean"] * scale
        w = sd[conv + ".weight"]          # Conv2d: [cout, cin, kh, kw]; ConvTranspose2d: [cin, cout, kh, kw]
        return w * (scale.view(1, -1, 1, 1) if transposed else scale.view(-1, 1, 1, 1)), shift

    blocks = []
    for si in range(1, 5):
        bi = 0
        while f"layer{si}.{bi}.conv1.weight" in sd:
            p = f"layer{si}.{bi}"
            stride = 2 if (si > 1 and bi == 0) else 1          # the first Bottleneck of layer2..4 carries the stride (on conv2 and downsample)
            ds = fold(p + ".downsample.0", p + ".downsample.1") if p + ".downsample.0.weight" in sd else None
            blocks.append(types.SimpleNamespace(c1=fold(p + ".conv1", p + ".bn1"), c2=fold(p + ".conv2", p + ".bn2"),
                                                c3=fold(p + ".conv3", p + ".bn3"), ds=ds, stride=stride, name=p))
            bi += 1
    ups = []
    while f"deconv_layers.{3 * len(ups)}.weight" in sd:
        i = 3 * len(ups)
        ups.append(fold(f"deconv_layers.{i}", f"deconv_layers.{i + 1}", transposed=True))
    _P64.update(stem=fold("conv1", "bn1"), blocks=blocks, ups=ups)
    assert len(blocks) == 16 and len(ups) == 3
    return _P64


def _bias(b):
    return b.view(1, -1, 1, 1)


def _conv1x1(x, w):
    return torch.einsum("oc,bchw->bohw", w[:, :, 0, 0], x)


def ref_stem(P, x):
    return F.conv2d(x, P["stem"][0], None, stride=2, padding=3)


def ref_tail(P, x):
    return F.max_pool2d(F.relu(x + _bias(P["stem"][1])), 3, 2, 1)


def ref_conv1(blk, x):
    return F.relu(_conv1x1(x, blk.c1[0]) + _bias(blk.c1[1]))


def ref_conv2(blk, x):
    """The raw 3x3 sums: bn2's bias and the ReLU belong to conv3's launch."""
    return F.conv2d(x, blk.c2[0], None, stride=blk.stride, padding=1)


def ref_conv3(blk, x, shortcut):
    return F.relu(_conv1x1(F.relu(x + _bias(blk.c2[1])), blk.c3[0]) + _bias(blk.c3[1]) + shortcut)


def ref_downsample(blk, x):
    s = blk.stride
    return _conv1x1(x[:, :, ::s, ::s], blk.ds[0]) + _bias(blk.ds[1])


def ref_up(P, li, x):
    w, b = P["ups"][li]
    return F.relu(F.conv_transpose2d(x, w, b, stride=2, padding=1))


def chain64(P, img):
    """The whole backbone in float64 from the image (reference PoseResNet.forward's ``features``)."""
    x = ref_tail(P, ref_stem(P, img))
    for blk in P["blocks"]:
        sc = x if blk.ds is None else ref_downsample(blk, x)
        x = ref_conv3(blk, ref_conv2(blk, ref_conv1(blk, x)), sc)
    for li in range(len(P["ups"])):
        x = ref_up(P, li, x)
    return x


# ------------------------------------------------------------------------------------------------
# the recorder (test side only: monkeypatch on FoldedBackbone, _lib and pose_resnet.F)
# ------------------------------------------------------------------------------------------------
_LIB_TAGS = {           # entry point -> its tag in a layer's route; packed kernels carry the tile read from the packed weight's shape
    "conv2d_1x1": lambda a: f"conv2d_1x1:{a[1].shape[2]}",
    "conv2d_1x1_small": lambda a: f"conv2d_1x1_small:{a[1].shape[2]}",
    "conv2d_1x1_s2": lambda a: f"conv2d_1x1_s2:{a[1].shape[2]}",
    "conv2d_3x3": lambda a: f"conv2d_3x3:{a[1].shape[3]}",
    "conv2d_3x3_s2": lambda a: f"conv2d_3x3_s2:{a[1].shape[3]}",
    "bias_act_nchw": lambda a: "bias_act_nchw",
    "bias_relu_maxpool": lambda a: "bias_relu_maxpool",
    "deconv2d_k4s2_assemble": lambda a: "deconv2d_k4s2_assemble",
}


class Recorder:
    """``layers``: one dict per layer call of the last forward, in call order - slot ("stem", "tail", (block, 0..3) with 0 = downsample,
    ("up", i)), kind, x / residual / out of the checked samples (copies: ``bias_act_nchw`` works in place), in_bias, relu, calls."""

    def __init__(self, monkeypatch):
        self.sel, self.layers, self.cur = [0], [], None
        rec = self
        o_pw, o_pw_s2, o_c3, o_dg = FoldedBackbone._pw, FoldedBackbone._pw_s2, FoldedBackbone._c3, FoldedBackbone._deconv_gemm

        def _pw(fb, x, wb, residual, relu, slot, in_bias=None):
            L = rec._open("pw", slot, x, residual=residual, in_bias=in_bias, relu=relu)
            return rec._close(L, o_pw(fb, x, wb, residual, relu, slot, in_bias=in_bias))

        def _pw_s2(fb, x, wb, slot):
            L = rec._open("pw_s2", slot, x)
            return rec._close(L, o_pw_s2(fb, x, wb, slot))

        def _c3(fb, x, wb, stride, slot):
            L = rec._open("c3", slot, x)
            return rec._close(L, o_c3(fb, x, wb, stride, slot))

        def _deconv_gemm(fb, li, x, bias):
            L = rec._open("up", ("up", li), x)
            return rec._close(L, o_dg(fb, li, x, bias))

        for n, f in (("_pw", _pw), ("_pw_s2", _pw_s2), ("_c3", _c3), ("_deconv_gemm", _deconv_gemm)):
            monkeypatch.setattr(FoldedBackbone, n, f)
        for n, tag in _LIB_TAGS.items():
            monkeypatch.setattr(_lib, n, self._wrap(getattr(_lib, n), n, tag))
        proxy = types.SimpleNamespace(**{n: getattr(F, n) for n in dir(F) if not n.startswith("__")})
        for n in ("conv2d", "conv_transpose2d", "max_pool2d"):
            setattr(proxy, n, self._wrap(getattr(F, n), "F." + n, lambda a, n=n: "F." + n))
        monkeypatch.setattr(pose_resnet, "F", proxy)

    def _wrap(self, orig, name, tag):
        rec = self

        def f(*a, **k):
            rec._enter(name, tag(a), a)
            out = orig(*a, **k)
            if rec.cur is not None and rec.cur["closes"] == name:
                rec._close(rec.cur, out)
            return out
        return f

    def _enter(self, name, tag, a):
        """A call outside _pw / _pw_s2 / _c3 / _deconv_gemm opens the layer of ``_call_fused`` it belongs to: the stem convolution, the stem
        tail (fused, or bias_act + max_pool2d) and the MIOpen route of a transposed layer (conv_transpose2d + bias_act)."""
        if self.cur is None:
            if name == "F.conv2d" and not self.layers:
                self._open("stem", "stem", a[0], closes=name)
            elif name == "bias_relu_maxpool":
                self._open("tail", "tail", a[0], closes=name, bias=a[1])
            elif name == "bias_act_nchw" and self.layers and self.layers[-1]["kind"] == "stem":
                self._open("tail", "tail", a[0], closes="F.max_pool2d", bias=a[1])
            elif name == "F.conv_transpose2d":
                self._open("up", ("up", sum(L["kind"] == "up" for L in self.layers)), a[0], closes="bias_act_nchw")
            else:
                raise AssertionError(f"{name} called outside any layer after {[L['slot'] for L in self.layers[-2:]]}")
        self.cur["calls"].append(tag)

    def _take(self, t):
        return None if t is None else t[self.sel].clone()

    def _open(self, kind, slot, x, residual=None, in_bias=None, relu=None, closes=None, bias=None):
        assert self.cur is None, f"layer {slot} opened inside {self.cur['slot']}"
        self.cur = dict(kind=kind, slot=slot, x=self._take(x), residual=self._take(residual), in_bias=in_bias, relu=relu, calls=[],
                        closes=closes, bias=bias, shape=tuple(x.shape))
        return self.cur

    def _close(self, L, out):
        assert self.cur is L
        L["out"] = self._take(out)
        self.layers.append(L)
        self.cur = None
        return out

    def run(self, fb, img, sel):
        """One forward; returns (layers, features of the checked samples)."""
        self.sel, self.layers, self.cur = list(sel), [], None
        with torch.no_grad():
            feats = fb(img)
        torch.cuda.synchronize()
        assert self.cur is None
        return self.layers, feats[self.sel].clone()


# route of a layer: (name for the census and the coverage test, detail, HIP kernel?, gate family).  The detail is for the census only:
# k groups of se_conv2d_1x1_f32 (two from 128 input channels on), tile width of the 3x3 kernels (8 pixels where the map's width is no
# multiple of 16)
def _route(L):
    k, c = L["kind"], tuple(L["calls"])
    r = None
    if k == "stem" and c == ("F.conv2d",):
        r = ("stem miopen", "", False, "stem")
    elif k == "tail":
        if c == ("bias_relu_maxpool",):
            r = ("tail fused", "", True, None)
        elif c == ("bias_act_nchw", "F.max_pool2d"):
            r = ("tail fallback", "", False, "tail_fallback")
    elif k == "pw":
        if c in (("conv2d_1x1:64",), ("conv2d_1x1:128",)):
            r = ("1x1 tile" + c[0].split(":")[1], "k2" if L["shape"][1] >= 128 else "k1", True, None)
        elif c == ("conv2d_1x1_small:16",):
            r = ("1x1 small", "", True, None)
        elif c == ("F.conv2d", "bias_act_nchw") and L["in_bias"] is None:
            r = ("1x1 miopen", "", False, "miopen_1x1")
        elif c == ("bias_act_nchw", "F.conv2d", "bias_act_nchw") and L["in_bias"] is not None:
            r = ("1x1 miopen+in_bias", "", False, "miopen_1x1")
    elif k == "pw_s2":
        if c in (("conv2d_1x1_s2:64",), ("conv2d_1x1_s2:128",)):
            r = ("1x1s2 tiled", "tile" + c[0].split(":")[1], True, None)
        elif c == ("conv2d_1x1_s2:16",):
            r = ("1x1s2 small", "", True, None)
        elif c == ("F.conv2d", "bias_act_nchw"):
            r = ("1x1s2 miopen", "", False, "miopen_1x1")
    elif k == "c3":
        if c in (("conv2d_3x3:16",), ("conv2d_3x3:32",)):
            r = ("3x3 tile" + c[0].split(":")[1], "w8" if L["shape"][3] % 16 else "w16", True, None)
        elif c == ("conv2d_3x3_s2:16",):
            r = ("3x3s2 hip", "w8" if (L["shape"][3] // 2) % 16 else "w16", True, None)
        elif c == ("F.conv2d",):
            r = ("3x3 miopen" if L["x"].shape[2:] == L["out"].shape[2:] else "3x3s2 miopen", "", False, "miopen_3x3")
    elif k == "up":
        if c == ("deconv2d_k4s2_assemble",):
            r = ("up gemm", "", False, "deconv_gemm")       # rocBLAS product in front of the assembly kernel: gated as a library tap
        elif c == ("F.conv_transpose2d", "bias_act_nchw"):
            r = ("up miopen", "", False, "deconv_miopen")
    assert r is not None, f"layer {L['slot']} ({k}) took an unknown route {c} (in_bias {'set' if L['in_bias'] is not None else 'None'})"
    return r


def _gates():
    return {"stem": GATE_STEM, "miopen_1x1": GATE_MIOPEN_1X1, "miopen_3x3": GATE_MIOPEN_3X3, "tail_fallback": GATE_TAIL_FALLBACK,
            "deconv_gemm": GATE_DECONV_GEMM, "deconv_miopen": GATE_DECONV_MIOPEN}


def tap_tolerance(L):
    hip, fam = _route(L)[2:]
    return TAP_TOL if hip else _gates()[fam]


def tap_error(got, ref):
    """(max|got - ref|, max|ref|) of one sample."""
    return float((got - ref).abs().max()), float(ref.abs().max())


def tap_ok(got, ref, tol):
    err, mx = tap_error(got, ref)
    return err <= tol * mx


# ------------------------------------------------------------------------------------------------
# one matrix point
# ------------------------------------------------------------------------------------------------
SEEN = {"routes": collections.OrderedDict(), "family": {}, "chain": collections.OrderedDict(), "points": set()}
_NET = {}
_B2 = {}


def _net():
    if not _NET:
        sd = {k[len("backbone."):]: v for k, v in synthetic_state_dict(False).items() if k.startswith("backbone.")}
        net = pose_resnet.PoseResNet()
        net.load_state_dict(sd, strict=True)
        _NET["net"] = net.to(DEV).eval()
    return _NET["net"]


def _image(B, H, W):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1000 * B + H + 3 * W))


def _slots(P):
    want = ["stem", "tail"]
    for bi, blk in enumerate(P["blocks"]):
        want += [(bi, 1), (bi, 2)] + ([(bi, 0)] if blk.ds is not None else []) + [(bi, 3)]
    return want + [("up", li) for li in range(len(P["ups"]))]


def layer_ref(P, by, L):
    """float64 reference of layer ``L`` from the HIP run's own input tap (all checked samples)."""
    slot = L["slot"]
    x = L["x"].double().cpu()
    if slot == "stem":
        return ref_stem(P, x)
    if slot == "tail":
        return ref_tail(P, x)
    if slot[0] == "up":
        return ref_up(P, slot[1], x)
    bi, j = slot
    blk = P["blocks"][bi]
    if j == 0:
        return ref_downsample(blk, x)
    if j == 1:
        return ref_conv1(blk, x)
    if j == 2:
        return ref_conv2(blk, x)
    shortcut = by[(bi, 0)]["out"] if blk.ds is not None else by[(bi, 1)]["x"]
    return ref_conv3(blk, x, shortcut.double().cpu())


def check_wiring(P, by, feats, label):
    """The taps chain as the network does, bit for bit: what one layer wrote is what the next one read."""
    pairs = [("tail", "x", "stem", "out"), ((0, 1), "x", "tail", "out")]
    for bi, blk in enumerate(P["blocks"]):
        pairs += [((bi, 2), "x", (bi, 1), "out"), ((bi, 3), "x", (bi, 2), "out")]
        pairs.append(((bi, 3), "residual", (bi, 0), "out") if blk.ds is not None else ((bi, 3), "residual", (bi, 1), "x"))
        if blk.ds is not None:
            pairs.append(((bi, 0), "x", (bi, 1), "x"))
        pairs.append(((bi + 1, 1) if bi + 1 < len(P["blocks"]) else ("up", 0), "x", (bi, 3), "out"))
    pairs += [(("up", li + 1), "x", ("up", li), "out") for li in range(len(P["ups"]) - 1)]
    for a, ka, b, kb in pairs:
        assert torch.equal(by[a][ka], by[b][kb]), f"{label}: {ka} of {a} is not {kb} of {b}"
    assert torch.equal(feats, by[("up", len(P["ups"]) - 1)]["out"]), f"{label}: the features are not the last layer's output"


def check_point(layers, feats, img, sel, label, only_library=False):
    """Compare every recorded layer of every checked sample with its float64 reference; ``only_library``: only the taps that went through
    MIOpen / rocBLAS (the second visit of a shape, whose HIP taps are compared bit for bit with the first)."""
    P = _params64()
    assert [L["slot"] for L in layers] == _slots(P), f"{label}: layers recorded {[L['slot'] for L in layers]}"
    by = {L["slot"]: L for L in layers}
    check_wiring(P, by, feats, label)
    census, fails, worst = collections.Counter(), [], {}
    for L in layers:
        name, detail, hip, fam = _route(L)
        census[(name, detail)] += 1
        assert not bool(torch.isnan(L["out"]).any()), f"{label}: NaN in {L['slot']} ({name})"
        if only_library and hip:
            continue
        tol = tap_tolerance(L)
        assert tol <= GATE_CAP
        ref = layer_ref(P, by, L)
        got = L["out"].double().cpu()
        assert got.shape == ref.shape, f"{label}: {L['slot']} ({name}) has shape {tuple(got.shape)}, the reference {tuple(ref.shape)}"
        for s in range(len(sel)):
            err, mx = tap_error(got[s], ref[s])
            assert mx > 0, f"{label}: the reference of {L['slot']} is all zero - dead activations check nothing"
            key = name if hip else "library:" + fam
            worst[key] = max(worst.get(key, 0.0), err / mx)
            if not err <= tol * mx:
                fails.append(f"{label} layer {L['slot']} sample {sel[s]} ({name} {detail}, input {L['shape']}): max|d| {err:.3e} > {tol} * {mx:.3e}")
        if name == "tail fused":        # max is exact and relu(. + b) monotone: the float32 expression, bit for bit
            want = F.max_pool2d(F.relu(L["x"] + _bias(L["bias"])), 3, 2, 1)
            if not torch.equal(L["out"], want):
                fails.append(f"{label} fused stem tail differs from max_pool2d(relu(x + b), 3, 2, 1): {float((L['out'] - want).abs().max()):.3e}")
    if not only_library:
        want = chain64(P, img[list(sel)].double())
        got = feats.double().cpu()
        for s in range(len(sel)):
            err, mx = tap_error(got[s], want[s])
            SEEN["chain"][label] = max(SEEN["chain"].get(label, 0.0), err / mx)
            if not err <= CHAIN_TOL * mx + CHAIN_ABS:
                fails.append(f"{label} features of sample {sel[s]} against the float64 chain: {err:.3e} > {CHAIN_TOL} * {mx:.3e} + {CHAIN_ABS}")
    for key, v in worst.items():
        SEEN["family"][key] = max(SEEN["family"].get(key, 0.0), v)
    SEEN["routes"][label] = census
    print(f"\n[{label}] " + ", ".join(f"{' '.join(n).strip()} x{c}" for n, c in sorted(census.items())))
    print("    worst tap / max|ref|: " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(worst.items()))
          + (f"; chain {SEEN['chain'][label]:.1e}" if not only_library else ""))
    assert not fails, "\n".join(fails)
    SEEN["points"].add(label)


def _sel(B):
    return tuple(range(B)) if B <= 2 else (0, B - 1)


def _label(H, W, B):
    return f"{H}x{W} B{B}"


WALK = (8, 1, 32, 2)
# (H, W, B): what each row is for is in the comments; which route a layer takes follows FoldedBackbone._pw / _pw_s2 / _c3 / _call_fused,
# se_conv2d_1x1_tile_f32 and se_conv2d_3x3_tile_f32 (workgroups against the CU count)
ROWS = [
    pytest.param(256, 256, 4, id="256x256-B4"),     # between the small-M and the tiled forms
    pytest.param(128, 128, 1, id="128x128-B1"),     # layer4 at 4 x 4 = 16 pixels: conv3 on MIOpen with an in_bias pass of its own, 3x3 on MIOpen
    pytest.param(128, 128, 8, id="128x128-B8"),     # ... and 128 pixels: tiles that straddle samples
    pytest.param(512, 512, 1, id="512x512-B1"),     # layer1's 3x3 above CONV3X3_MAX_PIXELS (MIOpen), its 1x1 layers on HIP
    pytest.param(256, 320, 2, id="256x320-B2"),     # not square: layer4 at 8 x 10 - 3x3 refused by the tile rule, 1x1 accepted with hw = 80
    pytest.param(264, 264, 1, id="264x264-B1"),     # stem output 132 wide, every hw fails & 15, odd maps into the stride-2 layers: all fallbacks
]


def test_backbone_layers_vs_float64_batch_walk(monkeypatch):
    """256 x 256 at B = 8, 1, 32, 2 and 8 again on ONE FoldedBackbone: the plans (per layer and input shape) and the packed weights
    (per layer and tile) serve changing shapes; the second B = 8 run must repeat the first bit for bit on every HIP tap."""
    rec = Recorder(monkeypatch)
    fb = FoldedBackbone(_net())
    first = None
    for B in WALK:
        img = _image(B, 256, 256)
        layers, feats = rec.run(fb, img.to(DEV), _sel(B))
        if B == WALK[0]:
            first = (img, layers, feats)
        if B == 2:
            _B2.update(layers=layers, feats=feats)
        check_point(layers, feats, img, _sel(B), _label(256, 256, B))
    img, layers0, _ = first
    layers, feats = rec.run(fb, img.to(DEV), _sel(WALK[0]))
    assert [(_route(L)[:2], L["calls"]) for L in layers] == [(_route(L)[:2], L["calls"]) for L in layers0]
    for L0, L in zip(layers0, layers):
        if _route(L)[2]:
            assert torch.equal(L["x"], L0["x"]) and torch.equal(L["out"], L0["out"]), \
                f"second B={WALK[0]} run: layer {L['slot']} ({_route(L)[0]}) differs from the first run: input " \
                f"{float((L['x'] - L0['x']).abs().max()):.3e}, output {float((L['out'] - L0['out']).abs().max()):.3e}"
    check_point(layers, feats, img, _sel(WALK[0]), _label(256, 256, WALK[0]) + " again", only_library=True)


@pytest.mark.parametrize("H,W,B", ROWS)
def test_backbone_layers_vs_float64(H, W, B, monkeypatch):
    rec = Recorder(monkeypatch)
    img = _image(B, H, W)
    layers, feats = rec.run(FoldedBackbone(_net()), img.to(DEV), _sel(B))
    check_point(layers, feats, img, _sel(B), _label(H, W, B))


# what the matrix must reach; a routing change that empties a route fails here instead of silently shrinking what the module checks
REQUIRED_ROUTES = ("1x1 tile64", "1x1 tile128", "1x1 small", "1x1 miopen", "1x1 miopen+in_bias",
                   "1x1s2 tiled", "1x1s2 small", "1x1s2 miopen",
                   "3x3 tile16", "3x3 tile32", "3x3 miopen", "3x3s2 hip", "3x3s2 miopen",
                   "tail fused", "tail fallback", "up gemm", "up miopen")


def test_backbone_sensitivity_of_the_comparison(monkeypatch):
    """The comparison rejects wrong layers: the taps of the 256 x 256 B = 2 run against deliberately wrong references (only the
    reference is altered; nothing is launched to make it fail), each next to the right reference, which passes."""
    if not _B2:
        img = _image(2, 256, 256)
        layers, feats = Recorder(monkeypatch).run(FoldedBackbone(_net()), img.to(DEV), (0, 1))
        _B2.update(layers=layers, feats=feats)
    P = _params64()
    by = {L["slot"]: L for L in _B2["layers"]}

    def tap(slot):
        L = by[slot]
        return L, L["x"].double().cpu(), L["out"].double().cpu(), tap_tolerance(L)

    def rejects(slot, got, good, bad, tol, what):
        for s in range(got.shape[0]):
            assert tap_ok(got[s], good[s], tol), f"{slot} sample {s}: the right reference fails"
            assert not tap_ok(got[s], bad[s], tol), f"{slot} sample {s}: a reference with {what} passes the bar {tol}"

    for bi in (0, 4, 15):       # identity and downsample shortcuts, first and last stage
        blk = P["blocks"][bi]
        # conv3 without in_bias
        L, x, got, tol = tap((bi, 3))
        sc = (by[(bi, 0)]["out"] if blk.ds is not None else by[(bi, 1)]["x"]).double().cpu()
        bad = F.relu(_conv1x1(F.relu(x), blk.c3[0]) + _bias(blk.c3[1]) + sc)
        rejects((bi, 3), got, ref_conv3(blk, x, sc), bad, tol, "no in_bias")
        # conv2 with its bias added
        L, x, got, tol = tap((bi, 2))
        good = ref_conv2(blk, x)
        rejects((bi, 2), got, good, good + _bias(blk.c2[1]), tol, "bn2's bias added")
        # one border row of the 3x3 with replicate padding instead of zero padding
        alt = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), blk.c2[0], None, stride=blk.stride)
        for row in (0, -1):
            if blk.stride == 2 and row == -1:
                continue            # an even map at stride 2 never reads the bottom padding
            bad = good.clone()
            bad[:, :, row] = alt[:, :, row]
            rejects((bi, 2), got, good, bad, tol, f"replicate padding in row {row}")
        # a 1x1 reference with two output channels swapped
        L, x, got, tol = tap((bi, 1))
        good = ref_conv1(blk, x)
        bad = good.clone()
        bad[:, [3, 4]] = good[:, [4, 3]]
        rejects((bi, 1), got, good, bad, tol, "output channels 3 and 4 swapped")
    # the stride-2 downsample reading the odd pixels
    for bi, blk in enumerate(P["blocks"]):
        if blk.ds is not None and blk.stride == 2:
            L, x, got, tol = tap((bi, 0))
            bad = _conv1x1(x[:, :, 1::2, 1::2], blk.ds[0]) + _bias(blk.ds[1])
            rejects((bi, 0), got, ref_downsample(blk, x), bad, tol, "the odd pixels")


def test_backbone_route_matrix_coverage():
    """The matrix above must reach every route of every layer kind (runs after it; asserted over the whole module)."""
    want = {_label(256, 256, B) for B in WALK} | {_label(256, 256, WALK[0]) + " again"} | {_label(*p.values) for p in ROWS}
    if not want <= SEEN["points"]:
        pytest.skip("coverage is asserted over the whole matrix; run the module without a selection")
    seen = collections.Counter()
    for census in SEEN["routes"].values():
        for (name, _), n in census.items():
            seen[name] += n
    print("\nroutes over the matrix: " + ", ".join(f"{n} x{c}" for n, c in sorted(seen.items())))
    print("worst tap / max|ref| per family: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(SEEN["family"].items())))
    print("chain / max|ref| per row: " + ", ".join(f"{k} {v:.2e}" for k, v in SEEN["chain"].items()))
    missing = [r for r in REQUIRED_ROUTES if not seen[r]]
    assert not missing, f"routes the matrix never took: {missing}; seen {dict(seen)}"
