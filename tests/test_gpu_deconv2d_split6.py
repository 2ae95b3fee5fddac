"""se_deconv2d_k4s2_s6_f32: ConvTranspose2d(k=4, s=2, p=1) + bias (+ ReLU) of the 2-D pose head as one launch whose float32 products
are six bf16 MFMA products each (csrc/deconv2d_k4s2.hip, csrc/split6.h), its packer, its domain and its place in ``FoldedBackbone``.

Reference: ``F.relu(F.conv_transpose2d(x, w, b, stride=2, padding=1))`` in float64 on the CPU.  Gate: max|out - ref| <= 5e-6 * max|ref|
per sample (the gate of tests/test_gpu_split6.py); the float32 route's error on the same data (rocBLAS GEMM +
se_deconv2d_k4s2_assemble_f32) is printed beside it.  A workgroup owns a tile of 8 rows x 16 columns of input positions and 64 output
channels and walks the input channels in chunks of 32 through two LDS buffers: the shapes are the smallest that reach every border and
corner in one workgroup, seams in both directions, one / two / three chunks, one / two cout blocks.  Every case runs on N(0, 1) values
and on a wide dynamic range (magnitudes 2^-20 ... 2^10, exact powers of two and zeros mixed in).
"""
import pytest
import torch
import torch.nn.functional as F

from sceneego_amd import _lib

DEV = "cuda:0"
GATE = 5e-6
pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def wide_range(shape, g):
    """Magnitudes 2^-20 ... 2^10 with random mantissas, 25 % exact powers of two, 10 % exact zeros, random signs."""
    e = torch.randint(-20, 11, shape, generator=g).float()
    m = 1.0 + torch.rand(shape, generator=g)
    m = torch.where(torch.rand(shape, generator=g) < 0.25, torch.ones(()), m)
    v = m * torch.exp2(e) * ((torch.rand(shape, generator=g) < 0.5).float() * 2.0 - 1.0)
    return torch.where(torch.rand(shape, generator=g) < 0.1, torch.zeros(()), v)


class Layer:
    def __init__(self, cin, cout):
        g = _gen(7 * cin + cout)
        self.w = torch.randn((cin, cout, 4, 4), generator=g) / (4 * cin) ** 0.5       # ConvTranspose2d layout, as FoldedBackbone folds it
        self.b = 0.1 * torch.randn(cout, generator=g)
        self.cin, self.cout = cin, cout
        self.wd, self.bd = self.w.to(DEV), self.b.to(DEV)
        self.planes = _lib.deconv2d_k4s2_s6_pack(self.wd)
        self.w_all = self.wd.permute(2, 3, 1, 0).reshape(16 * cout, cin).contiguous()      # the float32 route's GEMM operand


_LAYERS, _CASES = {}, {}


def layer(cin, cout):
    if (cin, cout) not in _LAYERS:
        _LAYERS[(cin, cout)] = Layer(cin, cout)
    return _LAYERS[(cin, cout)]


def f32_route(L, x, relu):
    B, C, H, W = x.shape
    z = torch.matmul(L.w_all, x.reshape(B, C, H * W))
    return _lib.deconv2d_k4s2_assemble(z, L.bd, B, L.cout, H, W, relu=relu)


def case(B, cin, cout, H, W, relu, kind):
    """Input, float64 reference, the split form's output and the float32 route's: computed once, shared, never changed."""
    key = (B, cin, cout, H, W, relu, kind)
    if key not in _CASES:
        L = layer(cin, cout)
        g = _gen(1000 * B + 100 * H + W + cin + (7 if kind == "wide" else 0))
        x = torch.randn((B, cin, H, W), generator=g) if kind == "normal" else wide_range((B, cin, H, W), g)
        if B == 3:
            x[1] *= 2.0 ** 10          # a halo read across a sample boundary lands far outside the gate of samples 0 and 2
        ref = F.conv_transpose2d(x.double(), L.w.double(), L.b.double(), stride=2, padding=1)
        if relu:
            ref = F.relu(ref)
        xd = x.to(DEV)
        out = _lib.deconv2d_k4s2_s6(xd, L.planes, L.bd, cout, relu=relu)
        _CASES[key] = (L, xd, ref, out, f32_route(L, xd, relu))
    return _CASES[key]


# (B, cin, cout, H, W, relu)
SHAPES = [
    pytest.param(1, 32, 64, 8, 16, True, id="one-tile-c32"),            # all four borders and corners in one workgroup; one chunk
    pytest.param(1, 64, 64, 16, 32, False, id="2x2-tiles-c64"),         # seams in both directions; both LDS buffers; no ReLU
    pytest.param(1, 32, 64, 24, 16, True, id="24x16"),                  # not square, W = 16
    pytest.param(1, 96, 128, 8, 48, False, id="8x48-c96-co128"),        # W = 48; a chunk buffer reused; two cout blocks
    pytest.param(1, 256, 256, 8, 16, True, id="production-K"),          # 256 -> 256 at one tile
    pytest.param(3, 64, 64, 16, 16, True, id="B3-scaled-sample"),       # sample 1 scaled by 2^10
]


@pytest.mark.parametrize("kind", ["normal", "wide"])
@pytest.mark.parametrize("B,cin,cout,H,W,relu", SHAPES)
def test_split_form_vs_float64(B, cin, cout, H, W, relu, kind):
    L, x, ref, out, out32 = case(B, cin, cout, H, W, relu, kind)
    assert out.shape == ref.shape and out.dtype == torch.float32
    got, got32 = out.double().cpu(), out32.double().cpu()
    assert not bool(torch.isnan(got).any())
    for s in range(B):
        mx = float(ref[s].abs().max())
        err, err32 = float((got[s] - ref[s]).abs().max()), float((got32[s] - ref[s]).abs().max())
        print(f"\n[{B}x{cin}->{cout} {H}x{W} relu={relu} {kind} sample {s}] split6 {err / mx:.2e}, float32 route {err32 / mx:.2e} of max|ref| {mx:.3e}")
        assert mx > 0 and err <= GATE * mx, f"sample {s}: max|d| {err:.3e} > {GATE} * {mx:.3e}"


@pytest.mark.parametrize("kind", ["normal", "wide"])
def test_launches_repeat_and_samples_do_not_depend_on_the_batch(kind):
    B, cin, cout, H, W, relu = 3, 64, 64, 16, 16, True
    L, x, ref, out, _ = case(B, cin, cout, H, W, relu, kind)
    again = _lib.deconv2d_k4s2_s6(x, L.planes, L.bd, cout, relu=relu)
    assert torch.equal(again, out)
    for s in range(B):
        alone = _lib.deconv2d_k4s2_s6(x[s:s + 1].contiguous(), L.planes, L.bd, cout, relu=relu)
        assert torch.equal(alone[0], out[s]), f"sample {s} alone differs from the batch of {B}: {float((alone[0] - out[s]).abs().max()):.3e}"


def test_assemble_entry_takes_the_split_planes():
    """``deconv2d_k4s2_assemble(x, ..., split6=planes)`` (the call FoldedBackbone makes) is the one-launch form."""
    L, x, ref, out, _ = case(1, 32, 64, 8, 16, True, "normal")
    assert torch.equal(_lib.deconv2d_k4s2_assemble(x, L.bd, 1, 64, 8, 16, relu=True, split6=L.planes), out)


def test_split_planes_sum_to_the_weight():
    cin, cout = 96, 128
    L = layer(cin, cout)
    p = L.planes
    assert p.dtype == torch.bfloat16 and tuple(p.shape) == (cin // 32, cout // 16, 2, 8, 3, 64, 8)
    assert p.numel() == int(_lib.load().se_deconv2d_k4s2_s6_packed_elems(cin, cout))
    # [chunk][tile][a][dy][f][plane][g][row][j] -> [plane][cin][cout][a][dy][f]
    q = p.double().cpu().view(cin // 32, cout // 16, 2, 2, 4, 3, 4, 16, 8).permute(5, 0, 6, 8, 1, 7, 2, 3, 4).reshape(3, cin, cout, 2, 2, 4)
    w = L.w.double()
    want = torch.empty(cin, cout, 2, 2, 4, dtype=torch.float64)
    for a in range(2):
        for dy in range(2):
            for f, kx in enumerate((3, 1, 2, 0)):
                want[:, :, a, dy, f] = w[:, :, 3 - a - 2 * dy, kx]
    assert torch.equal(q[0].float(), want.float().bfloat16().float())                  # plane 0 is bf16(w), round to nearest even
    assert torch.equal(q.sum(0), want), float((q.sum(0) - want).abs().max())          # three 8-bit parts cover the 24 bits: exact
    assert bool((q[1].abs() <= 2.0 ** -8 * want.abs()).all()) and bool((q[2].abs() <= 2.0 ** -16 * want.abs()).all())
    assert _lib.deconv2d_k4s2_s6_pack(torch.zeros(48, 64, 4, 4, device=DEV)) is None


def test_out_of_domain_arguments_are_refused():
    lib = _lib.load()
    L = layer(32, 64)
    bad = -1            # SE_ERR_BAD_ARG
    out = torch.empty(1, 64, 16, 96, device=DEV)

    def launch(x, cin, h, w, elem=None):
        return lib.se_deconv2d_k4s2_s6_f32(_lib._ptr(x), x.element_size() if elem is None else elem, _lib._ptr(L.planes), _lib._ptr(L.bd),
                                           _lib._ptr(out), 1, cin, 64, h, w, 1, _lib._stream())

    assert _lib.deconv2d_k4s2_s6_ok(1, 32, 64, 8, 16) and launch(torch.zeros(1, 32, 8, 16, device=DEV), 32, 8, 16) == 0
    assert not _lib.deconv2d_k4s2_s6_ok(1, 32, 64, 8, 40) and launch(torch.zeros(1, 32, 8, 40, device=DEV), 32, 8, 40) == bad       # W = 40
    assert not _lib.deconv2d_k4s2_s6_ok(1, 48, 64, 8, 16) and launch(torch.zeros(1, 48, 8, 16, device=DEV), 48, 8, 16) == bad       # cin = 48
    assert not _lib.deconv2d_k4s2_s6_ok(1, 32, 64, 4, 16) and not _lib.deconv2d_k4s2_s6_ok(1, 32, 32, 8, 16)
    assert launch(torch.zeros(1, 32, 8, 16, device=DEV, dtype=torch.bfloat16), 32, 8, 16) == bad                                    # bf16 input
    with pytest.raises(_lib.HipExtensionError):
        _lib.deconv2d_k4s2_s6(torch.zeros(1, 32, 8, 16, device=DEV, dtype=torch.bfloat16), L.planes, L.bd, 64)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# through FoldedBackbone (128 x 128, B = 2: the last transposed layer is 256 -> 256 on 16 x 16 maps, two tiles per sample)
# ------------------------------------------------------------------------------------------------
def _backbone_inputs():
    import test_gpu_backbone_routes as R
    return R, R._net(), R._image(2, 128, 128)


def test_backbone_features_with_the_split_form(monkeypatch):
    """The routing threshold is lowered so that this small map takes the new form (the default asks for one workgroup per CU).
    Bar per sample, against the float64 chain: three times the error of the same backbone with the layer on its float32 route (the
    rest of the chain is the same launches; 3x leaves room for the roundings falling differently) plus the layer's own gate,
    5e-6 * max|ref| - and never above the chain bar of tests/test_gpu_backbone_routes.py."""
    from sceneego_amd.pose_resnet import FoldedBackbone
    R, net, img = _backbone_inputs()
    monkeypatch.delenv("SCENEEGO_DECONV_S6", raising=False)
    fb = FoldedBackbone(net)
    fb.deconv_s6_min_wg = 0
    calls = []
    orig = _lib.deconv2d_k4s2_s6
    monkeypatch.setattr(_lib, "deconv2d_k4s2_s6", lambda x, *a, **k: (calls.append(tuple(x.shape)), orig(x, *a, **k))[1])
    with torch.no_grad():
        feats = fb(img.to(DEV)).double().cpu()
        assert calls == [(2, 256, 16, 16)], calls          # 4 x 4 and 8 x 8 maps are outside the domain (W % 16): rocBLAS + assembly
        feats32 = FoldedBackbone(net)(img.to(DEV)).double().cpu()      # default threshold: every transposed layer on GEMM + assembly
    assert len(calls) == 1
    want = R.chain64(R._params64(), img.double())
    for s in range(2):
        mx = float(want[s].abs().max())
        err, err32 = float((feats[s] - want[s]).abs().max()), float((feats32[s] - want[s]).abs().max())
        print(f"\n[backbone 128x128 B2 sample {s}] features against the float64 chain: split form {err / mx:.2e}, float32 route {err32 / mx:.2e} of max|ref|")
        assert err <= min(3.0 * err32 + GATE * mx, R.CHAIN_TOL * mx + R.CHAIN_ABS)


def test_backbone_knob_off_is_the_gemm_route_bit_for_bit(monkeypatch):
    from sceneego_amd.pose_resnet import FoldedBackbone
    R, net, img = _backbone_inputs()
    monkeypatch.setenv("SCENEEGO_DECONV_S6", "0")
    monkeypatch.setenv("SCENEEGO_DECONV_S6_MIN_WG", "0")
    fb = FoldedBackbone(net)

    def refuse(*a, **k):
        raise AssertionError("se_deconv2d_k4s2_s6_f32 reached with SCENEEGO_DECONV_S6=0")
    monkeypatch.setattr(_lib, "deconv2d_k4s2_s6", refuse)
    taps = []
    o_dg = FoldedBackbone._deconv_gemm
    monkeypatch.setattr(FoldedBackbone, "_deconv_gemm", lambda self, li, x, b: (taps.append((li, x.clone())), o_dg(self, li, x, b))[1])
    with torch.no_grad():
        feats = fb(img.to(DEV))
    assert [t[0] for t in taps] == [0, 1, 2]
    x = taps[0][1]                      # the route of the transposed layers before the split form: one GEMM + the assembly pass each
    for w, b in fb.ups:
        B, C, H, W = x.shape
        w_all = w.permute(2, 3, 1, 0).reshape(16 * w.shape[1], C).contiguous()
        x = _lib.deconv2d_k4s2_assemble(torch.matmul(w_all, x.reshape(B, C, H * W)), b, B, w.shape[1], H, W, relu=True)
    assert torch.equal(feats, x)
