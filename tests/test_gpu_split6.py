"""The six-product bf16 forms of the float32 program (csrc/split6.h): split planes, the split form of the 3x3x3 kernel of the
8^3-sized levels, its place in the plan and the SCENEEGO_SPLIT6 knob.

References are float64 on the host, computed from the UNFOLDED weights with BatchNorm folded in float64.  Every case runs on two
inputs: N(0, 1) values, and a wide dynamic range - magnitudes 2^-20 ... 2^10 (1e-6 ... 1e3) mixed in one tensor, a quarter of them
exact powers of two, a tenth exact zeros, both signs (the skip tensor too).  Gate of the form: max|out - ref| <= 5e-6 * max|ref|,
``GATE_OTHER`` of tests/test_gpu_v2v_routes.py; the float32 form's error on the same data is printed beside it.
"""
import pytest
import torch
import torch.nn.functional as F

from sceneego_amd import _lib

DEV = "cuda:0"
GATE_OTHER = 5e-6
R, PRE, POST = _lib.EPI_RELU, _lib.EPI_RES_PRE_RELU, _lib.EPI_RES_POST_RELU
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


def _values(kind, shape, g):
    return torch.randn(shape, generator=g) if kind == "normal" else wide_range(shape, g)


class Layer:
    """Conv3d / ConvTranspose3d + BatchNorm3d: float32 parameters, the packed float32 buffer, its split planes, the float64 fold."""

    def __init__(self, cout, cin, k, transposed, seed):
        g = _gen(seed)
        taps = 8 if transposed else k ** 3
        shape = (cin, cout) + (2,) * 3 if transposed else (cout, cin) + (k,) * 3
        self.w = torch.randn(shape, generator=g) / (taps * cin) ** 0.5
        self.b = 0.1 * torch.randn(cout, generator=g)
        self.gamma, self.var = 0.5 + torch.rand(cout, generator=g), 0.5 + torch.rand(cout, generator=g)
        self.beta, self.mean = 0.1 * torch.randn(cout, generator=g), 0.1 * torch.randn(cout, generator=g)
        self.eps = 1e-5
        self.cout, self.cin, self.k, self.transposed, self.taps = cout, cin, k, transposed, taps
        d = lambda t: t.to(DEV)
        self.wpack = torch.empty(_lib.conv3d_packed_elems(cout, cin, k, transposed), device=DEV)
        self.bpack = torch.empty((cout + 15) // 16 * 16, device=DEV)
        _lib.conv3d_pack(d(self.w), d(self.b), d(self.gamma), d(self.beta), d(self.mean), d(self.var), self.eps, self.wpack, self.bpack,
                         cout, cin, cin, k, transposed)
        self.wpack_f32 = self.wpack.clone()           # no split planes hung on it: _lib.conv3d keeps the float32 forms
        self.wsplit = _lib.conv3d_split6_pack(self.wpack, cout, cin, k, transposed)
        # the fold in float64
        scale = self.gamma.double() / torch.sqrt(self.var.double() + self.eps)
        self.w64 = self.w.double() * (scale.view(1, -1, 1, 1, 1) if transposed else scale.view(-1, 1, 1, 1, 1))
        self.b64 = (self.b.double() - self.mean.double()) * scale + self.beta.double()

    def folded_f32(self):
        """[cout, cin, taps]: the folded float32 weights as section A of the packed buffer holds them ([cg][tap][nt][h][row][j])."""
        nts, cgs = (self.cout + 15) // 16, self.cin // 16
        a = self.wpack_f32[:self.taps * cgs * nts * 256].view(cgs, self.taps, nts, 4, 16, 4)
        return a.permute(2, 4, 0, 3, 5, 1).reshape(nts * 16, cgs * 16, self.taps)

    def planes(self):
        """[3, cout, cin, taps] from the split buffer ([sg][tap][nt][plane][g][row][j])."""
        nts, sgs = (self.cout + 15) // 16, self.cin // 32
        s = self.wsplit.view(sgs, self.taps, nts, 3, 4, 16, 8)
        return s.permute(3, 2, 5, 0, 4, 6, 1).reshape(3, nts * 16, sgs * 32, self.taps)


_LAYERS = {}


def layer(cout, cin, k=3, transposed=False, tag=0):
    key = (cout, cin, k, transposed, tag)
    if key not in _LAYERS:
        _LAYERS[key] = Layer(cout, cin, k, transposed, seed=100 + cout + 7 * cin + k + 1000 * tag)
    return _LAYERS[key]


# ------------------------------------------------------------------------------------------------
# split planes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,cin,k,transposed", [(128, 128, 3, False), (32, 64, 2, True)], ids=["128x128x27", "64x32x8-transposed"])
def test_split_planes_sum_to_the_folded_weight(cout, cin, k, transposed):
    L = layer(cout, cin, k, transposed)
    assert L.wsplit.numel() == L.taps * (cin // 32) * (cout // 16) * 3 * 512 and L.wsplit.dtype == torch.bfloat16
    w = L.folded_f32().double()
    p = L.planes().double()
    assert float(w.abs().max()) > 0 and torch.equal(p[0].float(), w.float().bfloat16().float())        # plane 0 is bf16(w), RNE
    err = (p.sum(0) - w).abs()
    assert bool((err <= 2.0 ** -26 * w.abs()).all()), float((err / w.abs().clamp_min(1e-300)).max())
    # and the folded float32 weight is the float64 fold to one rounding (the planes describe the layer, not something else)
    w64 = L.w64.permute(1, 0, 2, 3, 4).reshape(cout, cin, 8) if transposed else L.w64.reshape(cout, cin, k ** 3)
    assert bool(((w.cpu() - w64).abs() <= 2.0 ** -22 * w64.abs()).all())
    assert _lib.conv3d_split6_pack(torch.empty(_lib.conv3d_packed_elems(32, 16, 3, False), device=DEV), 32, 16, 3) is None   # cin_pad % 32


@pytest.mark.parametrize("kind", ["normal", "wide"])
def test_device_split_of_activations(kind):
    x = _values(kind, (3, 8 * 8 * 8 * 128), _gen(5)).to(DEV)
    p = _lib.split6_planes(x).double().view(3, *x.shape)
    xd = x.double()
    assert torch.equal(p[0].float(), x.bfloat16().float())
    err = (p.sum(0) - xd).abs()
    assert bool((err <= 2.0 ** -26 * xd.abs()).all()), float(err.max())
    assert bool((p[1].abs() <= 2.0 ** -8 * xd.abs()).all()) and bool((p[2].abs() <= 2.0 ** -16 * xd.abs()).all())


# ------------------------------------------------------------------------------------------------
# the 8^3 form
# ------------------------------------------------------------------------------------------------
SHAPES = [(8, 1), (8, 3), (16, 1)]
VARIANTS = {"plain": (0, False), "skip-relu": (R | PRE, True), "relu-skip": (R | POST, True)}
_CASES = {}


def case(dim, B, ch, kind, variant):
    """Input, skip tensor, float64 reference, the split form's output and the float32 form's - computed once, shared, never changed."""
    key = (dim, B, ch, kind, variant)
    if key not in _CASES:
        L = layer(ch, ch)
        flags, has_res = VARIANTS[variant]
        g = _gen(1000 * dim + 100 * B + ch + (7 if kind == "wide" else 0))
        x = _values(kind, (B, dim, dim, dim, ch), g)
        res = _values(kind, (B, dim, dim, dim, ch), g) if has_res else None
        ref = F.conv3d(x.double().permute(0, 4, 1, 2, 3), L.w64, L.b64, padding=1)
        if flags & PRE:
            ref = ref + res.double().permute(0, 4, 1, 2, 3)
        if flags & R:
            ref = ref.clamp_min(0)
        if flags & POST:
            ref = ref + res.double().permute(0, 4, 1, 2, 3)
        ref = ref.permute(0, 2, 3, 4, 1).contiguous()
        xd, rd = x.to(DEV), None if res is None else res.to(DEV)
        out = torch.full((B, dim, dim, dim, ch), float("nan"), device=DEV)
        _lib.conv3d_k3_split6(xd, L.wsplit, L.bpack, rd, out, B, dim, ch, ch, ch, flags)
        f32 = torch.full_like(out, float("nan"))
        ws = torch.empty(27 * B * dim ** 3 * ch, device=DEV)
        _lib.conv3d(xd, L.wpack_f32, L.bpack, rd, f32, B, dim, ch, ch, ch, 3, flags, ws)
        torch.cuda.synchronize()
        _CASES[key] = (xd, rd, ref, out, f32)
    return _CASES[key]


@pytest.mark.parametrize("variant", ["plain", "skip-relu"])
@pytest.mark.parametrize("kind", ["normal", "wide"])
@pytest.mark.parametrize("ch", [128, 64])
@pytest.mark.parametrize("dim,B", SHAPES)
def test_halo64_split_form_vs_float64(dim, B, ch, kind, variant):
    _, _, ref, out, f32 = case(dim, B, ch, kind, variant)
    mx = float(ref.abs().max())
    err, err32 = float((out.double().cpu() - ref).abs().max()), float((f32.double().cpu() - ref).abs().max())
    print(f"\nsplit6 halo64 dim {dim} B {B} {ch}->{ch} {kind} {variant}: split form {err / mx:.2e}, float32 form {err32 / mx:.2e} of max|ref| {mx:.3e}")
    assert err32 <= GATE_OTHER * mx                   # the reference and the data are sound
    assert err <= GATE_OTHER * mx, (err / mx, err32 / mx)


def test_halo64_split_form_post_relu_skip():
    _, _, ref, out, _ = case(8, 3, 128, "wide", "relu-skip")
    assert float((out.double().cpu() - ref).abs().max()) <= GATE_OTHER * float(ref.abs().max())


@pytest.mark.parametrize("dim,ch", [(8, 128), (16, 64)])
def test_halo64_split_form_is_deterministic_and_batch_invariant(dim, ch):
    B = 3 if dim == 8 else 2
    L = layer(ch, ch)
    g = _gen(31 + dim)
    x, res = wide_range((B, dim, dim, dim, ch), g).to(DEV), torch.randn((B, dim, dim, dim, ch), generator=g).to(DEV)

    def run(xi, ri, n):
        o = torch.full((n, dim, dim, dim, ch), float("nan"), device=DEV)
        _lib.conv3d_k3_split6(xi, L.wsplit, L.bpack, ri, o, n, dim, ch, ch, ch, R | PRE)
        return o

    a, b = run(x, res, B), run(x, res, B)
    assert not bool(torch.isnan(a).any()) and torch.equal(a, b)
    for s in range(B):
        assert torch.equal(run(x[s:s + 1].contiguous(), res[s:s + 1].contiguous(), 1)[0], a[s]), s


def test_plan_routes_the_split_form_and_declines_outside_its_domain():
    """>= 2048 voxels at dim 8 / 16 with 32-channel stages: _lib.conv3d on a buffer with split planes runs the split form (the direct
    entry point's output, bit for bit), on one without them the float32 form; the query says which."""
    assert _lib.conv3d_split6(8, 8, 128, 128, 3, R) and _lib.conv3d_split6(4, 8, 128, 128, 3, R | PRE) and _lib.conv3d_split6(1, 16, 64, 64, 3, 0)
    assert not _lib.conv3d_split6(1, 8, 128, 128, 3, R) and not _lib.conv3d_split6(3, 8, 128, 128, 3, R)      # < 2048 voxels
    assert not _lib.conv3d_split6(8, 4, 128, 128, 3, R) and not _lib.conv3d_split6(8, 16, 128, 128, 3, R)     # 4^3; 16^3 x 8: 2-D Winograd
    assert not _lib.conv3d_split6(8, 8, 16, 32, 3, R) and not _lib.conv3d_split6(8, 8, 128, 128, 1, R)        # 16 channels; 1x1x1
    assert _lib.conv3d_variant(8, 8, 128, 128, 3, R) == 0
    L = layer(128, 128)
    B, dim = 4, 8
    g = _gen(77)
    x, res = torch.randn((B, dim, dim, dim, 128), generator=g).to(DEV), torch.randn((B, dim, dim, dim, 128), generator=g).to(DEV)
    ws = torch.empty(1 << 20, device=DEV)
    outs = []
    for wpack in (L.wpack, L.wpack_f32):
        o = torch.full((B, dim, dim, dim, 128), float("nan"), device=DEV)
        _lib.conv3d(x, wpack, L.bpack, res, o, B, dim, 128, 128, 128, 3, R | PRE, ws)
        outs.append(o)
    direct = torch.full_like(outs[0], float("nan"))
    _lib.conv3d_k3_split6(x, L.wsplit, L.bpack, res, direct, B, dim, 128, 128, 128, R | PRE)
    assert torch.equal(outs[0], direct) and not torch.equal(outs[0], outs[1])
    assert float((outs[0] - outs[1]).abs().max()) <= 2 * GATE_OTHER * float(outs[1].abs().max())
    # outside the form's domain the direct entry point launches nothing
    lib = _lib.load()
    p = x.data_ptr()
    assert lib.se_conv3d_k3_split6_f32(p, p, p, None, p, 1, 4, 128, 128, 128, 0, None) == -1       # dim 4
    assert lib.se_conv3d_k3_split6_f32(p, p, p, None, p, 1, 8, 48, 48, 128, 0, None) == -1         # cin % 32
    assert lib.se_conv3d_k3_split6_f32(p, p, p, None, p, 1, 8, 128, 128, 48, 0, None) == -1        # cout % 32
    assert lib.se_conv3d_k3_split6_f32(p, p, p, None, p, 17, 8, 128, 128, 128, 0, None) == -1      # > 8192 voxels
    assert lib.se_conv3d_k3_split6_f32(p, p, p, None, p, 1, 8, 128, 128, 128, 8, None) == -1       # planar output


# ------------------------------------------------------------------------------------------------
# the knob
# ------------------------------------------------------------------------------------------------
def test_knob_off_keeps_every_launch_on_its_float32_form(monkeypatch):
    """SCENEEGO_SPLIT6=0: no split planes are packed, the route names no split block and is otherwise the same record, and no launch
    goes through se_conv3d_w6_f32 - every convolution is the se_conv3d_f32 call of the program without split forms.  With the knob on
    (the default) the 8^3-level blocks of a B = 8 forward at G = 32 run on the split form, and the logits agree."""
    from sceneego_amd.v2v import V2VModel, _PackedConv
    G, B = 32, 8
    torch.manual_seed(11)
    model = V2VModel(33, 15).to(DEV).eval()
    x = torch.randn(B, 33, G, G, G, device=DEV)
    lib = _lib.load()
    calls = []
    orig = lib.se_conv3d_w6_f32
    monkeypatch.setattr(lib, "se_conv3d_w6_f32", lambda *a: (calls.append(a[7]), orig(*a))[1])      # a[7]: dim
    coord = torch.zeros(G ** 3, 3, device=DEV)
    scratch = torch.empty(_lib.softargmax3d_scratch_elems(B * 15), device=DEV)
    logits, routes = {}, {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SCENEEGO_SPLIT6", knob)
        prog = model.compile()
        packed = [pc for blk in prog.front_res + prog.enc + prog.skip + prog.dec + [prog.mid, prog.back_res] for pc in blk if isinstance(pc, _PackedConv)]
        assert prog.split6 == (knob == "1")
        assert all((pc.w_split6 is not None) == (knob == "1" and pc.k == 3 and pc.cin_pad % 32 == 0) for pc in packed)
        assert all((getattr(pc.w, "split6", None) is not None) == (pc.w_split6 is not None) for pc in packed)
        del calls[:]
        logits[knob] = prog.run(x, B, G, softargmax=(coord, scratch), planar1=True).clone()
        torch.cuda.synchronize()
        (routes[knob],) = prog._routes.values()
        if knob == "0":
            assert not calls and routes[knob].split6 == frozenset()
        else:
            assert routes[knob].split6 == {"skip3", "enc2", "decres2"} and calls.count(8) == 6, (routes[knob].split6, calls)
    assert routes["0"][:5] == routes["1"][:5]
    mx = float(logits["0"].abs().max())       # 1e-4: the bar the chained logits are held to against float64 (tests/test_gpu_v2v_routes.py)
    assert not torch.equal(logits["0"], logits["1"]) and float((logits["0"] - logits["1"]).abs().max()) <= 1e-4 * mx
