"""CPU: the float64 interval model of a bf16-storage launch (tests/bf16_launch_model.py) over the case matrix of the GPU tests.

For every case: a correct implementation - torch-CPU float32 on the identical operands, ONE round to nearest even - lies inside
its interval; the factor g of the interval is at least 4 x what that reference needs; at most 10 % of the elements have lo != hi;
and the comparison REJECTS what a subtly wrong kernel would produce: truncation instead of round-to-nearest-even, one weight tap
zeroed, one weight off by one bf16 ulp, PRE and POST residual swapped, ReLU dropped, the output rotated by one voxel or by one
channel octet.  The wrong outputs are built from the float32 accumulator, i.e. they are otherwise exact.

Two rejections are asserted only where the mutation can show.  "One weight off by one bf16 ulp" moves an output by 2^-8 |w x|, a
small fraction of the output's own bf16 spacing when K is large, so it shows as a flipped rounding in about that fraction of the
elements: the mutant is built for the cases with at least 4096 output elements, NOT for the one- and few-voxel cases (3^3 at B1 / B5
D1 and B1 D2, the 1x1x1 D1 cases, the transposed B2 D1 cases).  PRE / POST swapped and ReLU dropped need a ReLU (and a skip tensor);
the rotation by a voxel needs more than one.  Every other mutant is built for every case.
"""
import pytest
import torch

import bf16_launch_cases as C
import bf16_launch_model as M

BF = torch.bfloat16
R, PRE, POST = M.EPI_RELU, M.EPI_RES_PRE_RELU, M.EPI_RES_POST_RELU
torch.set_num_threads(min(16, torch.get_num_threads()))
IDS = [c.id for c in C.LAUNCH_CASES]


def _store(acc, c, o, flags=None):
    """epilogue + ONE round to nearest even of a float32 accumulator (torch's float32 -> bfloat16 conversion)"""
    return M.epilogue(acc, o.res, c.flags if flags is None else flags).to(BF)


@pytest.mark.parametrize("c", C.LAUNCH_CASES, ids=IDS)
def test_float32_reference_inside_interval_and_cap(c):
    o, ref = C.operands(c), C.reference(c)
    got = _store(ref.acc32, c, o)
    bad = M.outside(got, ref.interval)
    share = M.straddle_share(ref.interval)
    lo_n, hi_n = M.on_edge(got, ref.interval)
    print(f"{c.id}: K={c.K} g_ref={ref.g_ref:.2f} g={ref.g:g} straddle={100 * share:.2f}% on_lo={lo_n} on_hi={hi_n} "
          f"kernel={C.case_kernel(c)} reference {ref.seconds:.2f}s")
    assert not bool(bad.any()), (c.id, int(bad.sum()))
    assert share <= M.STRADDLE_CAP, (c.id, share)
    assert bool((ref.lo.double() <= ref.hi.double()).all())


def test_factor_g_is_four_times_the_reference():
    """g = 4 x the largest g_ref over the matrix, rounded up to a power of two: the constant in the model is not below that.
    g_ref is a property of torch-CPU's float32 summation and so of the host and its thread count: 3.75 and 3.91 were measured on two
    machines (profiles/bf16_launch_parity.txt), both for the 64-term 1x1x1 case with 5 M outputs, where the maximum over so many
    elements of a 64-step rounding walk is taken.  A torch build whose order gives more than 4.0 fails here on purpose: by the rule
    g is then 32, and G_FACTOR, the straddle shares and the device ratio (measured 2.0, bar g / 4) have to be re-derived with it,
    not this assertion loosened."""
    worst = max(C.reference(c).g_ref for c in C.LAUNCH_CASES)
    for cout3, B, dim in ((15, 1, 16), (16, 2, 6)):
        o, cm = C.chain_operands(cout3, B, dim), C.chain_reference(cout3, B, dim)
        ratio, n = M.device_ratio(M.chain_float32(C.rows(o.x), *o.wb), cm)
        assert n > 0
        worst = max(worst, ratio)
    print(f"largest g_ref {worst:.2f} -> g = {M.pow2_ceil(4 * worst):g} (model: {M.G_FACTOR:g})")
    assert M.pow2_ceil(4.0 * worst) <= M.G_FACTOR, f"g_ref {worst:.2f} on this host: the rule gives g = {M.pow2_ceil(4.0 * worst):g}, re-derive G_FACTOR"
    assert M.g_of(16) == 16.0 and M.g_of(8) == 10.0


def test_bf16_rne_matches_the_format():
    v = torch.tensor([1.0, 1.00390625, 1.005859375, 1.01171875, -1.00390625, 257.0, 0.0, 3.0e-39, 2.0 ** -133 * 1.5], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0078125, 1.015625, -1.0, 256.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    got = M.bf16_rne(v)
    assert torch.equal(got[:7], want[:7])
    assert float(got[8]) == 2.0 ** -132                     # tie between 2^-133 and 2^-132: to even
    x = torch.randn(100000, generator=torch.Generator().manual_seed(1)) * torch.tensor(10.0) ** torch.randint(-30, 30, (100000,))
    assert torch.equal(M.bf16_rne(x.double()), x.to(BF).double())         # float32 inputs: torch's own conversion
    t = M.bf16_truncate(x)
    assert bool((t.abs() <= x.abs()).all()) and torch.equal(t.to(BF).float(), t)


# ------------------------------------------------------------------------------------------------
# what the comparison must reject
# ------------------------------------------------------------------------------------------------
def _tap(c, o, co, ci):
    """Contribution of weight (co, ci, centre tap; transposed: parity 0) to output channel co: (index of its outputs, value)."""
    if c.transposed:
        return (slice(None), co, slice(0, None, 2), slice(0, None, 2), slice(0, None, 2)), o.w[ci, co, 0, 0, 0], o.x[:, ci]
    h = c.k // 2
    return (slice(None), co), o.w[co, ci, h, h, h], o.x[:, ci]


def _mutants(c, o, ref):
    acc = ref.acc32
    yield "truncation", M.bf16_truncate(M.epilogue(acc, o.res, c.flags))
    a = acc.clone()
    for co in range(c.cout):        # the slot (input channel 0, centre tap) dropped, as a packer or a k loop would drop it: for every cout
        idx, w, x = _tap(c, o, co, 0)
        a[idx] -= w * x
    yield "tap_zeroed", _store(a, c, o)
    if acc.numel() >= 4096:
        # one bf16 ulp of a weight moves an output by 2^-8 |w x|, a small fraction of the OUTPUT's bf16 spacing when K is large: it
        # shows as a flipped rounding in about that fraction of the elements, so the case must have enough of them
        a = acc.clone()
        for co in range(c.cout):
            idx, w, x = _tap(c, o, co, 0)
            a[idx] += float(M.bf16_ulp(w)) * x
        yield "weight_ulp", _store(a, c, o)
    if c.flags & R and o.res is not None:
        yield "pre_post_swapped", _store(acc, c, o, c.flags ^ (PRE | POST))
    if c.flags & R:
        yield "relu_dropped", _store(acc, c, o, c.flags & ~R)
    good = _store(acc, c, o)
    if c.B * c.dim_out ** 3 > 1:
        v = good.permute(1, 0, 2, 3, 4).reshape(c.cout, -1).roll(1, 1)
        yield "rotated_voxel", v.reshape(c.cout, c.B, *good.shape[2:]).permute(1, 0, 2, 3, 4)
    yield "rotated_octet", good.roll(8, 1)


@pytest.mark.parametrize("c", C.LAUNCH_CASES, ids=IDS)
def test_comparison_rejects_wrong_kernels(c):
    o, ref = C.operands(c), C.reference(c)
    iv = ref.interval
    names = []
    for name, got in _mutants(c, o, ref):
        n = int(M.outside(got, iv).sum())
        names.append(f"{name} {n}")
        assert n > 0, f"{c.id}: the comparison accepts '{name}'"
    print(f"{c.id}: elements outside of {ref.lo.numel()}: " + ", ".join(names))
    nan = _store(ref.acc32, c, o).clone()
    nan.view(-1)[nan.numel() // 2] = float("nan")
    assert int(M.outside(nan, iv).sum()) == 1


# ------------------------------------------------------------------------------------------------
# the fused tail
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.CHAIN_CASES, ids=[c.id for c in C.CHAIN_CASES])
def test_chain_reference_inside_interval_and_cap(c):
    o, cm = C.chain_operands(c.cout, c.B, c.dim), C.chain_reference(c.cout, c.B, c.dim)
    got = M.chain_float32(C.rows(o.x), *o.wb)
    assert not bool(M.outside(got, cm.logits).any())
    s1, s2 = M.straddle_share(cm.h1), M.straddle_share(cm.h2)
    ratio, n = M.device_ratio(got, cm)
    print(f"{c.id}: hidden straddle {100 * s1:.2f}% / {100 * s2:.2f}%, {n} of {got.shape[0]} voxels determined, float32 ratio {ratio:.2f}")
    assert s1 <= M.STRADDLE_CAP and s2 <= M.STRADDLE_CAP


@pytest.mark.parametrize("cout3,B,dim", [(15, 1, 16), (16, 2, 6)])
def test_chain_comparison_rejects_wrong_kernels(cout3, B, dim):
    """(3 voxels of the (3, 1) shape cannot tell a rounding mode apart; the two larger shapes must.)"""
    o, cm = C.chain_operands(cout3, B, dim), C.chain_reference(cout3, B, dim)
    x = C.rows(o.x)
    w1, b1, w2, b2, w3, b3 = o.wb
    r = lambda t: t.to(BF).float()
    tr = M.bf16_truncate
    relu = torch.relu
    good = M.chain_float32(x, *o.wb)
    w2z = w2.clone()
    w2z[5, 7] = 0.0
    w3u = w3.clone()
    w3u[:, 0] += M.bf16_ulp(w3[:, 0]).float()
    mutants = {
        "truncation": tr(relu(tr(relu(x @ w1.T + b1)) @ w2.T + b2)) @ w3.T + b3,
        "tap_zeroed": M.chain_float32(x, w1, b1, w2z, b2, w3, b3),
        "weight_ulp": M.chain_float32(x, w1, b1, w2, b2, w3u, b3),
        "relu_dropped": r(relu(r(x @ w1.T + b1) @ w2.T + b2)) @ w3.T + b3,
        "rotated_voxel": good.roll(1, 0),
        "rotated_joint": good.roll(1, 1),
    }
    for name, got in mutants.items():
        assert int(M.outside(got, cm.logits).sum()) > 0, f"the chain comparison accepts '{name}'"


def test_box_reference_equals_the_whole_volume():
    """The optional crop: a box plus halo, the volume's own border keeping its zero padding, gives the whole volume's values."""
    gen = torch.Generator().manual_seed(5)
    for k, cin, cout in ((3, 16, 32), (7, 8, 16), (1, 16, 32)):
        x = torch.randn((1, cin, 12, 12, 12), generator=gen).to(BF).double()
        w = torch.randn((cout, cin, k, k, k), generator=gen).to(BF).double()
        b = torch.randn(cout, generator=gen).double()
        y, S = M.exact(x, w, b, k)
        for box in (((0, 6), (0, 6), (0, 6)), ((6, 12), (2, 8), (5, 12))):
            yb, Sb = M.exact(x, w, b, k, box=box)
            (z0, z1), (y0, y1), (x0, x1) = box
            for full, part in ((y, yb), (S, Sb)):
                want = full[:, :, z0:z1, y0:y1, x0:x1]
                assert float((part - want).abs().max()) <= 1e-13 * float(want.abs().max())
    x = torch.randn((1, 32, 6, 6, 6), generator=gen).to(BF).double()
    w = torch.randn((32, 32, 2, 2, 2), generator=gen).to(BF).double()
    y, _ = M.exact(x, w, torch.zeros(32), 2, transposed=True)
    yb, _ = M.exact(x, w, torch.zeros(32), 2, transposed=True, box=((4, 12), (0, 6), (2, 8)))
    assert torch.equal(yb, y[:, :, 4:12, 0:6, 2:8])
    # the slab form of the convolution is the same operator
    keep = M._IM2COL_BYTES
    try:
        xs = torch.randn((1, 8, 10, 9, 9), generator=gen).double()
        ws = torch.randn((16, 8, 3, 3, 3), generator=gen).double()
        want = M.conv3d(xs, ws, None, 3)
        M._IM2COL_BYTES = 1 << 16
        got = M.conv3d(xs, ws, None, 3)
    finally:
        M._IM2COL_BYTES = keep
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_case_matrix_reaches_every_kernel():
    """The dispatcher's rules, restated in bf16_launch_cases.kernel_of: the launch cases cover every convolution and transposed
    convolution kernel and every split-K / transposed instantiation the dispatcher can choose."""
    seen = {C.case_kernel(c) for c in C.LAUNCH_CASES}
    want = {"conv_bf16_k3_splitk_kernel<1,4>", "conv_bf16_k3_splitk_kernel<2,4>", "conv_bf16_k3_kernel<8>", "conv_bf16_k7r_kernel",
            "conv_bf16_k7_kernel<false>", "conv_bf16_direct_kernel<1>", "conv_bf16_direct_kernel<3>", "conv_bf16_direct_kernel<7>",
            "deconv_bf16_kernel<1>", "deconv_bf16_kernel<2>", "deconv_bf16_kernel<3>", "deconv_bf16_kernel<4>"}
    assert want <= seen, want - seen
    assert C.case_kernel(C.Case("conv", 64, 8, 16, 32, 3, R)) == "conv_bf16_k3_splitk_kernel<2,4>"        # 32768 voxels: the last split-K shape
    assert C.case_kernel(C.Case("conv", 65, 8, 16, 32, 3, R)) == "conv_bf16_direct_kernel<3>"
    assert C.case_kernel(C.Case("conv", 10, 6, 128, 128, 3, R)) == "conv_bf16_k3_splitk_kernel<2,4>"      # 135 tiles
    assert C.case_kernel(C.Case("conv", 3, 6, 128, 128, 3, R)) == "conv_bf16_k3_splitk_kernel<1,4>"
