"""``sceneego_amd.v2v.v2v_route``: the layouts, flag words and fused forms of a V2V forward, checked before anything is launched.

The route is a pure function of a few integers and of ``se_conv3d_f32_variant`` (a host function: without a device the library
answers for 256 CUs, the MI355X's count), so every invariant the executor relies on is checked here on the host over a sweep of
batches, grids, input forms and number formats.  One GPU test then checks that ``V2VProgram.run`` issues exactly the launches its
route names.  Numerical checks of the composed program are ``tests/test_gpu_v2v_routes.py``'s.

The split-bf16 program keeps tensors octet-planar where its own kernel runs (D % 16 == 0), as it always has; "no planar tensor"
means for it: no quad-planar tensor, no pooled and no fused-skip form.  The bf16 program has no planar tensor at all.
"""
import itertools

import pytest
import torch

from sceneego_amd import _lib
from sceneego_amd.v2v import _DEC_UP, V2VModel, v2v_route

ALL_LEVELS = frozenset(range(5))
BATCHES = (1, 2, 3, 4, 8, 16, 32, 34)
GRIDS = (32, 64, 96, 128)
FORMS = ("planar1", "planar3", "cl")
DTYPES = {"f32": (torch.float32, False), "split3": (torch.float32, True), "bf16": (torch.bfloat16, False)}
COUT = 15
QUAD = _lib.IN_QUAD | _lib.OUT_QUAD | _lib.RES_QUAD
OCT = _lib.IN_OCTET | _lib.OUT_OCTET | _lib.RES_OCTET
BITS = {"quad": (_lib.IN_QUAD, _lib.OUT_QUAD, _lib.RES_QUAD), "oct": (_lib.IN_OCTET, _lib.OUT_OCTET, _lib.RES_OCTET)}
POOL_FED = ("front3", "enc1", "enc2", "enc3", "enc4")          # blocks whose output an encoder max-pool reads

_SWEEP = {}


def sweep():
    """(dtype name, B, G, form, fused soft-argmax, fork) -> route, computed once.  bf16 has the channels-last (octet) input only."""
    if not _SWEEP:
        for dt, B, G, form, sa, fork in itertools.product(DTYPES, BATCHES, GRIDS, FORMS, (False, True), (frozenset(), ALL_LEVELS)):
            if dt == "bf16" and form != "cl":
                continue
            dtype, split3 = DTYPES[dt]
            _SWEEP[(dt, B, G, form, sa, fork)] = v2v_route(COUT, dtype, split3, B, G, form, sa, fork)
    return _SWEEP


def lay_of(flags, which):
    """Layout the IN (0) / OUT (1) / RES (2) bits of a flag word name."""
    q, o = bool(flags & BITS["quad"][which]), bool(flags & BITS["oct"][which])
    assert not (q and o)
    return "quad" if q else "oct" if o else None


def expected_launches(route, G, cin, cout):
    """(function, dim, cin, cout, ksize, flags) of every launch of a plain float32 forward, in issue order: the structural walk of
    V2VProgram.run (front, five encoder levels, middle, five decoder levels, back, tail) over the route's entries."""
    L = []

    def res(name):
        r = route.blocks[name]
        L.append(("conv3d", r.dim, r.cin, r.cout, 3, r.flags1))
        if r.skip == "skip16":
            L.append(("conv3d_skip16", r.dim, r.cout, r.cout, 3, r.flags2))
            return r
        if r.skip == "conv":
            L.append(("conv3d", r.dim, r.cin, r.cout, 1, 0))
        L.append(("conv3d_pool" if r.pools else "conv3d", r.dim, r.cout, r.cout, 3, r.flags2))
        return r

    L.append(("conv3d_k7_fft" if route.front0.fft else "conv3d", G, cin, 16, 7, route.front0.flags))
    for i in (1, 2, 3):
        src = res(f"front{i}")
    for k in range(5):
        res(f"skip{k + 1}")
        if not src.pools:
            L.append(("maxpool3d_2", G >> k, src.cout, src.cout, 2, int(src.lay_out == "oct")))
        src = res(f"enc{k + 1}")
    res("mid")
    for k in range(5, 0, -1):
        res(f"decres{k}")
        L.append(("deconv3d_k2s2", G >> k, _DEC_UP[k - 1][0], _DEC_UP[k - 1][1], 2, route.up[k - 1]))
    res("back0")
    if route.tail.fused:
        L.append(("pointwise_chain3", G, 32, cout, 1, (_lib.IN_QUAD if route.tail.in_quad else 0) | (1 if route.tail.softargmax else 0)))
    else:
        L += [("conv3d", G, 32, 32, 1, _lib.EPI_RELU)] * 2 + [("conv3d", G, 32, cout, 1, _lib.EPI_OUT_PLANAR)]
    return L


def test_route_record():
    r = v2v_route(COUT, torch.float32, False, 8, 64, "planar1", True, ALL_LEVELS)
    assert r == v2v_route(COUT, torch.float32, False, 8, 64, "planar1", True, ALL_LEVELS) and r.fork == ALL_LEVELS
    assert set(r.blocks) == {f"front{i}" for i in (1, 2, 3)} | {f"{n}{k}" for n in ("skip", "enc", "decres") for k in range(1, 6)} | {"mid", "back0"}
    with pytest.raises(TypeError):
        r.blocks["mid"] = None
    with pytest.raises(ValueError):
        v2v_route(COUT, torch.float32, False, 1, 48)


def test_layouts_agree_between_producer_and_consumer():
    for key, r in sweep().items():
        b = r.blocks
        for name, e in b.items():
            # inside the block: the flag words say what the entry says, and the tensor between the two launches has one layout
            assert lay_of(e.flags1, 0) == e.lay_in and lay_of(e.flags2, 1) == e.lay_out, (key, name)
            assert lay_of(e.flags1, 1) == lay_of(e.flags2, 0), (key, name)
            assert lay_of(e.flags2, 2) == (e.lay_in if e.skip != "conv" else None), (key, name)
            assert e.skip in ("identity", "conv", "skip16") and (e.skip == "identity") == (e.cin == e.cout), (key, name)
        assert ("quad" if r.front0.flags & _lib.OUT_QUAD else None) == r.front0.lay_out == b["front1"].lay_in, key
        assert b["front1"].lay_out == b["front2"].lay_in and b["front2"].lay_out == b["front3"].lay_in, key
        for k in range(5):
            src = b["front3"] if k == 0 else b[f"enc{k}"]
            assert b[f"skip{k + 1}"].lay_in == src.lay_out, (key, k)
            assert b[f"enc{k + 1}"].lay_in is None, (key, k)                 # a pooled tensor is channels-last
            # skip block -> residual of the transposed convolution -> the block behind it
            assert b[f"skip{k + 1}"].lay_out == ("quad" if r.up[k] & _lib.RES_QUAD else None), (key, k)
            nxt = b[f"decres{k}"] if k else b["back0"]
            assert nxt.lay_in == ("quad" if r.up[k] & _lib.OUT_QUAD else None), (key, k)
            assert not r.up[k] & (OCT | _lib.IN_QUAD), (key, k)
        assert b["decres5"].lay_in is None, key
        assert b["back0"].lay_out == ("quad" if r.tail.in_quad else None), key


def test_planar_outputs_in_front_of_a_pool_are_pooled():
    for key, r in sweep().items():
        pools = [l for l in expected_launches(r, key[2], 33, COUT) if l[0] == "maxpool3d_2"]
        for name in POOL_FED:
            e = r.blocks[name]
            if e.lay_out == "quad":
                assert e.pools, (key, name)
            if e.lay_out == "oct" and not e.pools:
                assert (e.dim, e.cout, 1) in [(p[1], p[2], p[5]) for p in pools], (key, name)
        assert not any(e.pools for n, e in r.blocks.items() if n not in POOL_FED), key
        assert len(pools) + sum(r.blocks[n].pools for n in POOL_FED) == 5, key


def test_no_planar_tensor_where_none_is_allowed():
    for key, r in sweep().items():
        b = r.blocks
        assert b["mid"].lay_in is None and b["mid"].lay_out is None, key
        assert all(b[f"decres{k}"].lay_out is None for k in range(1, 6)), key       # what a transposed convolution reads
        assert all(e.lay_in is None for e in b.values() if e.skip == "conv"), key
        assert r.tail.fused or b["back0"].lay_out is None, key
        assert r.tail.softargmax or not r.tail.in_quad, key
        unfused = v2v_route(17, *DTYPES[key[0]], *key[1:])        # more than 16 output channels: three launches, channels-last input
        assert unfused.tail == (False, False, False) and unfused.blocks["back0"].lay_out is None, key
        words = [f for e in b.values() for f in (e.flags1, e.flags2)] + list(r.up) + [r.front0.flags]
        if key[0] == "bf16":
            assert not any(f & (QUAD | OCT) for f in words) and not any(e.lay_in or e.lay_out for e in b.values()), key
        if key[0] != "f32":
            assert not any(f & QUAD for f in words) and not r.tail.in_quad, key
            assert not any(e.pools or e.skip == "skip16" for e in b.values()), key
            assert all(e.dim % 16 == 0 for e in b.values() if (e.flags1 | e.flags2) & OCT), key
            assert all(e.variants == (None, None) for e in b.values() if key[0] == "bf16" or e.dim % 16 == 0), key


def test_library_accepts_every_flag_word():
    """The conditions under which conv3d_f32_impl / se_conv3d_skip16_f32 / se_deconv3d_k2s2_f32 return SE_ERR_BAD_ARG."""
    for key, r in sweep().items():
        if key[0] != "f32":
            continue
        B = key[1]
        for name, e in r.blocks.items():
            for ci, flags, var, fused in ((e.cin, e.flags1, e.variants[0], False), (e.cout, e.flags2, e.variants[1], e.skip == "skip16")):
                where = (key, name, flags)
                assert var == _lib.conv3d_variant(B, e.dim, ci, e.cout, 3, flags), where
                assert not (flags & QUAD and flags & OCT), where
                assert not (flags & _lib.EPI_RES_PRE_RELU and flags & _lib.EPI_RES_POST_RELU) and not flags & _lib.EPI_OUT_PLANAR, where
                if flags & (QUAD | OCT):
                    assert _lib.conv3d_algo(e.dim, ci, e.cout, 3) == 2, where
                if flags & (_lib.IN_QUAD | _lib.RES_QUAD):
                    assert var == 3, where
                if flags & OCT:
                    assert var in (2, 3), where
                if fused:
                    assert ci % 16 == 0 and _lib.conv3d_algo(e.dim, ci, e.cout, 3) == 2 and e.cin == 16, where
                    assert flags & (QUAD | OCT) in (_lib.IN_OCTET | _lib.OUT_OCTET, _lib.IN_QUAD | _lib.OUT_QUAD, QUAD), where
            # pooled forms: only the 2-D Winograd kernels pool, and only even levels
            if e.pools:
                assert _lib.conv3d_algo(e.dim, e.cout, e.cout, 3) == 2 and e.dim % 2 == 0, (key, name)
        for k, flags in enumerate(r.up):
            assert flags & ~(QUAD | OCT) == _lib.EPI_RELU | _lib.EPI_RES_POST_RELU, (key, k)
            if flags & _lib.OUT_QUAD:
                assert (key[2] >> (k + 1)) % 16 == 0 and _DEC_UP[k] in ((64, 32), (128, 64)), (key, k)
            assert not flags & _lib.RES_QUAD or flags & _lib.OUT_QUAD, (key, k)
        assert r.front0.fft == (key[3] == "planar1") and bool(r.front0.flags & _lib.IN_PLANAR3) == (key[3] == "planar3"), key


def test_gpu_route_matrix_still_covers_every_kernel_and_layout():
    """Host twin of test_gpu_v2v_routes.test_route_matrix_coverage."""
    from test_gpu_v2v_routes import ROUTES
    points = [(p.values[0], p.values[1]) for p in ROUTES] + [(128, 1)]
    variants, layouts = set(), set()
    for G, B in points:
        r = v2v_route(COUT, torch.float32, False, B, G, "planar1", True)
        layouts.add(r.front0.lay_out or "cl")
        for e in r.blocks.values():
            variants.update(e.variants)
            layouts.add(e.lay_out or "cl")
    assert {0, 1, 2, 3} <= variants, variants
    assert {"quad", "oct", "cl"} <= layouts, layouts


# The production routes (G = 64, float32, planar input, fused soft-argmax) as the program ran them before the route function
# existed: per block (input layout, output layout, pools, skip mode, variant pair), recorded from that program's launches.
_CL5 = (None, None, False, "identity", (0, 0))
PINNED = {
    1: {
        "front1": ("quad", "quad", False, "skip16", (3, 3)), "front2": ("quad", "quad", False, "identity", (3, 3)),
        "front3": ("quad", "quad", True, "identity", (3, 3)), "skip1": ("quad", "quad", False, "identity", (3, 3)),
        "enc1": (None, "oct", True, "conv", (2, 2)), "skip2": ("oct", None, False, "identity", (2, 2)),
        "enc2": (None, None, False, "conv", (0, 0)), "skip3": _CL5, "enc3": _CL5, "skip4": _CL5, "enc4": _CL5, "skip5": _CL5,
        "enc5": _CL5, "mid": _CL5, "decres5": _CL5, "decres4": _CL5, "decres3": _CL5, "decres2": _CL5,
        "decres1": (None, None, False, "identity", (2, 2)), "back0": ("quad", "quad", False, "identity", (3, 3)),
    },
    8: {
        "front1": ("quad", "quad", False, "skip16", (3, 3)), "front2": ("quad", "quad", False, "identity", (3, 3)),
        "front3": ("quad", "quad", True, "identity", (3, 3)), "skip1": ("quad", "quad", False, "identity", (3, 3)),
        "enc1": (None, "quad", True, "conv", (2, 3)), "skip2": ("quad", "quad", False, "identity", (3, 3)),
        "enc2": (None, "oct", True, "conv", (2, 2)), "skip3": ("oct", None, False, "identity", (2, 2)),
        "enc3": _CL5, "skip4": _CL5, "enc4": _CL5, "skip5": _CL5, "enc5": _CL5, "mid": _CL5, "decres5": _CL5, "decres4": _CL5,
        "decres3": _CL5, "decres2": (None, None, False, "identity", (2, 2)), "decres1": ("quad", None, False, "identity", (3, 3)),
        "back0": ("quad", "quad", False, "identity", (3, 3)),
    },
}
PINNED_UP_QUAD = {1: (True, False, False, False, False), 8: (True, True, False, False, False)}


@pytest.mark.parametrize("B", (1, 8))
def test_production_routes_are_pinned(B):
    r = v2v_route(COUT, torch.float32, False, B, 64, "planar1", True)
    got = {n: (e.lay_in, e.lay_out, e.pools, e.skip, e.variants) for n, e in r.blocks.items()}
    assert got == PINNED[B]
    assert r.front0 == (True, _lib.EPI_RELU | _lib.OUT_QUAD, "quad") and r.tail == (True, True, True) and not r.fork
    quad = _lib.OUT_QUAD | _lib.RES_QUAD
    assert r.up == tuple(_lib.EPI_RELU | _lib.EPI_RES_POST_RELU | (quad if q else 0) for q in PINNED_UP_QUAD[B])


# ------------------------------------------------------------------------------------------------
# GPU: the executor launches what the route says
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", (1, 8))
def test_executed_launches_match_route(B, monkeypatch):
    """G = 32 (the smallest grid run() accepts) at B = 1 and B = 8 (top level octet / quad): a recorder around the _lib launch
    functions sees exactly the route's entries - function, level, channels, flag word - in the order of the structural walk."""
    G, dev = 32, "cuda:0"
    torch.manual_seed(5)
    prog = V2VModel(33, COUT).to(dev).eval().compile()
    seen = []

    def wrap(name, describe):
        orig = getattr(_lib, name)

        def f(*a, **k):
            seen.append(describe(*a, **k))
            return orig(*a, **k)
        monkeypatch.setattr(_lib, name, f)

    wrap("conv3d", lambda i, w, b, r, o, batch, dim, cin, cin_pad, cout, ks, flags, workspace=None, pool_out=None:
         ("conv3d" if pool_out is None else "conv3d_pool", dim, cin, cout, ks, flags))
    wrap("conv3d_skip16", lambda i, w, b, si, sw, o, batch, dim, cin, cout, flags: ("conv3d_skip16", dim, cin, cout, 3, flags))
    wrap("conv3d_k7_fft", lambda i, h, b, o, batch, dim, cin, cout, flags, ws: ("conv3d_k7_fft", dim, cin, cout, 7, flags))
    wrap("deconv3d_k2s2", lambda i, w, b, r, o, batch, dim, cin, cout, flags: ("deconv3d_k2s2", dim, cin, cout, 2, flags))
    wrap("maxpool3d_2", lambda i, o, batch, dim, c, in_octet=False: ("maxpool3d_2", dim, c, c, 2, int(in_octet)))
    wrap("pointwise_chain3", lambda i, p1, p2, p3, o, batch, dim, softargmax=None, in_quad=False:
         ("pointwise_chain3", dim, 32, p3.cout, 1, (_lib.IN_QUAD if in_quad else 0) | (1 if softargmax is not None else 0)))
    wrap("conv3d_k3_split3", lambda *a, **k: ("conv3d_k3_split3",))
    x = torch.randn(B, 33, G, G, G, device=dev)
    coord = torch.zeros(G ** 3, 3, device=dev)
    scratch = torch.empty(_lib.softargmax3d_scratch_elems(B * COUT), device=dev)
    prog.run(x, B, G, softargmax=(coord, scratch), planar1=True)
    torch.cuda.synchronize()
    (key, route), = prog._routes.items()
    assert key == (B, G, "planar1", True, frozenset())
    assert route.blocks["front3"].lay_out == ("quad" if B == 8 else "oct")
    assert seen == expected_launches(route, G, 33, COUT)
