"""float64 interval model of ONE launch of the bf16-storage V2V program.  Plain torch on the CPU.

Operands of a launch: bf16 activations ``x``, bf16 weights ``w`` (the BatchNorm-folded float32 weights rounded once), a float32
bias ``b`` and an optional bf16 residual ``r``.  All of them are exact in float64, so

    y = sum x * w + b                     (float64: error 2^-53 relative per term, seven orders below the bound)
    S = sum |x * w| + |b|                 (the same convolution on absolute values)

are the exact value and the magnitude the rounding errors of any summation order scale with.  A kernel accumulates in float32 in
an order of its own, applies the epilogue ONCE - (+r), ReLU, (+r), round to nearest even - and stores bf16.  The epilogue is
monotone in the accumulator, so with delta = g * 2^-24 * S every output element must satisfy

    lo <= got <= hi,    lo = bf16_rne(epi(y - delta)),    hi = bf16_rne(epi(y + delta))

compared as bf16 values (NaN never satisfies it).  Where lo == hi the kernel is held to the exact bit pattern; elsewhere the exact
value lies within delta of a rounding boundary and both neighbours are correct.  The factor ``g`` (G_FACTOR, capped by the worst
case K + 2 of a K-term sum with a bias and an epilogue add) is 4 x the largest ratio max|y32 - y| / (2^-24 S) that torch-CPU float32
shows on the identical operands over the case matrix (3.75 to 3.91, depending on the host), rounded up to a power of two;
tests/test_bf16_launch_model_host.py re-measures it, and holds every case to at most STRADDLE_CAP elements with lo != hi so that
the interval cannot pass trivially.

The fused tail has two hidden bf16 roundings: the intervals go through the next layer by interval arithmetic
(W+ lo + W- hi + b - delta and its mirror) and the float32 logits are compared with [lo3, hi3] directly.
"""
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

BF = torch.bfloat16
EPI_RELU, EPI_RES_PRE_RELU, EPI_RES_POST_RELU = 1, 2, 4       # sceneego_amd._lib.EPI_*
U24 = 2.0 ** -24                # unit roundoff of float32
G_FACTOR = 16.0                 # see the module docstring; measured g_ref: profiles/bf16_launch_parity.txt
STRADDLE_CAP = 0.10             # at most this share of a case's elements may have lo != hi
_IM2COL_BYTES = 1 << 28         # torch's CPU conv3d materialises the im2col matrix of a sample: walk z slabs above this


def g_of(K):
    """The factor of a K-term dot product: G_FACTOR, never above the worst case of K products, a bias and an epilogue add."""
    return min(G_FACTOR, K + 2.0)


# ------------------------------------------------------------------------------------------------
# bf16 rounding of float64 values (no double rounding through float32)
# ------------------------------------------------------------------------------------------------
def bf16_rne(v):
    """float64 -> the nearest bf16 VALUE (ties to even), as float64.  Gradual underflow below 2^-126 as in the format."""
    v = v.double()
    _, e = torch.frexp(v)                                  # |v| = m * 2^e, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(v), e.clamp(min=-125) - 8)
    out = torch.round(v / ulp) * ulp                       # torch.round: half to even
    assert bool((out.abs() < 3.0e38).all()), "bf16 overflow in the reference"
    return out


def bf16_truncate(v32):
    """float32 -> bf16 by dropping the low 16 bits (the WRONG rounding: what the comparison must reject)."""
    return (v32.float().contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)


def bf16_ulp(v):
    """The spacing of bf16 at |v| (float64)."""
    _, e = torch.frexp(v.double())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e.clamp(min=-125) - 8)


def epilogue(v, res, flags):
    """(+r), ReLU, (+r) on a tensor of any float type: monotone in ``v``."""
    if res is not None and flags & EPI_RES_PRE_RELU:
        v = v + res
    if flags & EPI_RELU:
        v = v.clamp(min=0)
    if res is not None and flags & EPI_RES_POST_RELU:
        v = v + res
    return v


# ------------------------------------------------------------------------------------------------
# exact value and magnitude of a convolution
# ------------------------------------------------------------------------------------------------
def conv3d(x, w, b, k):
    """F.conv3d with zero padding k // 2, in output z slabs when the im2col matrix of a sample would be large (7^3 x 40 channels
    at 48^3 in float64: 12 GB).  The same operator on every slab: no output element changes its summation."""
    p = k // 2
    D = x.shape[2]
    per_plane = x.shape[1] * k ** 3 * x.shape[3] * x.shape[4] * x.element_size()
    if per_plane * D <= _IM2COL_BYTES:
        return F.conv3d(x, w, b, padding=p)
    xp = F.pad(x, (0, 0, 0, 0, p, p))
    S = max(1, _IM2COL_BYTES // per_plane)
    return torch.cat([F.conv3d(xp[:, :, z:z + S + 2 * p], w, b, padding=(0, p, p)) for z in range(0, D, S)], dim=2)


def _apply(x, w, b, k, transposed):
    return F.conv_transpose3d(x, w, b, stride=2) if transposed else conv3d(x, w, b, k)


def crop(t, box, halo):
    """t [n,C,D,D,D]; box ((z0,z1),(y0,y1),(x0,x1)) or None.  The box grown by ``halo`` and clipped to the volume - the volume's own
    border keeps its zero padding - and the box's offsets inside the crop."""
    if box is None:
        return t, None
    D = t.shape[2]
    lo = [max(0, a - halo) for a, _ in box]
    hi = [min(D, b + halo) for _, b in box]
    return t[:, :, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], tuple((a - l, b - l) for (a, b), l in zip(box, lo))


def inner(t, off):
    if off is None:
        return t
    (z0, z1), (y0, y1), (x0, x1) = off
    return t[:, :, z0:z1, y0:y1, x0:x1]


def exact(x, w, b, k, transposed=False, box=None):
    """(y, S) in float64 of a convolution (k = 1, 3, 7, zero padding) or the k2s2 transposed convolution, on the OUTPUT box ``box``
    (None: everything).  x [B,cin,D,D,D], w in torch's layout, b [cout]; any float dtype holding the operands exactly."""
    x, w, b = x.double(), w.double(), b.double()
    if transposed:
        off = None
        if box is not None:
            assert all(a % 2 == 0 and e % 2 == 0 for a, e in box)
            x, off = crop(x, tuple((a // 2, e // 2) for a, e in box), 0)
            off = tuple((2 * a, 2 * e) for a, e in off)
    else:
        x, off = crop(x, box, k // 2)
    y = inner(_apply(x, w, b, k, transposed), off)
    S = inner(_apply(x.abs(), w.abs(), b.abs(), k, transposed), off)
    return y, S


def float32_reference(x, w, b, k, transposed=False, box=None):
    """torch-CPU float32 accumulator (convolution + bias, before the epilogue) on the identical operands."""
    x, w, b = x.float(), w.float(), b.float()
    if transposed:
        assert box is None
        return _apply(x, w, b, k, True)
    x, off = crop(x, box, k // 2)
    return inner(_apply(x, w, b, k, False), off)


# ------------------------------------------------------------------------------------------------
# the interval and the comparison
# ------------------------------------------------------------------------------------------------
class Interval(NamedTuple):
    lo: torch.Tensor            # float64 tensors holding bf16 values (the chain's logits: plain float64 bounds)
    hi: torch.Tensor


def interval(y, S, res, flags, g):
    """[lo, hi] of a launch's bf16 output."""
    d = g * U24 * S
    r = None if res is None else res.double()
    return Interval(bf16_rne(epilogue(y - d, r, flags)), bf16_rne(epilogue(y + d, r, flags)))


def outside(got, iv):
    """Mask of the elements that violate lo <= got <= hi.  NaN violates it.  No element is left out."""
    got = got.double()
    assert got.shape == iv.lo.shape, (got.shape, iv.lo.shape)
    return ~((got >= iv.lo) & (got <= iv.hi))


def straddle_share(iv):
    return float((iv.lo != iv.hi).double().mean())


def on_edge(got, iv):
    """How many elements sit on lo or on hi where the two differ (both are correct there)."""
    got = got.double()
    s = iv.lo != iv.hi
    return int((s & (got == iv.lo)).sum()), int((s & (got == iv.hi)).sum())


def g_ref(acc32, y, S):
    """max |y32 - y| / (2^-24 S): the float32 reference's own distance from the exact value, in units of the bound."""
    return float(((acc32.double() - y).abs() / (U24 * S)).max())


# ------------------------------------------------------------------------------------------------
# the fused tail: 1x1x1 (+ReLU) -> 1x1x1 (+ReLU) -> 1x1x1, float32 logits
# ------------------------------------------------------------------------------------------------
class ChainModel(NamedTuple):
    h1: Interval                # bf16 hidden activations after layer 1 / 2: [N, 32]
    h2: Interval
    logits: Interval            # float64 bounds of the float32 logits [N, cout3]
    y3: torch.Tensor            # exact logits of the voxels whose hidden values are determined (lo == hi on all 64 of them)
    S3: torch.Tensor
    determined: torch.Tensor    # [N] bool


def _through(lo, hi, w, b, g):
    wp, wn = w.clamp(min=0), w.clamp(max=0)
    ylo = lo @ wp.T + hi @ wn.T + b
    yhi = hi @ wp.T + lo @ wn.T + b
    S = torch.maximum(lo.abs(), hi.abs()) @ w.abs().T + b.abs()
    d = g * U24 * S
    return ylo - d, yhi + d, S


def chain(x, w1, b1, w2, b2, w3, b3):
    """x [N,32] bf16 values; w* [cout,cin] bf16 values, b* float32 values -> ChainModel (everything float64)."""
    x, w1, b1, w2, b2, w3, b3 = (t.double() for t in (x, w1, b1, w2, b2, w3, b3))
    g = g_of(x.shape[1])
    lo, hi, _ = _through(x, x, w1, b1, g)
    h1 = Interval(bf16_rne(lo.clamp(min=0)), bf16_rne(hi.clamp(min=0)))
    lo, hi, _ = _through(h1.lo, h1.hi, w2, b2, g_of(w2.shape[1]))
    h2 = Interval(bf16_rne(lo.clamp(min=0)), bf16_rne(hi.clamp(min=0)))
    lo, hi, S3 = _through(h2.lo, h2.hi, w3, b3, g_of(w3.shape[1]))
    det = (h1.lo == h1.hi).all(dim=1) & (h2.lo == h2.hi).all(dim=1)
    y3 = h2.lo @ w3.T + b3
    return ChainModel(h1, h2, Interval(lo, hi), y3, S3, det)


def chain_float32(x, w1, b1, w2, b2, w3, b3):
    """The chain in torch-CPU float32 with round-to-nearest-even hidden tensors: a correct implementation the model must accept."""
    r = lambda t: t.to(BF).float()
    h = r(F.relu(x.float() @ w1.float().T + b1.float()))
    h = r(F.relu(h @ w2.float().T + b2.float()))
    return h @ w3.float().T + b3.float()


def device_ratio(got, cm):
    """The device's own |logit - y3| / (2^-24 S3) over the voxels whose hidden values the model determines; (ratio, voxel count)."""
    if not bool(cm.determined.any()):
        return float("nan"), 0
    d = cm.determined
    return float(((got.double()[d] - cm.y3[d]).abs() / (U24 * cm.S3[d])).max()), int(d.sum())


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))
