"""Exact checks of the kernels around the tile kernels: the fused L2
normalize pair, the per-tensor and row-wise e4m3 quantizers, the in-place
bf16 scale and the split-K weight gradient.

Every reference is float64 (or, where the kernel does one correctly rounded
fp32 operation, that same operation done by torch on the CPU), computed from
exactly what the kernel reads.  Generators are seeded; inputs and references
are built once per case and never modified.

Notation: ``ulp_bf16(v) = 2^(floor(log2|v|) - 7)`` (the smallest normal
binade for zero and subnormals).  The e4m3 code table is
``arange(256, uint8).view(float8_e4m3fn)`` decoded to float64 without its two
NaN codes; the *nearest code* of a value is found by search in that table,
ties to the even code, magnitudes above 448 to +-448, the sign bit that of the
value (so a negative value that rounds to zero is 0x80, as IEEE rounding and
the hardware conversion give).  Torch's own ``.to(float8_e4m3fn)`` is not the
reference: it casts 465.0 to NaN where the kernel's conversion saturates.

Bounds (derived, none measured on the GPU):

1. ``l2_normalize`` forward.  ``|y - y64| <= 1 ulp_bf16(y64)``: half an ulp
   is the rounding; the fp32 sum of d squares (d/64 sequential adds per lane,
   6 shuffle adds), sqrt, reciprocal and product are at most
   ``(d + 8) 2^-24`` relative, under 2^-13 for d <= 1026, inside the other
   half.  The all-zero row gives exactly 0; no NaN or Inf anywhere; the
   output norm of each row with ``||x|| >= eps`` is within ``sqrt(d) 2^-9``
   of 1 (d roundings of at most 2^-9 relative each move the norm of a unit
   vector by at most ``sqrt(d) 2^-9``).  ``rn`` equals
   ``1 / max(||x||, eps)`` to ``(d + 8) 2^-24`` relative, ``1/eps`` on the
   zero row.  Each shape carries an all-zero row, a row scaled by 2^-60 and
   a row scaled by 2^40 (b = 1: one run per kind).  The 2^-60 row has
   ``||x|| ~ 1e-16 < eps = 1e-12``: it is the eps clamp on non-zero data,
   ``y = x / eps`` as ``F.normalize`` defines it, so it is held to the
   element bound but not to the unit norm, and it is left out of the two
   backward preconditions (its projection term is ~1e-10 of ``dy``).
2. ``l2_normalize`` backward, ``dx = rn (dy - y <y, dy>)``.  Inputs are
   *informative*: ``dy = c_i sqrt(d) y + randn`` with ``c_i ~ 2 randn`` per
   row, so that the projection term matters -- asserted as a precondition on
   the reference: at least 50 % of the elements (of rows with
   ``||x|| >= eps``) have ``|y_k <y, dy>| >= 0.25 |dy_k|``.  (With
   ``dy ~ randn`` at d = 768 the term is 3 % of ``dy`` and a kernel that
   drops it passes a bf16-class tolerance.)
   - kernel arithmetic: ``ref = rn64 (dy - yb <yb, dy>)`` with ``yb`` the
     bf16 output the forward saved; per element
     ``|dx - ref| <= ulp_bf16(ref)
                      + rn64 (d + 8) 2^-24 (|dy_k| + |yb_k| sum_j |yb_j dy_j|)``
     -- the rounding, plus the fp32 dot and products relative to the
     magnitudes that cancel rather than to their difference.
   - the true gradient: the float64 gradient of ``x / ||x||`` at the bf16
     ``x``; the bound above plus
     ``rn64 2^-8 |y_k| (sum_j |y_j dy_j| + |<y, dy>|)`` for the kernel
     reading ``y`` rounded to bf16 (2^-9 relative per element, doubled).
   - the tests bite: an emulated kernel without the projection term
     (``bf16(fp32(rn64) dy)``) must break the first bound on more than 90 %
     of the elements; the share is computed and asserted per case.
   - zero row: ``dx = dy / eps`` to 1 bf16 ulp, finite.
3. Per-tensor quantizer.  ``amax`` = exact max |x|;
   ``r = fp32(448) / fp32(amax)`` and ``p = fp32(x) r`` are single correctly
   rounded fp32 operations in the kernel (no fast-math; one multiply cannot
   contract) and are done the same way by torch on the CPU.  The bytes equal
   the nearest code of ``p``.  Excused: an element whose ``p`` lies within 2
   fp32 ulps of the midpoint of two adjacent codes, but not on it, may take
   either neighbour; the share of such elements is asserted under 0.1 % on
   the reference first.  ``scale == amax / 448`` to 1 fp32 ulp.  Every amax
   element has code 0x7E / 0xFE and no byte is 0x7F / 0xFF (``p`` can reach
   ``448 (1 + 2^-23)`` there; the conversion saturates).
4. Row-wise quantizer.  ``k`` = the smallest integer with
   ``max(amax, 1e-30f) <= 448 2^k`` (found by comparison), clamped to
   [-126, 127]; ``e8 = 127 + k``; the codes equal the nearest code of
   ``x 2^-k``.  That product is exact, so there are no excused elements.
   ``ratio = 2^(e8 - emax)`` and ``s_ref = 2^(emax - 127)`` bit-equal in
   fp32; ``q 2^(e8 - 127)`` within half the local e4m3 step of ``x``.
   Every shape holds (asserted on the reference; shapes with too few rows
   spread them over several tensors) rows with ``amax`` exactly
   ``448 2^k``, the bf16 below and the bf16 above (which gives ``k + 1``)
   for five ``k``, an all-zero row, a row at bf16's largest finite value and
   one at 2^-120 (under the 1e-30 floor).
5. ``scale_bf16_``: bitwise ``x * s.to(bfloat16)`` of torch.
6. wgrad with integer operands in {-3..3} and K <= 4128: every partial and
   sum is an integer below 4128 * 9 < 2^24, exact in fp32 in any order, so
   the result is ``(a.double().T @ x.double()).to(bfloat16)`` bit for bit
   and independent of the slice count.  Outputs with ``|v| > 256`` and odd
   are not representable in bf16; their presence (asserted where K makes
   them reachable: 4 sqrt(K) >= 126) exercises the final rounding.

Grid trips covered: the per-tensor quantizer's 2048 x 256 x 8 = 4 194 304
elements, the row-wise quantizer's 1024 x 8 = 8192 rows and the scale
kernel's 4096 x 256 x 8 = 8 388 608 elements are each crossed, with the
tensor maximum placed past the first trip and, in a second run, inside it.
``(4096, 1025)`` has ``n % 8 == 0``: its remainder past the full trip is 512
vector accesses, not the scalar loop, so ``(4099, 1025)`` (``n % 8 == 3``)
is added with the maximum in the scalar tail.
"""

import ctypes
import functools
import math
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops

DEV = "cuda"
BF16 = torch.bfloat16
E4M3 = torch.float8_e4m3fn
EPS32 = float(torch.tensor(1e-12, dtype=torch.float32))   # as the entry gets it
NANBITS = int(torch.tensor(float("nan"), dtype=BF16).view(torch.int16))
RN_SENTINEL = -12345.0
GUARD = 64                            # guard elements on either side

TABLE = torch.arange(256, dtype=torch.uint8).view(E4M3).float().double()
POS = TABLE[:0x7F]                    # codes 0x00..0x7E: 0 .. 448 ascending
MIDS = (POS[1:] + POS[:-1]) / 2       # 126 midpoints of adjacent codes
assert float(POS[-1]) == 448.0 and bool((POS[1:] > POS[:-1]).all())


def _floor_log2(v, emin):
    """floor(log2|v|) of a float64 tensor, ``emin`` for zero and below."""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)


def ulp_bf16(v):
    return torch.exp2((_floor_log2(v, -126) - 7).double())


def ulp_fp32(v):
    return torch.exp2((_floor_log2(v, -126) - 23).double())


def nearest_code(p):
    """(codes, distance of |p| to the nearest midpoint, is-on-a-midpoint)."""
    p = p.double()
    a = p.abs().clamp(max=448.0)
    idx = torch.searchsorted(MIDS, a)           # midpoints strictly below a
    lo = MIDS[(idx - 1).clamp(min=0)]
    hi = MIDS[idx.clamp(max=125)]
    tie = hi == a
    dist = torch.minimum((a - lo).abs(), (hi - a).abs())
    idx = idx + (tie & (idx % 2 == 1))
    code = (idx + 128 * torch.signbit(p)).to(torch.uint8)
    return code, dist, tie


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _guarded(numel, dtype, fill):
    """(whole buffer, inner view of ``numel`` elements) with GUARD elements of
    ``fill`` on either side and inside."""
    if dtype == BF16:
        buf = torch.full((numel + 2 * GUARD,), fill, dtype=torch.int16,
                         device=DEV).view(BF16)
    else:
        buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def _assert_guards(buf, fill, what):
    raw = buf.view(torch.int16) if buf.dtype == BF16 else buf
    inner = raw[GUARD:-GUARD]
    assert bool((raw[:GUARD] == fill).all()), f"{what}: front guard changed"
    assert bool((raw[-GUARD:] == fill).all()), f"{what}: back guard changed"
    assert not bool((inner == fill).any()), f"{what}: sentinel left inside"


# ---------------------------------------------------------------------------
# 1, 2. l2_normalize
# ---------------------------------------------------------------------------

L2_SHAPES = [(1, 2), (7, 66), (9, 130), (1000, 768), (17, 1026)]
PLAIN, ZERO, TINY, HUGE = "plain", "zero", "2^-60", "2^40"


def _l2_variants(b):
    """Row kinds per run: all three special rows at once where b allows it,
    otherwise (b = 1) one run per kind."""
    if b >= 4:
        kinds = [PLAIN] * b
        kinds[1], kinds[b // 2], kinds[b - 1] = ZERO, TINY, HUGE
        return [tuple(kinds)]
    return [(k,) * b for k in (PLAIN, ZERO, TINY, HUGE)]


L2_CASES = [(b, d, v) for b, d in L2_SHAPES
            for v in range(len(_l2_variants(b)))]


class _L2(NamedTuple):
    x: torch.Tensor          # bf16 (b, d)
    dy: torch.Tensor         # bf16 (b, d)
    nz: torch.Tensor         # bool (b,): non-zero rows
    unit: torch.Tensor       # bool (b,): rows with ||x|| >= eps
    rn64: torch.Tensor       # (b, 1)
    y64: torch.Tensor
    informative: float


@functools.lru_cache(maxsize=None)
def _l2_case(b, d, v):
    kinds = _l2_variants(b)[v]
    gen = torch.Generator().manual_seed(1000 * d + 10 * b + v)
    x = 3 * torch.randn(b, d, generator=gen)
    mul = torch.tensor([{PLAIN: 1.0, ZERO: 0.0, TINY: 2.0 ** -60,
                         HUGE: 2.0 ** 40}[k] for k in kinds])
    x = (x.to(BF16).float() * mul[:, None]).to(BF16)   # pow2: exact
    xd = x.double()
    nz = mul != 0
    assert bool((xd[nz].abs().amax(dim=1) > 0).all())
    unit = xd.norm(dim=1) >= EPS32
    assert [bool(u) for u in unit] == [k in (PLAIN, HUGE) for k in kinds]
    rn64 = 1.0 / xd.norm(dim=1, keepdim=True).clamp(min=EPS32)
    y64 = xd * rn64
    c = 2 * torch.randn(b, 1, generator=gen)
    dy = (c.double() * math.sqrt(d) * y64.to(BF16).double()
          + torch.randn(b, d, generator=gen).double()).to(BF16)
    dyd = dy.double()
    proj = (y64 * (y64 * dyd).sum(1, keepdim=True)).abs()
    big = proj[unit] >= 0.25 * dyd[unit].abs()
    informative = float(big.double().mean()) if bool(unit.any()) else 1.0
    return _L2(x, dy, nz, unit, rn64, y64, informative)


def _bwd_bound(ref, dyd, yb, rn64, d):
    return (ulp_bf16(ref) + rn64 * (d + 8) * 2.0 ** -24
            * (dyd.abs() + yb.abs() * (yb * dyd).abs().sum(1, keepdim=True)))


@pytest.mark.parametrize("b,d,v", L2_CASES)
def test_l2_forward(b, d, v):
    c = _l2_case(b, d, v)
    y = ops.l2_normalize(c.x.to(DEV))
    assert y.dtype == BF16 and y.shape == (b, d)
    yd = y.cpu().double()
    assert bool(torch.isfinite(yd).all())
    err = (yd - c.y64).abs() / ulp_bf16(c.y64)
    print(f"l2 fwd ({b},{d},{v}): max err {float(err.max()):.3f} ulp")
    assert float(err.max()) <= 1.0
    assert bool((yd[~c.nz] == 0).all())
    if bool(c.unit.any()):
        dev = (yd[c.unit].norm(dim=1) - 1).abs().max()
        assert float(dev) <= math.sqrt(d) * 2.0 ** -9


@pytest.mark.parametrize("b,d,v", L2_CASES)
def test_l2_backward_informative(b, d, v):
    c = _l2_case(b, d, v)
    nz, unit = c.nz, c.unit
    assert c.informative >= 0.5, c.informative
    x = c.x.to(DEV).requires_grad_()
    y = ops.l2_normalize(x)
    y.backward(c.dy.to(DEV))
    dx = x.grad.cpu().double()
    yb = y.detach().cpu().double()
    dyd = c.dy.double()
    assert bool(torch.isfinite(dx).all())

    ref = c.rn64 * (dyd - yb * (yb * dyd).sum(1, keepdim=True))
    bound = _bwd_bound(ref, dyd, yb, c.rn64, d)
    # The check is only meaningful if dropping the projection breaks it.
    noproj = (c.rn64.float() * c.dy.float()).to(BF16).double()
    if bool(unit.any()):
        share = float(((noproj - ref).abs() > bound)[unit].double().mean())
        print(f"l2 bwd ({b},{d},{v}): informative {c.informative:.3f}, "
              f"no-projection kernel fails on {share:.3f}")
        assert share > 0.9, share
    r1 = float(((dx - ref).abs() / bound).max())

    y64 = c.y64
    true = c.rn64 * (dyd - y64 * (y64 * dyd).sum(1, keepdim=True))
    bound2 = (_bwd_bound(true, dyd, yb, c.rn64, d)
              + c.rn64 * 2.0 ** -8 * y64.abs()
              * ((y64 * dyd).abs().sum(1, keepdim=True)
                 + (y64 * dyd).sum(1, keepdim=True).abs()))
    r2 = float(((dx - true).abs() / bound2).max())
    print(f"l2 bwd ({b},{d},{v}): kernel arithmetic at {r1:.3f} of its bound, "
          f"true gradient at {r2:.3f}")
    assert r1 <= 1.0 and r2 <= 1.0

    if bool((~nz).any()):
        z = dyd[~nz] / EPS32
        assert bool(((dx[~nz] - z).abs() <= ulp_bf16(z)).all())


@pytest.mark.parametrize("b,d", [(9, 130), (7, 66)])
def test_l2_entries_stay_inside_their_buffers(b, d):
    c = _l2_case(b, d, 0)
    lib = ops._require_lib()
    x = c.x.to(DEV)
    ybuf, y = _guarded(b * d, BF16, NANBITS)
    rbuf, rn = _guarded(b, torch.float32, RN_SENTINEL)
    ops._check(lib.l2norm_fwd_bf16(_stream(), _p(x), _p(y), _p(rn), b, d,
                                   ctypes.c_float(EPS32)), "l2norm_fwd")
    _assert_guards(ybuf, NANBITS, "y")
    _assert_guards(rbuf, RN_SENTINEL, "rn")
    assert torch.equal(y.view(b, d), ops.l2_normalize(x))
    rel = (rn.cpu().double()[:, None] / c.rn64 - 1).abs()
    assert float(rel.max()) <= (d + 8) * 2.0 ** -24, float(rel.max())
    assert float(c.rn64[1]) == 1 / EPS32          # the zero row

    dy = c.dy.to(DEV)
    dbuf, dx = _guarded(b * d, BF16, NANBITS)
    yc, rc = y.clone(), rn.clone()
    ops._check(lib.l2norm_bwd_bf16(_stream(), _p(dy), _p(yc), _p(rc), _p(dx),
                                   b, d), "l2norm_bwd")
    _assert_guards(dbuf, NANBITS, "dx")
    xg = x.clone().requires_grad_()
    ops.l2_normalize(xg).backward(dy)
    assert torch.equal(dx.view(b, d), xg.grad)


def test_l2_dispatch():
    gen = torch.Generator().manual_seed(5)
    odd = torch.randn(9, 67, generator=gen).to(BF16).to(DEV)
    assert torch.equal(ops.l2_normalize(odd),
                       F.normalize(odd, dim=-1, eps=1e-12))
    cube = torch.randn(3, 5, 66, generator=gen).to(BF16).to(DEV)
    assert torch.equal(ops.l2_normalize(cube),
                       F.normalize(cube, dim=-1, eps=1e-12))
    wide = torch.randn(9, 200, generator=gen).to(BF16).to(DEV)
    sl = wide[:, 3:133]
    assert not sl.is_contiguous()
    assert torch.equal(ops.l2_normalize(sl), ops.l2_normalize(sl.contiguous()))


# ---------------------------------------------------------------------------
# 3. per-tensor e4m3 quantizer
# ---------------------------------------------------------------------------

TRIP = 2048 * 256 * 8                 # elements per grid trip

# (b, d, flat index that gets the tensor's largest magnitude, or None)
QUANT_CASES = [
    (5462, 768, TRIP + 300),          # just past one trip, max in the second
    (5462, 768, 70001),               # the same tensor, max in the first
    (1000, 120, None),
    (7, 9, None),                     # scalar tail
    (1, 5, None),                     # n < 8
    (4096, 1025, 4096 * 1025 - 1234),  # max past the full trip
    (4099, 1025, 4099 * 1025 - 1),    # max in the scalar tail past a trip
]


@functools.lru_cache(maxsize=2)
def _quant_input(b, d, at):
    gen = torch.Generator().manual_seed(b * 131 + d)
    x = (2.5 * torch.randn(b, d, generator=gen)).to(BF16)
    if at is not None:
        top = -(1.5 * x.float().abs().max()).to(BF16)
        assert float(top.abs()) > float(x.float().abs().max())
        x.view(-1)[at] = top
    return x


def _check_per_tensor(x, q, scale):
    """x bf16 on the CPU; q uint8 and scale as the op returned them."""
    xf = x.float()
    amax = xf.abs().max()
    amax_k = torch.maximum(amax, torch.tensor(2.0 ** -20))
    r = torch.tensor(448.0, dtype=torch.float32) / amax_k
    p = (xf * r).double()
    ref, dist, tie = nearest_code(p)
    excused = (dist <= 2 * ulp_fp32(p)) & ~tie
    share = float(excused.double().mean())
    assert share < 1e-3, share
    got = q.cpu().view(torch.uint8)
    bad = got != ref
    print(f"per-tensor {tuple(x.shape)}: {int(bad.sum())} differ, "
          f"{int(excused.sum())} excusable")
    assert not bool((bad & ~excused).any()), int((bad & ~excused).sum())
    near = ((got & 0x7F).int() - (ref & 0x7F).int()).abs() <= 1
    assert bool((near & ((got ^ ref) < 0x80))[bad].all())
    assert not bool(((got & 0x7F) == 0x7F).any())
    s64 = amax_k.double() / 448
    assert abs(float(scale) - float(s64)) <= float(ulp_fp32(s64))
    if float(amax) > 0:
        assert bool(((got[xf.abs() == amax] & 0x7F) == 0x7E).all())
    else:
        assert not bool(got.any())


@pytest.mark.parametrize("b,d,at", QUANT_CASES)
def test_per_tensor_quant_bytes(b, d, at):
    x = _quant_input(b, d, at)
    if at is not None:
        flat = x.view(-1).float().abs()
        assert int(flat.argmax()) == at and int((flat == flat[at]).sum()) == 1
    q, scale = ops._quant_fp8(x.to(DEV))
    assert q.dtype == E4M3 and q.shape == x.shape
    _check_per_tensor(x, q, scale)


@pytest.mark.parametrize("b,d", [(7, 9), (1000, 120)])
def test_per_tensor_quant_zeros(b, d):
    x = torch.zeros(b, d, dtype=BF16)
    q, scale = ops._quant_fp8(x.to(DEV))
    floor = torch.tensor(2.0 ** -20) / torch.tensor(448.0)      # in fp32
    assert float(scale) == float(floor)
    assert not bool(q.view(torch.uint8).any())
    _check_per_tensor(x, q, scale)


def test_per_tensor_quant_noncontiguous():
    gen = torch.Generator().manual_seed(11)
    wide = (2.5 * torch.randn(257, 100, generator=gen)).to(BF16).to(DEV)
    sl = wide[:, 5:72]
    assert not sl.is_contiguous()
    q1, s1 = ops._quant_fp8(sl)
    q2, s2 = ops._quant_fp8(sl.contiguous())
    assert torch.equal(q1.view(torch.uint8), q2.view(torch.uint8))
    assert torch.equal(s1, s2)
    _check_per_tensor(sl.cpu().contiguous(), q1, s1)


# ---------------------------------------------------------------------------
# 4. row-wise e4m3 / e8m0 quantizer
# ---------------------------------------------------------------------------

KS = (-20, -3, 0, 5, 30)
BF16_MAX = float(torch.tensor(0x7F7F, dtype=torch.int16).view(BF16))
ROW_TRIP = 1024 * 8
# kind -> amax of the row; ("k", k, j): 448 2^k moved by j bf16 steps
SPECIALS = ([("k", k, j) for k in KS for j in (0, -1, 1)]
            + [("zero",), ("max",), ("tiny",)])
THRESH = 448.0 * torch.exp2(torch.arange(-200, 128).double())   # exact

# (b, d, row of the bf16-max row or None for anywhere)
ROW_CASES = [(512, 768, None), (300, 8, None), (33, 12, None), (5, 66, None),
             (8200, 8, ROW_TRIP + 3), (8200, 8, 100)]


def _special_amax(kind):
    if kind[0] == "k":
        return (448 + 2 * kind[2]) * 2.0 ** kind[1]   # bf16 step at 448 is 2
    return {"zero": 0.0, "max": BF16_MAX, "tiny": 2.0 ** -120}[kind[0]]


def _rowwise_inputs(b, d, max_at):
    """A list of (x bf16 (b, d), {row: kind}) that together hold every special
    row; one tensor where b allows it, several otherwise."""
    gen = torch.Generator().manual_seed(7 * b + d)
    per = min(len(SPECIALS), b - 1)               # keep a plain row
    out = []
    for s0 in range(0, len(SPECIALS), per):
        kinds = SPECIALS[s0:s0 + per]
        rowexp = torch.randint(-8, 9, (b, 1), generator=gen)
        x = torch.randn(b, d, generator=gen).double() * torch.exp2(rowexp)
        rows = torch.randperm(b, generator=gen)[:len(kinds)].tolist()
        if max_at is not None:
            assert ("max",) in kinds
            i = kinds.index(("max",))
            if max_at in rows:
                rows[rows.index(max_at)] = rows[i]
            rows[i] = max_at
        placed = dict(zip(rows, kinds))
        for row, kind in placed.items():
            amax = _special_amax(kind)
            body = torch.randn(d, generator=gen).double()
            x[row] = body / body.abs().max() * 0.4 * amax if amax else 0.0
            col = int(torch.randint(0, d, (1,), generator=gen))
            if amax:
                x[row, col] = amax * (1 if row % 2 else -1)
        out.append((x.to(BF16), placed))
    return out


def _rowwise_reference(x):
    xd = x.double()
    amax = xd.abs().amax(dim=1).clamp(min=float(torch.tensor(
        1e-30, dtype=torch.float32)))
    # smallest k with amax <= 448 2^k, by comparison against exact thresholds
    k = (torch.searchsorted(THRESH, amax) - 200).clamp(-126, 127)
    code, _, _ = nearest_code(xd * torch.exp2(-k.double())[:, None])
    return k, code


@pytest.mark.parametrize("b,d,max_at", ROW_CASES)
def test_rowwise_quant_bytes_and_exponents(b, d, max_at):
    seen = set()
    for x, placed in _rowwise_inputs(b, d, max_at):
        k, code = _rowwise_reference(x)
        e8_ref = (127 + k).to(torch.uint8)
        emax = int(e8_ref.max())
        # the reference holds the rows it is meant to hold
        for row, kind in placed.items():
            amax = float(x[row].double().abs().max())
            assert amax == _special_amax(kind), (kind, amax)
            if kind[0] == "k":
                assert int(k[row]) == kind[1] + (kind[2] == 1), (kind, k[row])
            elif kind[0] == "zero":
                assert not bool(code[row].any()) and int(e8_ref[row]) < emax
            elif kind[0] == "max":
                assert int(e8_ref[row]) == emax == 247
                if max_at is not None:
                    assert row == max_at and emax > int(
                        e8_ref[torch.arange(b) != row].max())
            seen.add(kind)

        q, e8, ratio, s_ref = ops._quant_fp8_rowwise(x.to(DEV))
        got = q.cpu().view(torch.uint8)
        assert torch.equal(e8.cpu(), e8_ref), (
            (e8.cpu() != e8_ref).nonzero().flatten()[:8])
        assert torch.equal(got, code), int((got != code).sum())
        ratio_ref = torch.exp2((e8_ref.int() - emax).double()).float()
        assert torch.equal(ratio.cpu().view(torch.int32),
                           ratio_ref.view(torch.int32))
        assert float(s_ref) == 2.0 ** (emax - 127)
        # reconstruction: within half the local e4m3 step, in units of 2^k
        p = x.double() * torch.exp2(-k.double())[:, None]
        i = (torch.searchsorted(POS, p.abs(), right=True) - 1).clamp(0, 125)
        half = (POS[i + 1] - POS[i]) / 2
        assert bool(((TABLE[got.long()] - p).abs() <= half).all())
    assert seen == set(SPECIALS), set(SPECIALS) - seen


# ---------------------------------------------------------------------------
# 5. scale_bf16_
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("numel", [4096 * 256 * 8 + 2048 * 5 + 3, 3])
def test_scale_inplace_second_trip_and_tail(numel):
    gen = torch.Generator().manual_seed(numel)
    x = torch.randn(numel, generator=gen).to(DEV).to(BF16)
    s = torch.tensor(0.0123, device=DEV)
    expect = x * s.to(BF16)
    y = x.clone()
    out = ops.scale_bf16_(y, s)
    assert out.data_ptr() == y.data_ptr()
    assert torch.equal(y, expect)


# ---------------------------------------------------------------------------
# 6. wgrad, exact
# ---------------------------------------------------------------------------

WGRAD_CASES = [(1000, 136, 200, None), (1000, 136, 200, 5), (8, 128, 128, 3),
               (200, 264, 128, 64), (4128, 768, 768, None),
               (4128, 768, 768, 8), (65, 8, 8, None)]


@functools.lru_cache(maxsize=None)
def _wgrad_case(K, M, N):
    gen = torch.Generator().manual_seed(K * 7 + M + N)
    a = torch.randint(-3, 4, (K, M), generator=gen).to(BF16)
    x = torch.randint(-3, 4, (K, N), generator=gen).to(BF16)
    exact = a.double().T @ x.double()
    assert float(exact.abs().max()) < 2 ** 24
    unrep = (exact.abs() > 256) & (exact.remainder(2) == 1)
    if 4 * math.sqrt(K) >= 126:       # |v| > 256 within ~2 sigma
        assert int(unrep.sum()) > 0
    return a, x, exact.to(BF16)


@functools.lru_cache(maxsize=None)
def _wgrad_run(K, M, N, slices):
    a, x, _ = _wgrad_case(K, M, N)
    return ops.linear_wgrad(a.to(DEV), x.to(DEV), slices=slices).cpu()


@pytest.mark.parametrize("K,M,N,slices", WGRAD_CASES)
def test_wgrad_is_exact_on_integers(K, M, N, slices):
    _, _, ref = _wgrad_case(K, M, N)
    got = _wgrad_run(K, M, N, slices)
    assert got.dtype == BF16 and got.shape == (M, N)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), (
        int((got != ref).sum()))


@pytest.mark.parametrize("K,M,N,s1,s2", [(1000, 136, 200, None, 5),
                                         (4128, 768, 768, None, 8),
                                         (1000, 136, 200, 5, 1)])
def test_wgrad_slices_agree_bitwise(K, M, N, s1, s2):
    a, b = _wgrad_run(K, M, N, s1), _wgrad_run(K, M, N, s2)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_wgrad_entry_stays_inside_its_buffers():
    K, M, N, slices = 1000, 136, 200, 5
    a, x, ref = _wgrad_case(K, M, N)
    a, x = a.to(DEV), x.to(DEV)
    lib = ops._require_lib()
    dbuf, dw = _guarded(M * N, BF16, NANBITS)
    wbuf, ws = _guarded(slices * M * N, torch.float32, RN_SENTINEL)
    ops._check(lib.linear_wgrad_bf16(
        _stream(), _p(a), _p(x), _p(ws), _p(dw), K, M, N, M, N, slices),
        "linear_wgrad_bf16")
    _assert_guards(dbuf, NANBITS, "dw")
    _assert_guards(wbuf, RN_SENTINEL, "ws")
    assert torch.equal(dw.view(M, N).cpu().view(torch.int16),
                       ref.view(torch.int16))
