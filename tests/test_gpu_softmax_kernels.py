"""The softmax-loss kernels, each on its own, against float64 computed from
the same bf16 inputs: ``ops.pair_lse`` (LSE partials + finish) and
``ops.softmax_g`` (dL/dlogit slab + per-tile ``Σ g·s``).

Shapes — the smallest at which each mechanism can fail: ``(1, 1, 8)``;
``(128, 128, 64)`` one full tile and one K-step; ``(129, 257, 72)`` ragged in
both directions plus a K tail; ``(1157, 130, 64)`` 10 tile-rows against the
block walk's locality group of 8 and 20 workgroups, not a multiple of the 8
XCDs.

Informative regime (the rule of ``test_gpu_tile_exact.py``): L2-normalised
Gaussian rows and ``t' = log(1.5 / std(s))``.  Every case first asserts that
at least 90 % of the rows and of the columns have a largest softmax
probability below 0.9, so a dropped or doubled column moves an LSE by about
``1/n`` — far outside the bound.  (At ``(1, 1, 8)`` a softmax over one
element is 1 by definition; the precondition is checked where a row has more
than one element.)

LSE bound (derived, not measured):

    |Δlse| ≤ ε = t·d·2⁻²³·max_ij Σ_k |a_ik·b_jk| + 2⁻²⁰·(1 + max z − min z)

First term: the MFMA accumulates d products in fp32; each of the d − 1 adds
and the final scale by t round at 2⁻²⁴ relative to a running sum bounded by
``Σ_k |a_ik b_jk|``, so ``|Δz| ≤ t·d·2⁻²⁴·Σ|ab|`` with a factor 2 of slack
(the bf16 products themselves are exact in fp32).  ``|Δlse| ≤ max |Δz|``
because the LSE is 1-Lipschitz in the sup norm.  Second term: v_exp_f32 and
v_log_f32 are good to about 1 ulp (2⁻²³ relative), the exponent's argument
``(z − max)·log2 e`` is rounded at 2⁻²⁴ of its magnitude, which is at most
``(max z − min z)·log2 e`` — a relative error of the term of the same size —
and the fold of the per-tile sums adds a few more roundings: together under
``2⁻²⁰·(1 + max z − min z)``, 8 ulp per unit of logit range.

g bound: ``|Δg| ≤ 1 bf16 ulp of g_ref + (row_w_i + col_w_j)·ε`` — the
rounding of the stored value plus the two exponentials, each of which moves
by at most ``Δz`` relative (``Δz`` is bounded by ε's first term alone).  The
LSEs the kernel reads are float64 ones rounded to fp32, and the reference
uses those same rounded values, so this test does not depend on the LSE
kernel.  Per-tile scalars, summed: ``1e-4·Σ|g·s|``, the project's scalar
bound, plus the fp32 resolution of the positive pairs.  There g is the
difference ``fl(row_w·p + col_w·q) − (row_w + col_w)`` with p, q near 1 where
a row's softmax is peaked (exactly 1 at ``(1, 1, 8)``, where the float64 g is
the 1e-8 left over from rounding the LSE to fp32 and ``Σ|g·s|`` is no scale
at all), so the scalar cannot resolve it below the roundings of the minuend:
two products, two sums and two v_exp_f32 results at 2⁻²⁴ each, and the
exponent's argument ``fma(s, t·log2 e, −lse·log2 e)`` at ``2·|z|·2⁻²⁴`` — in
all ``(row_w + col_w)·(6 + 2|z|)·2⁻²⁴·|s|`` per positive pair.  At the larger
shapes this adds a few per cent to the bound.
"""

import functools
import math
from typing import NamedTuple

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops

DEV = "cuda"
SHAPES = [(1, 1, 8), (128, 128, 64), (129, 257, 72), (1157, 130, 64)]
RAGGED = [(129, 257, 72), (1157, 130, 64)]
SENTINEL = 777.0


class _Case(NamedTuple):
    zi: torch.Tensor          # bf16 (b, d)
    zt: torch.Tensor          # bf16 (n, d)
    tp: torch.Tensor          # fp32 0-d, on the device
    s: torch.Tensor           # float64 (b, n) dots
    z: torch.Tensor           # float64 (b, n) logits
    row_lse: torch.Tensor     # float64
    col_lse: torch.Tensor
    eps: float                # the LSE bound


def _case(zi, zt, tp) -> _Case:
    a, bm = zi.double(), zt.double()
    s = a @ bm.T
    t = float(tp.double().exp())
    z = s * t
    absdot = float((a.abs() @ bm.abs().T).max())
    d = zi.shape[1]
    eps = (t * d * 2.0 ** -23 * absdot
           + 2.0 ** -20 * (1.0 + float(z.max()) - float(z.min())))
    return _Case(zi, zt, tp, s, z, torch.logsumexp(z, 1),
                 torch.logsumexp(z, 0), eps)


def _unit_rows(r, d, gen):
    x = torch.randn(r, d, generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).to(DEV).bfloat16()


@functools.lru_cache(maxsize=None)
def _informative(b, n, d) -> _Case:
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    zi, zt = _unit_rows(b, d, gen), _unit_rows(n, d, gen)
    s = zi.double() @ zt.double().T
    std = float(s.std()) if s.numel() > 1 else float(s.abs().max())
    tp = torch.tensor(math.log(1.5 / std), device=DEV, dtype=torch.float32)
    c = _case(zi, zt, tp)
    if n > 1:
        p = torch.exp(c.z.max(1).values - c.row_lse)
        assert float((p < 0.9).double().mean()) >= 0.9, "uninformative rows"
    if b > 1:
        p = torch.exp(c.z.max(0).values - c.col_lse)
        assert float((p < 0.9).double().mean()) >= 0.9, "uninformative cols"
    return c


def _check_lse(c: _Case, tag):
    row, col = ops.pair_lse(c.zi, c.zt, c.tp)
    assert row.dtype == torch.float32 and row.shape == c.row_lse.shape
    assert col.dtype == torch.float32 and col.shape == c.col_lse.shape
    assert bool(torch.isfinite(row).all()) and bool(torch.isfinite(col).all())
    er = float((row.double() - c.row_lse).abs().max())
    ec = float((col.double() - c.col_lse).abs().max())
    print(f"SOFTMAX_LSE {tag} eps={c.eps:.3e} row_err/eps={er / c.eps:.4f} "
          f"col_err/eps={ec / c.eps:.4f}")
    assert er <= c.eps, (er, c.eps)
    assert ec <= c.eps, (ec, c.eps)
    return row, col


@pytest.mark.parametrize("b,n,d", SHAPES)
def test_lse_informative(b, n, d):
    c = _informative(b, n, d)
    row, col = _check_lse(c, f"{b}x{n}x{d}")
    # one side at a time: the same values, the other side None
    r_only, none = ops.pair_lse(c.zi, c.zt, c.tp, cols=False)
    assert none is None and torch.equal(r_only, row)
    none, c_only = ops.pair_lse(c.zi, c.zt, c.tp, rows=False)
    assert none is None and torch.equal(c_only, col)
    assert ops.pair_lse(c.zi, c.zt, c.tp, rows=False, cols=False) == (None,
                                                                      None)


def test_lse_overflow_range():
    """A quarter of the text rows equal their image rows and t = 100: z
    reaches 100 and exp overflows fp32 unless the max is subtracted."""
    b, n, d = RAGGED[0]
    gen = torch.Generator().manual_seed(3)
    zi, zt = _unit_rows(b, d, gen), _unit_rows(n, d, gen)
    idx = torch.arange(0, b, 4, device=DEV)
    zt[idx] = zi[idx]
    tp = torch.tensor(math.log(100.0), device=DEV, dtype=torch.float32)
    c = _case(zi, zt, tp)
    assert float(c.z.max()) > 95.0
    _check_lse(c, "overflow")


def test_lse_negative_logits_padding_does_not_leak():
    """zimg_i = v and ztxt_j = −v with t = 100: every z is −100·|v|² and every
    LSE is that plus log(count); a padding column (z = 0) leaking into a
    ragged tile would give about 0."""
    b, n, d = RAGGED[0]
    gen = torch.Generator().manual_seed(4)
    v = _unit_rows(1, d, gen)
    zi, zt = v.expand(b, d).contiguous(), (-v).expand(n, d).contiguous()
    tp = torch.tensor(math.log(100.0), device=DEV, dtype=torch.float32)
    c = _case(zi, zt, tp)
    z0 = float(c.z[0, 0])
    assert -101.0 < z0 < -99.0
    row, col = _check_lse(c, "negative")
    assert abs(float(row[0]) - (z0 + math.log(n))) < 1e-3
    assert abs(float(col[-1]) - (z0 + math.log(b))) < 1e-3


@pytest.mark.parametrize("b,n,d", SHAPES)
def test_lse_reproducible(b, n, d):
    c = _informative(b, n, d)
    r1, c1 = ops.pair_lse(c.zi, c.zt, c.tp)
    r2, c2 = ops.pair_lse(c.zi, c.zt, c.tp)
    assert torch.equal(r1, r2) and torch.equal(c1, c2)


# ---------------------------------------------------------------------------
# g kernel
# ---------------------------------------------------------------------------

class _GRef(NamedTuple):
    row_lse: torch.Tensor     # fp32: what the kernel reads
    col_lse: torch.Tensor
    row_w: torch.Tensor
    col_w: torch.Tensor
    g: torch.Tensor           # float64 (b, n)
    tol: torch.Tensor         # float64 (b, n) element bound
    gs: float                 # Σ g·s
    gs_abs: float             # Σ |g·s|
    gs_tol: float             # the scalar bound


@functools.lru_cache(maxsize=None)
def _g_reference(b, n, d, diag, rows=True, cols=True) -> _GRef:
    c = _informative(b, n, d)
    gen = torch.Generator().manual_seed(b + 31 * n)
    row_w = (0.5 + torch.rand(b, generator=gen)).to(DEV)
    col_w = (0.5 + torch.rand(n, generator=gen)).to(DEV)
    row_lse, col_lse = c.row_lse.float(), c.col_lse.float()
    g = torch.zeros_like(c.z)
    w = torch.zeros_like(c.z)
    if rows:
        g += row_w.double()[:, None] * torch.exp(
            c.z - row_lse.double()[:, None])
        w += row_w.double()[:, None]
    if cols:
        g += col_w.double()[None, :] * torch.exp(
            c.z - col_lse.double()[None, :])
        w += col_w.double()[None, :]
    i = torch.arange(b, device=DEV)[:, None]
    j = torch.arange(n, device=DEV)[None, :]
    pos = j == i + diag
    g -= w * pos
    ulp = torch.exp2(torch.floor(torch.log2(g.abs())) - 7)
    gs_abs = float((g * c.s).abs().sum())
    cancel = float((w * (6.0 + 2.0 * c.z.abs()) * 2.0 ** -24
                    * c.s.abs())[pos].sum())
    return _GRef(row_lse, col_lse, row_w, col_w, g, ulp + w * c.eps,
                 float((g * c.s).sum()), gs_abs, 1e-4 * gs_abs + cancel)


def _check_g(got, gs, ref: _GRef, tag):
    err = (got.double() - ref.g).abs()
    worst = float((err / ref.tol.clamp_min(1e-300)).max())
    gs_err = abs(float(gs.double().sum()) - ref.gs)
    print(f"SOFTMAX_G {tag} err/bound={worst:.4f} "
          f"gs_err/bound={gs_err / max(ref.gs_tol, 1e-300):.4f} "
          f"gs_rel={gs_err / max(ref.gs_abs, 1e-300):.3e}")
    assert bool((err <= ref.tol).all()), worst
    assert gs_err <= ref.gs_tol, (gs_err, ref.gs_tol, ref.gs_abs)


def _diag(n, diag):
    return n if diag == "n" else diag


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("diag", [0, 128 + 3, -5, "n"])
def test_g_elements_and_scalar(b, n, d, diag):
    diag = _diag(n, diag)
    c = _informative(b, n, d)
    ref = _g_reference(b, n, d, diag)
    g, gs = ops.softmax_g(c.zi, c.zt, c.tp, ref.row_lse, ref.row_w,
                          ref.col_lse, ref.col_w, diag)
    assert g.dtype == torch.bfloat16 and g.shape == (b, n)
    assert gs.dtype == torch.float32
    assert gs.numel() == -(-b // 128) * -(-n // 128)
    _check_g(g, gs, ref, f"{b}x{n}x{d}-diag{diag}")
    g2, gs2 = ops.softmax_g(c.zi, c.zt, c.tp, ref.row_lse, ref.row_w,
                            ref.col_lse, ref.col_w, diag)
    assert torch.equal(g, g2) and torch.equal(gs, gs2)


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("side", ["rows", "cols"])
def test_g_side_omission(b, n, d, side):
    diag = 2
    c = _informative(b, n, d)
    rows = side == "rows"
    ref = _g_reference(b, n, d, diag, rows=rows, cols=not rows)
    zero_r, zero_c = torch.zeros_like(ref.row_w), torch.zeros_like(ref.col_w)
    if rows:
        one = ops.softmax_g(c.zi, c.zt, c.tp, ref.row_lse, ref.row_w, None,
                            None, diag)
        two = ops.softmax_g(c.zi, c.zt, c.tp, ref.row_lse, ref.row_w,
                            ref.col_lse, zero_c, diag)
    else:
        one = ops.softmax_g(c.zi, c.zt, c.tp, None, None, ref.col_lse,
                            ref.col_w, diag)
        two = ops.softmax_g(c.zi, c.zt, c.tp, ref.row_lse, zero_r,
                            ref.col_lse, ref.col_w, diag)
    _check_g(one[0], one[1], ref, f"{b}x{n}x{d}-{side}-only")
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


def test_g_without_sides_is_zero():
    """A skipped side is a skipped term: with both skipped, g and every
    per-tile scalar are exactly 0."""
    b, n, d = RAGGED[0]
    c = _informative(b, n, d)
    g, gs = ops.softmax_g(c.zi, c.zt, c.tp, None, None, None, None, 0)
    assert float(g.float().abs().max()) == 0.0
    assert float(gs.abs().max()) == 0.0


@pytest.mark.parametrize("b,n,d", RAGGED)
@pytest.mark.parametrize("c0", [0, 8, 3])
def test_g_strided_view_stays_inside(b, n, d, c0):
    diag = 1
    c = _informative(b, n, d)
    ref = _g_reference(b, n, d, diag)
    width = -(-(c0 + n + 5) // 8) * 8       # rows 16-byte aligned at c0 % 8 == 0
    slab = torch.full((b + 2, width), SENTINEL, device=DEV,
                      dtype=torch.bfloat16)
    view = slab[1:b + 1, c0:c0 + n]
    g, gs = ops.softmax_g(c.zi, c.zt, c.tp, ref.row_lse, ref.row_w,
                          ref.col_lse, ref.col_w, diag, g=view)
    assert g.data_ptr() == view.data_ptr()
    _check_g(view, gs, ref, f"{b}x{n}x{d}-c0={c0}")
    outside = torch.ones_like(slab, dtype=torch.bool)
    outside[1:b + 1, c0:c0 + n] = False
    assert torch.equal(slab[outside],
                       torch.full_like(slab[outside], SENTINEL))
    dense, _ = ops.softmax_g(c.zi, c.zt, c.tp, ref.row_lse, ref.row_w,
                             ref.col_lse, ref.col_w, diag)
    assert torch.equal(view, dense)


def test_validation_errors():
    c = _informative(*SHAPES[1])
    with pytest.raises(RuntimeError, match="bf16"):
        ops.pair_lse(c.zi.float(), c.zt, c.tp)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.pair_lse(c.zi[:, :4], c.zt[:, :4], c.tp)
    lse = torch.zeros(128, device=DEV)
    with pytest.raises(RuntimeError, match="together"):
        ops.softmax_g(c.zi, c.zt, c.tp, lse, None, None, None, 0)
    with pytest.raises(RuntimeError, match="row_w"):
        ops.softmax_g(c.zi, c.zt, c.tp, lse, lse[:5], None, None, 0)
    with pytest.raises(RuntimeError, match="g must be"):
        ops.softmax_g(c.zi, c.zt, c.tp, lse, lse, None, None, 0,
                      g=torch.empty((128, 64), device=DEV,
                                    dtype=torch.bfloat16))
