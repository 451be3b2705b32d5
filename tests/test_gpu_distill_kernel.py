"""The sigmoid distillation kernel (``ops.sigmoid_distill``) against float64
from the same bf16 inputs.

Shapes ``(b, n, d, d_T)``: one element; one full tile and K-step; ragged both
ways with two K tails; 10 tile-rows (walk group of 8), 20 workgroups on 8
XCDs.  Regime: unit Gaussian rows, independent for the teacher, temperatures
``log(1.5 / std(s))``, biases ``−0.5``; asserted at the larger shapes: ≥ 90 %
of ``p`` and ``σ(z)`` in ``[0.05, 0.95]``, ≥ 80 % of ``|g_ref| ≥ 0.05`` — a
dropped or swapped pair misses by thousands of ulps.

Bounds, derived.  ``g = σ(z) − q`` is a difference of probabilities whose
logits carry the fp32 accumulation error ``ε = d·2⁻²³·Σ_k|a_k·b_k|``, scaled
by the temperature and ``σ' ≤ 1/4``: every element is within 1 bf16 ulp of
``g_ref`` plus ``0.25·(t·ε + t_T·ε_T) + 2⁻¹⁹`` (absolute: the difference can
be far smaller than either probability), each scalar within ``1e-4·Σ|·|``.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops

DEV, BIAS = "cuda", -0.5
SHAPES = [(1, 1, 8, 8), (128, 128, 64, 64), (129, 257, 72, 136),
          (1157, 130, 64, 72)]
TARGETS = [(1.0, None)] + [(a, dg) for a in (0.5, 0.0)
                           for dg in (None, 0, 3, -5)]


def _pair(b, n, d, gen):
    """bf16 unit rows, t', their float64 dots and the bound ε per pair."""
    a, c = (torch.nn.functional.normalize(
        torch.randn(r, d, generator=gen), dim=-1).bfloat16() for r in (b, n))
    s = a.double() @ c.double().T
    std = float(s.std()) if s.numel() > 1 else float(s.abs().max())
    eps = d * 2.0 ** -23 * (a.double().abs() @ c.double().abs().T)
    return a.to(DEV), c.to(DEV), torch.tensor(math.log(1.5 / std),
                                              device=DEV), s, eps


@functools.lru_cache(maxsize=None)
def _case(b, n, d, d_t):
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    zi, zt, tp, s, eps = _pair(b, n, d, gen)
    ti, tt, tp_t, s_t, eps_t = _pair(b, n, d_t, gen)
    bias = torch.tensor(BIAS, device=DEV)
    t, t_t = float(tp.double().exp()), float(tp_t.double().exp())
    z, p = t * s + BIAS, torch.sigmoid(t_t * s_t + BIAS)
    for x in (p, torch.sigmoid(z)) if b > 1 else ():
        share = float(((x >= 0.05) & (x <= 0.95)).double().mean())
        assert share >= 0.9, f"uninformative regime: {share:.3f}"
    slack = 0.25 * (t * eps + t_t * eps_t) + 2.0 ** -19
    return (zi, zt, tp, bias, ti, tt, tp_t, bias), s, z, p, slack


@pytest.mark.parametrize("alpha,diag", TARGETS)
@pytest.mark.parametrize("b,n,d,d_t", SHAPES)
def test_elements_scalars_and_instantiations(b, n, d, d_t, alpha, diag):
    args, s, z, p, slack = _case(b, n, d, d_t)
    q = alpha * p
    if diag is not None:
        lo = max(0, -diag)
        i = torch.arange(lo, max(lo, min(b, n - diag)))
        q[i, i + diag] += 1.0 - alpha
    g_ref = torch.sigmoid(z) - q
    assert b == 1 or float((g_ref.abs() >= 0.05).double().mean()) >= 0.8
    parts = torch.stack([torch.nn.functional.softplus(z, threshold=1e9)
                         - q * z, g_ref * s, g_ref])
    sums, bound = parts.sum(dim=(1, 2)), 1e-4 * parts.abs().sum(dim=(1, 2))

    partials, g = ops.sigmoid_distill(*args, alpha, diag)
    tol = torch.exp2(torch.floor(torch.log2(g_ref.abs())) - 7) + slack
    off = (g.double().cpu() - g_ref).abs()
    err = (partials.double().sum(dim=0).cpu() - sums).abs()
    print(f"DISTILL {b}x{n}x{d}x{d_t} alpha={alpha} diag={diag} g_err/bound="
          f"{float((off / tol).max()):.4f} scalar_err/bound="
          + " ".join(f"{float(e / t):.4f}" for e, t in zip(err, bound)))
    assert bool((off <= tol).all()) and bool((err <= bound).all())
    # the loss-only instantiation: no g, the same bits; both reproducible
    p0, none = ops.sigmoid_distill(*args, alpha, diag, want_g=False)
    assert none is None and torch.equal(p0, partials)
    p2, g2 = ops.sigmoid_distill(*args, alpha, diag)
    assert torch.equal(p2, partials) and torch.equal(g2, g)


def test_g_band_of_a_wider_slab():
    """Odd column offset and row stride: only the view changes."""
    (b, n, _, _), args = SHAPES[2], _case(*SHAPES[2])[0]
    partials, g = ops.sigmoid_distill(*args, 0.5, 3)
    slab = torch.full((b, n + 12), 777.0, device=DEV, dtype=torch.bfloat16)
    p1, _ = ops.sigmoid_distill(*args, 0.5, 3, g=slab[:, 3:3 + n])
    assert torch.equal(p1, partials) and torch.equal(slab[:, 3:3 + n], g)
    assert bool((slab[:, :3] == 777.0).all())
    assert bool((slab[:, 3 + n:] == 777.0).all())


def test_bad_inputs_raise_before_any_launch():
    zi, zt, tp, bias, ti, tt, tp_t, bias_t = _case(*SHAPES[2])[0]
    bad = [
        (ti[:-1], tt, 0.5), (ti, tt[:-1], 0.5),          # mismatched rows
        (ti[:, :132], tt[:, :132], 0.5),                 # d_T % 8 != 0
        (ti, tt, 1.5), (ti, tt, -0.1),                   # alpha
        (ti.float(), tt.float(), 0.5),                   # not bf16
    ]
    for ti_x, tt_x, alpha in bad:
        with pytest.raises((RuntimeError, ValueError)):
            ops.sigmoid_distill(zi, zt, tp, bias, ti_x, tt_x, tp_t, bias_t,
                                alpha)
