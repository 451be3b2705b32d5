"""The softmax distillation kernels (``ops.pair_distill_stats``,
``ops.softmax_distill_g``) against float64 from the same bf16 inputs.

Shapes ``(b, n, d, d_T)`` and regime are those of
``test_gpu_distill_kernel.py``: one element; one full tile and K-step; ragged
both ways with two K tails and a non-square grid (a swapped row and column
vector shows); 10 tile-rows against the walk group of 8.  Unit Gaussian rows,
an independent teacher, ``t' = log(1.5 / std(s))`` per pair.  Asserted on the
reference at the three larger shapes: every row and column of both grids has
its largest softmax probability under 0.9, and for ``alpha ≥ 0.5`` at least
80 % of the elements carry a teacher term ``alpha·(P^r + P^c)`` of at least 8
bf16 ulps of ``g_ref`` — a dropped or swapped teacher term misses the bound.

Bounds, derived (the manner of ``test_gpu_softmax_kernels.py``).  Per grid,
``ε = t·d·2⁻²³·max Σ_k|a_k·b_k|`` is the fp32 accumulation error of a logit
(d − 1 adds and the scale at 2⁻²⁴ of a running sum below ``Σ|ab|``, a factor
2 of slack) and ``ρ = 2⁻²⁰·(1 + max − min)`` covers v_exp_f32, v_log_f32, the
rounding of the exponent's argument and the folds.

- LSEs: ``|Δlse| ≤ E = ε + ρ`` of their grid (an LSE is 1-Lipschitz).
- ``x = Σ P·δ``, ``δ = v − z``, ``P = softmax(v)``: the logits' errors move
  ``δ`` by at most ``ε_s + ε_t`` and ``P_j`` by ``P_j·(Δv_j − Σ P·Δv)``, which
  moves x by at most ``2·ε_t·A`` with ``A = Σ P·|δ − x|``; the weighted sum
  and its normaliser are sums of about 30 roundings deep (16 in a lane, the
  shuffles, two waves, the tiles) of exp terms good to ρ_t:
  ``|Δx| ≤ ε_s + ε_t·(1 + 2A) + 4·ρ_t·Σ P·|δ|``.
- ``g``: the kernel reads the float64 LSEs rounded to fp32 and the reference
  uses those same values.  Each of the four exponentials moves by at most its
  grid's E relative, so ``|Δg| ≤ 1 bf16 ulp of g_ref + rw·Q^r·E_s + cw·Q^c·E_s
  + rtw·P^r·E_t + ctw·P^c·E_t``.
- ``Σ g·s`` within ``1e-4·Σ|g·s|`` plus the fp32 resolution of the terms g is
  a difference of, ``(6 + 2·max(|z|, |v|))·2⁻²⁴`` of each (as in
  ``test_gpu_softmax_kernels.py``): at ``(1, 1, 8, 8)`` every probability is 1
  and the float64 g is what rounding the LSEs to fp32 left over, no scale at
  all.  At the larger shapes that adds about a per cent; ``gs_rel`` printed
  below is the error against the bare ``Σ|g·s|``.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops

DEV = "cuda"
SHAPES = [(1, 1, 8, 8), (128, 128, 64, 64), (129, 257, 72, 136),
          (1157, 130, 64, 72)]
TARGETS = [(1.0, None)] + [(a, dg) for a in (0.5, 0.0)
                           for dg in (None, 0, 3, -5)]


def _pair(b, n, d, gen):
    """bf16 unit rows, t', the float64 logits and (ε, ρ) of the grid."""
    a, c = (torch.nn.functional.normalize(
        torch.randn(r, d, generator=gen), dim=-1).bfloat16().to(DEV)
        for r in (b, n))
    s = a.double() @ c.double().T
    std = float(s.std()) if s.numel() > 1 else float(s.abs().max())
    tp = torch.tensor(math.log(1.5 / std), device=DEV)
    t = float(tp.double().exp())
    eps = t * d * 2.0 ** -23 * float((a.double().abs()
                                      @ c.double().abs().T).max())
    rho = 2.0 ** -20 * (1.0 + float(s.max() - s.min()) * t)
    return a, c, tp, s, s * t, eps, rho


@functools.lru_cache(maxsize=None)
def _case(b, n, d, d_t):
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    zi, zt, tp, s, z, eps_s, rho_s = _pair(b, n, d, gen)
    ti, tt, tp_t, _, v, eps_t, rho_t = _pair(b, n, d_t, gen)
    stats, bounds = [], []
    for dim in (1, 0):
        ls, lt = torch.logsumexp(z, dim), torch.logsumexp(v, dim)
        p = torch.exp(v - lt.unsqueeze(dim))
        x = (p * (v - z)).sum(dim)
        spread = (p * (v - z - x.unsqueeze(dim)).abs()).sum(dim)
        if b > 1:
            for grid, lse in ((z, ls), (v, lt)):
                assert float(torch.exp(grid.max(dim).values - lse).max()) < 0.9
        stats += [ls, lt, x]
        bounds += [eps_s + rho_s, eps_t + rho_t,
                   eps_s + eps_t * (1.0 + 2.0 * spread)
                   + 4.0 * rho_t * (p * (v - z).abs()).sum(dim)]
    args = (zi, zt, tp, ti, tt, tp_t)
    return args, s, z, v, stats, bounds, (eps_s + rho_s, eps_t + rho_t)


def _check_stats(got, case, tag):
    worst = []
    for name, g, ref, bound in zip(ops.PairDistillStats._fields, got, case[4],
                                   case[5]):
        assert g.dtype == torch.float32 and g.shape == ref.shape
        worst.append(float(((g.double() - ref).abs() / bound).max()))
    print(f"DISTILL_STATS {tag} err/bound="
          + " ".join(f"{w:.4f}" for w in worst))
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("b,n,d,d_t", SHAPES)
def test_stats_sides_and_reruns(b, n, d, d_t):
    case = _case(b, n, d, d_t)
    both = ops.pair_distill_stats(*case[0])
    _check_stats(both, case, f"{b}x{n}x{d}x{d_t}")
    again = ops.pair_distill_stats(*case[0])
    r_only = ops.pair_distill_stats(*case[0], cols=False)
    c_only = ops.pair_distill_stats(*case[0], rows=False)
    assert r_only[3:] == (None,) * 3 and c_only[:3] == (None,) * 3
    for k in range(6):
        assert torch.equal(both[k], again[k])
        assert torch.equal(both[k], (r_only if k < 3 else c_only)[k])


def test_stats_chunks_off_the_tile_grid_fold():
    case = _case(*SHAPES[2])
    zi, zt, tp, ti, tt, tp_t = case[0]
    row, cols = None, []
    for j0 in range(0, zt.shape[0], 100):
        st = ops.pair_distill_stats(zi, zt[j0:j0 + 100], tp, ti,
                                    tt[j0:j0 + 100], tp_t)
        if row is None:
            row = st[:3]
        else:
            lt = torch.logaddexp(row[1], st[1])
            row = (torch.logaddexp(row[0], st[0]), lt,
                   torch.exp(row[1] - lt) * row[2]
                   + torch.exp(st[1] - lt) * st[2])
        cols.append(torch.stack(st[3:]))
    _check_stats((*row, *torch.cat(cols, 1)), case, "chunks of 100")


def _g_reference(case, alpha, diag, rows=True, cols=True):
    """The kernel's vectors (go = 1), float64 g from them, the element bound
    and (Σ g·s, Σ|g·s|, the scalar bound)."""
    _, s, z, v, stats, _, (e_s, e_t) = case
    b, n = z.shape
    i = torch.arange(b, device=DEV)[:, None]
    j = torch.arange(n, device=DEV)[None, :]
    pos = (j == i + diag) if diag is not None else torch.zeros_like(z).bool()
    sides, g, tol, teacher, mag = [], 0.0, 0.0, 0.0, 0.0
    for on, dim, k in ((rows, 1, 0), (cols, 0, 3)):
        if not on:
            sides.append(None)
            continue
        ls, lt = stats[k].float(), stats[k + 1].float()
        tw = torch.full_like(ls, alpha)
        hw = (1.0 - alpha) * pos.any(dim).float()
        sides.append((ls, lt, tw + hw, tw, hw))
        w, tw64, hw64 = ((tw + hw).double().unsqueeze(dim),
                         tw.double().unsqueeze(dim), hw.double().unsqueeze(dim))
        q = w * torch.exp(z - ls.double().unsqueeze(dim))
        p = tw64 * torch.exp(v - lt.double().unsqueeze(dim))
        g = g + q - p - hw64 * pos
        tol = tol + q * e_s + p * e_t
        teacher = teacher + p
        mag = mag + q + p + hw64 * pos
    ulp = torch.exp2(torch.floor(torch.log2(g.abs())) - 7)
    if alpha >= 0.5 and b > 1 and rows and cols:
        assert float((teacher >= 8 * ulp).double().mean()) >= 0.8
    gs_abs = float((g * s).abs().sum())
    res = float((mag * (6.0 + 2.0 * torch.maximum(z.abs(), v.abs()))
                 * 2.0 ** -24 * s.abs()).sum())
    return sides, g, ulp + tol, (float((g * s).sum()), gs_abs,
                                 1e-4 * gs_abs + res)


def _check_g(g, gs, ref, tag):
    _, g_ref, tol, (gs_ref, gs_abs, gs_tol) = ref
    err = (g.double() - g_ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    gs_err = abs(float(gs.double().sum()) - gs_ref)
    print(f"DISTILL_G {tag} err/bound={worst:.4f} "
          f"gs_err/bound={gs_err / max(gs_tol, 1e-300):.4f} "
          f"gs_rel={gs_err / max(gs_abs, 1e-300):.3e}")
    assert bool((err <= tol).all()), worst
    assert gs_err <= gs_tol, (gs_err, gs_tol, gs_abs)


@pytest.mark.parametrize("alpha,diag", TARGETS)
@pytest.mark.parametrize("b,n,d,d_t", SHAPES)
def test_g_elements_scalar_and_reruns(b, n, d, d_t, alpha, diag):
    case = _case(b, n, d, d_t)
    ref = _g_reference(case, alpha, diag)
    g, gs = ops.softmax_distill_g(*case[0], *ref[0], diag)
    assert g.dtype == torch.bfloat16 and g.shape == (b, n)
    assert gs.numel() == -(-b // 128) * -(-n // 128)
    _check_g(g, gs, ref, f"{b}x{n}x{d}x{d_t} alpha={alpha} diag={diag}")
    g2, gs2 = ops.softmax_distill_g(*case[0], *ref[0], diag)
    assert torch.equal(g, g2) and torch.equal(gs, gs2)


@pytest.mark.parametrize("rows,cols", [(True, False), (False, True),
                                       (False, False)])
def test_g_side_omission(rows, cols):
    case = _case(*SHAPES[2])
    if not (rows or cols):      # a skipped side is a skipped term
        g, gs = ops.softmax_distill_g(*case[0], None, None, 3)
        assert float(g.float().abs().max()) == 0.0
        assert float(gs.abs().max()) == 0.0
        return
    ref = _g_reference(case, 0.5, 3, rows, cols)
    g, gs = ops.softmax_distill_g(*case[0], *ref[0], 3)
    _check_g(g, gs, ref, f"rows={rows} cols={cols}")


def test_g_band_of_a_wider_slab():
    """Odd column offset and row stride: only the view changes."""
    (b, n, _, _), case = SHAPES[2], _case(*SHAPES[2])
    sides = _g_reference(case, 0.5, 3)[0]
    g, gs = ops.softmax_distill_g(*case[0], *sides, 3)
    slab = torch.full((b + 2, n + 12), 777.0, device=DEV,
                      dtype=torch.bfloat16)
    g1, gs1 = ops.softmax_distill_g(*case[0], *sides, 3,
                                    g=slab[1:b + 1, 3:3 + n])
    assert torch.equal(gs1, gs) and torch.equal(slab[1:b + 1, 3:3 + n], g)
    outside = torch.ones_like(slab, dtype=torch.bool)
    outside[1:b + 1, 3:3 + n] = False
    assert bool((slab[outside] == 777.0).all())


def test_bad_inputs_raise_before_any_launch():
    case = _case(*SHAPES[2])
    zi, zt, tp, ti, tt, tp_t = case[0]
    row, col = _g_reference(case, 0.5, 3)[0]
    for ti_x, tt_x in ((ti[:-1], tt), (ti, tt[:-1]),         # mismatched rows
                       (ti[:, :132], tt[:, :132]),           # d_T % 8 != 0
                       (ti.float(), tt.float())):            # not bf16
        with pytest.raises(RuntimeError):
            ops.pair_distill_stats(zi, zt, tp, ti_x, tt_x, tp_t)
        with pytest.raises(RuntimeError):
            ops.softmax_distill_g(zi, zt, tp, ti_x, tt_x, tp_t, row, col, 3)
    for bad_row in (row[:4], row[:4] + (None,), row[:4] + (row[4][:5],),
                    row[:4] + (row[4].double(),)):
        with pytest.raises(RuntimeError):
            ops.softmax_distill_g(*case[0], bad_row, col, 3)
    with pytest.raises(RuntimeError, match="g must be"):
        ops.softmax_distill_g(*case[0], row, col, 3, g=torch.empty(
            (129, 64), device=DEV, dtype=torch.bfloat16))
