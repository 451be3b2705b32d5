"""The distillation kernels with an MXFP8 teacher (``ops.sigmoid_distill_mx``,
``ops.pair_distill_stats_mx``, ``ops.softmax_distill_g_mx``).

Shapes ``(b, n, d, d_T)``: one element, a quarter K-step; one full tile, one MX
step; ragged both ways, a step plus a one-block tail; 10 tile-rows, three
steps plus a tail.

1. Bits.  Teacher values ``m·2^k``, integer ``|m| ≤ 3``, ``k`` per (row,
   32-block) in ``−2 … 2``: ``quantize_mx`` is exact on them (asserted) and
   every dot is exact in fp32 in any order, so the three ops must return the
   bits of their bf16-teacher siblings.  Each operand carries ≥ 4 distinct
   scale bytes (the one it has at ``(1, 1, 8, 32)``) and some scale row two
   (at ``d_T = 32`` the second is the pad byte).
2. Float64 from the dequantised values at real block scales
   (``test_gpu_id_labels_mx.py``'s operand, ``k`` in ``−6 … 6``), with the
   bounds of ``test_gpu_distill_kernel.py`` and
   ``test_gpu_softmax_distill_kernel.py`` and ``ε_T = EPS_T_SCALE·d_T·2⁻²³·
   Σ|a_k·b_k|`` over the dequantised teacher; ``EPS_T_SCALE = 1``, the plain
   fp32 summation model, holds (worst ratio 0.4975).
3. ``g`` as an odd-offset band of a wider slab; bad inputs raise.
"""

import functools
import math

import pytest
import torch

from distributed_sigmoid_loss_amd import ops
from test_gpu_distill_kernel import BIAS, DEV, _pair     # skips without a GPU
import test_gpu_softmax_distill_kernel as sm
from test_gpu_id_labels_mx import _mx_operand

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 8, 32), (128, 128, 64, 128), (129, 257, 72, 160),
          (1157, 130, 64, 416)]
TARGETS = [(1.0, None), (0.5, 3), (0.5, -5)]
EPS_T_SCALE = 1.0


def _dequant(q, e8):
    scale = torch.exp2(e8[:, :q.shape[1] // 32].double() - 127)
    return q.float().double() * scale.repeat_interleave(32, dim=1)


def _tprime(s):
    std = float(s.std()) if s.numel() > 1 else float(s.abs().max())
    return torch.tensor(math.log(1.5 / std), device=DEV)


def _exact_operand(r, d_t, gen):
    m = torch.randint(-3, 4, (r, d_t // 32, 32), generator=gen).float()
    k = torch.randint(-2, 3, (r, d_t // 32, 1), generator=gen).float()
    x = (m * torch.exp2(k)).reshape(r, d_t).bfloat16().to(DEV)
    q, e8 = ops.quantize_mx(x)
    assert torch.equal(_dequant(q, e8), x.double()), "quantize_mx not exact"
    real = e8[:, :d_t // 32]
    assert len(real.unique()) >= min(4, real.numel())
    assert bool((e8 != e8[:, :1]).any()), "no row with two scale bytes"
    return x, (q, e8)


@functools.lru_cache(maxsize=None)
def _exact_case(b, n, d, d_t):
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d_t)
    zi, zt, tp, _, _ = _pair(b, n, d, gen)
    (ti, ti_mx), (tt, tt_mx) = (_exact_operand(r, d_t, gen) for r in (b, n))
    s_t = ti.double() @ tt.double().T
    tp_t = _tprime(s_t)
    p = torch.sigmoid(float(tp_t.double().exp()) * s_t + BIAS)
    assert b == 1 or float(((p >= 0.05) & (p <= 0.95)).double().mean()) >= 0.9
    return (zi, zt, tp), (ti, tt), ti_mx + tt_mx, tp_t


def _same(got, ref):
    return all((x is None and y is None) or torch.equal(x, y)
               for x, y in zip(got, ref))


@pytest.mark.parametrize("alpha,diag", TARGETS)
@pytest.mark.parametrize("b,n,d,d_t", SHAPES)
def test_exact_dots_give_the_bf16_teacher_bits(b, n, d, d_t, alpha, diag):
    (zi, zt, tp), bf, mx, tp_t = _exact_case(b, n, d, d_t)
    bias = torch.tensor(BIAS, device=DEV)
    for want_g in (True, False):
        tail = (tp_t, bias, alpha, diag, None, want_g)
        assert _same(ops.sigmoid_distill_mx(zi, zt, tp, bias, *mx, *tail),
                     ops.sigmoid_distill(zi, zt, tp, bias, *bf, *tail))
    st = ops.pair_distill_stats(zi, zt, tp, *bf, tp_t)
    assert _same(ops.pair_distill_stats_mx(zi, zt, tp, *mx, tp_t), st)
    sides = [(ls, lt, torch.ones_like(ls), torch.full_like(ls, alpha),
              torch.full_like(ls, 1.0 - alpha))
             for ls, lt in ((st[0], st[1]), (st[3], st[4]))]
    assert _same(ops.softmax_distill_g_mx(zi, zt, tp, *mx, tp_t, *sides, diag),
                 ops.softmax_distill_g(zi, zt, tp, *bf, tp_t, *sides, diag))


@functools.lru_cache(maxsize=None)
def _scaled_case(b, n, d, d_t):
    """Student pair, MX teacher and both references' ingredients."""
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d_t + 1)
    zi, zt, tp, s, z, eps_s, rho_s = sm._pair(b, n, d, gen)
    (ti_q, ti_e8, ti), (tt_q, tt_e8, tt) = (_mx_operand(r, d_t, gen)
                                            for r in (b, n))
    s_t = ti @ tt.T
    tp_t = _tprime(s_t)
    t, t_t = float(tp.double().exp()), float(tp_t.double().exp())
    v, abs_t = s_t * t_t, EPS_T_SCALE * d_t * 2.0 ** -23 * (ti.abs()
                                                            @ tt.abs().T)
    # the sigmoid op: test_gpu_distill_kernel.py's slack per element
    abs_s = d * 2.0 ** -23 * (zi.double().abs() @ zt.double().abs().T)
    slack = 0.25 * (t * abs_s + t_t * abs_t) + 2.0 ** -19
    # the softmax ops: test_gpu_softmax_distill_kernel.py's case
    eps_t = t_t * float(abs_t.max())
    rho_t = 2.0 ** -20 * (1.0 + float(s_t.max() - s_t.min()) * t_t)
    stats, bounds = [], []
    for dim in (1, 0):
        ls, lt = torch.logsumexp(z, dim), torch.logsumexp(v, dim)
        p = torch.exp(v - lt.unsqueeze(dim))
        x = (p * (v - z)).sum(dim)
        spread = (p * (v - z - x.unsqueeze(dim)).abs()).sum(dim)
        stats += [ls, lt, x]
        bounds += [eps_s + rho_s, eps_t + rho_t,
                   eps_s + eps_t * (1.0 + 2.0 * spread)
                   + 4.0 * rho_t * (p * (v - z).abs()).sum(dim)]
    case = ((zi, zt, tp), s, z, v, stats, bounds,
            (eps_s + rho_s, eps_t + rho_t))
    return case, (ti_q, ti_e8, tt_q, tt_e8), tp_t, slack


@pytest.mark.parametrize("alpha,diag", TARGETS[:2])
@pytest.mark.parametrize("b,n,d,d_t", SHAPES[2:])
def test_float64_at_real_block_scales(b, n, d, d_t, alpha, diag):
    case, mx, tp_t, slack = _scaled_case(b, n, d, d_t)
    (zi, zt, tp), s, z, v = case[:4]
    tag = f"{b}x{n}x{d}x{d_t} alpha={alpha} diag={diag}"
    bias = torch.tensor(BIAS, device=DEV)
    zb, i = z + BIAS, torch.arange(b, device=DEV)[:, None]
    q = alpha * torch.sigmoid(v + BIAS)
    if diag is not None:
        q = q + (1.0 - alpha) * (torch.arange(n, device=DEV)[None, :]
                                 == i + diag)
    g_ref = torch.sigmoid(zb) - q
    parts = torch.stack([torch.nn.functional.softplus(zb, threshold=1e9)
                         - q * zb, g_ref * s, g_ref])
    sums, bound = parts.sum(dim=(1, 2)), 1e-4 * parts.abs().sum(dim=(1, 2))
    partials, g = ops.sigmoid_distill_mx(zi, zt, tp, bias, *mx, tp_t, bias,
                                         alpha, diag)
    tol = torch.exp2(torch.floor(torch.log2(g_ref.abs())) - 7) + slack
    off = (g.double() - g_ref).abs()
    err = (partials.double().sum(dim=0) - sums).abs()
    print(f"DISTILL_MX {tag} g_err/bound={float((off / tol).max()):.4f} "
          "scalar_err/bound="
          + " ".join(f"{float(e / t):.4f}" for e, t in zip(err, bound)))
    assert bool((off <= tol).all()) and bool((err <= bound).all())

    sm._check_stats(ops.pair_distill_stats_mx(zi, zt, tp, *mx, tp_t), case,
                    "mx " + tag)
    ref = sm._g_reference(case, alpha, diag)
    g, gs = ops.softmax_distill_g_mx(zi, zt, tp, *mx, tp_t, *ref[0], diag)
    sm._check_g(g, gs, ref, "mx " + tag)


def test_g_band_of_a_wider_slab():
    """Odd column offset and row stride: only the view changes."""
    (b, n, d, d_t) = SHAPES[2]
    (zi, zt, tp), _, mx, tp_t = _exact_case(b, n, d, d_t)
    bias = torch.tensor(BIAS, device=DEV)
    args = (zi, zt, tp, bias, *mx, tp_t, bias, 0.5, 3)
    partials, g = ops.sigmoid_distill_mx(*args)
    slab = torch.full((b, n + 12), 777.0, device=DEV, dtype=torch.bfloat16)
    p1, _ = ops.sigmoid_distill_mx(*args, g=slab[:, 3:3 + n])
    assert torch.equal(p1, partials) and torch.equal(slab[:, 3:3 + n], g)
    assert bool((slab[:, :3] == 777.0).all())
    assert bool((slab[:, 3 + n:] == 777.0).all())


@pytest.mark.parametrize("edit", [
    lambda m: [m[0][:, :48].contiguous(), m[1][:, :4].contiguous(),
               m[2][:, :48].contiguous(), m[3][:, :4].contiguous()],  # d_T % 32
    lambda m: [m[0], m[1].view(torch.int8), m[2], m[3]],         # e8 dtype
    lambda m: [m[0], m[1], m[2], m[3][:, :4].contiguous()],      # e8 width
    lambda m: [m[0], m[1][:-1], m[2], m[3]],                     # e8 rows
    lambda m: [m[0], m[1], m[2].view(torch.uint8).repeat(1, 2)       # q strided
               [:, :m[2].shape[1]].view(m[2].dtype), m[3]],
    lambda m: [m[0][:-1], m[1][:-1], m[2], m[3]],                # teacher rows
])
def test_bad_inputs_raise_before_any_launch(edit):
    (zi, zt, tp), _, mx, tp_t = _exact_case(*SHAPES[2])
    bias = torch.tensor(BIAS, device=DEV)
    bad = edit(list(mx))
    with pytest.raises(RuntimeError):
        ops.sigmoid_distill_mx(zi, zt, tp, bias, *bad, tp_t, bias, 0.5)
    with pytest.raises(RuntimeError):
        ops.pair_distill_stats_mx(zi, zt, tp, *bad, tp_t)
    with pytest.raises(RuntimeError):
        ops.softmax_distill_g_mx(zi, zt, tp, *bad, tp_t, None, None, 3)
    for alpha in (1.5, -0.1):
        with pytest.raises(ValueError):
            ops.sigmoid_distill_mx(zi, zt, tp, bias, *mx, tp_t, bias, alpha)
