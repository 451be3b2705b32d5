"""The softmax distillation loss on CPU: the chunked composite in float64
against a dense textbook form (``log_softmax`` and autograd), chunk
invariance, the two ends of ``alpha``, the one-grid form over gloo, and
validation."""

import math

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

import distributed_sigmoid_loss_amd as pkg
from distributed_sigmoid_loss_amd import (
    DistributedSoftmaxDistillLoss,
    softmax_contrastive_loss,
    softmax_distillation_loss,
)
from helpers import run_distributed

B, N, D, D_T, TP, TP_T = 7, 11, 8, 16, math.log(9.0), math.log(6.0)


def _inputs(b=B, n=N, dtype=torch.float64, seed=5):
    g = torch.Generator().manual_seed(seed)
    zi, zt, ti, tt = (F.normalize(torch.randn(r, d, generator=g,
                                              dtype=dtype), dim=-1)
                      for r, d in ((b, D), (n, D), (b, D_T), (n, D_T)))
    return (zi.requires_grad_(), zt.requires_grad_(),
            torch.tensor(TP, dtype=dtype).requires_grad_(), ti, tt)


def _textbook(zi, zt, tp, ti, tt, alpha, diag):
    z, v = tp.exp() * zi @ zt.T, math.exp(TP_T) * ti @ tt.T
    total = 0.0
    for dim in (1, 0):
        logp, logq = F.log_softmax(v, dim), F.log_softmax(z, dim)
        total = total + alpha * (logp.exp() * (logp - logq)).sum()
        if diag is not None:
            i = torch.arange(max(0, -diag), min(z.shape[0], z.shape[1] - diag))
            total = total - (1 - alpha) * logq[i, i + diag].sum()
    return total


def _grads(total, *leaves):
    return torch.autograd.grad(total, leaves)


@pytest.mark.parametrize("alpha,diag", [(1.0, None), (0.5, 0), (0.3, 3),
                                        (0.5, -2), (0.0, 1)])
@pytest.mark.parametrize("col_chunk", [None, 4])
def test_composite_matches_textbook(alpha, diag, col_chunk):
    zi, zt, tp, ti, tt = _inputs()
    got = softmax_distillation_loss(zi, zt, tp, ti, tt, TP_T, alpha, diag,
                                    col_chunk=col_chunk, impl="torch")
    ref = _textbook(zi, zt, tp, ti, tt, alpha, diag)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    for a, r in zip(_grads(got, zi, zt, tp), _grads(ref, zi, zt, tp)):
        torch.testing.assert_close(a, r, rtol=1e-10, atol=1e-12)
    assert ti.grad is None and tt.grad is None


def test_alpha_zero_is_the_hard_loss():
    zi, zt, tp, ti, tt = _inputs()
    got = softmax_distillation_loss(zi, zt, tp, ti, tt, TP_T, 0.0, 2,
                                    impl="torch")
    ref = softmax_contrastive_loss(zi, zt, tp, 2, impl="torch")
    torch.testing.assert_close(got, ref, rtol=1e-13, atol=1e-13)
    for a, r in zip(_grads(got, zi, zt, tp), _grads(ref, zi, zt, tp)):
        torch.testing.assert_close(a, r, rtol=1e-12, atol=1e-14)


def test_student_equal_to_teacher_is_a_zero_of_the_pure_loss():
    zi, zt, _, _, _ = _inputs()
    tp = torch.tensor(TP_T, dtype=torch.float64).requires_grad_()
    got = softmax_distillation_loss(zi, zt, tp, zi.detach(), zt.detach(),
                                    TP_T, 1.0, col_chunk=4, impl="torch")
    assert abs(float(got.detach())) < 1e-13
    for a in _grads(got, zi, zt, tp):
        assert float(a.abs().max()) < 1e-13
    other = softmax_distillation_loss(*_inputs(), TP_T, 1.0, impl="torch")
    assert float(other.detach()) > 1e-3


# gloo: W = 2 ranks against the single-process gradients of Σ_q w_q·loss_q.
B_RANK = 5


def _module_worker(rank, world):
    zi_all, zt_all, _, ti_all, tt_all = _inputs(world * B_RANK, world * B_RANK,
                                                torch.float32)
    sl = slice(rank * B_RANK, (rank + 1) * B_RANK)
    zi = zi_all.detach()[sl].clone().requires_grad_()
    zt = zt_all.detach()[sl].clone().requires_grad_()
    mod = DistributedSoftmaxDistillLoss(B_RANK, 0.6, TP_T, col_chunk=4)
    (mod(zi, zt, ti_all[sl], tt_all[sl]) * (rank + 1)).backward()
    gi, gt = torch.zeros_like(zi_all), torch.zeros_like(zt_all)
    gi[sl], gt[sl] = zi.grad, zt.grad
    gtp = mod.t_prime.grad.clone()
    for t in (gi, gt, gtp):
        dist.all_reduce(t)
    if rank == 0:
        return gi, gt, gtp


def test_gloo_unequal_upstream_matches_single_process():
    world = 2
    gi, gt, gtp = run_distributed(_module_worker, world)[0]
    zi, zt, _, ti, tt = _inputs(world * B_RANK, world * B_RANK, torch.float32)
    tp = torch.tensor(math.log(1 / 0.07)).requires_grad_()
    z, v = tp.exp() * zi @ zt.T, math.exp(TP_T) * ti @ tt.T
    total = 0.0
    for q in range(world):
        own = torch.arange(B_RANK) + q * B_RANK
        for dim, pick in ((1, lambda x: x[own]), (0, lambda x: x[:, own])):
            logp, logq = F.log_softmax(v, dim), F.log_softmax(z, dim)
            kl = pick(logp.exp() * (logp - logq)).sum()
            hard = -logq[own, own].sum()
            total = total + (q + 1) * (0.6 * kl + 0.4 * hard) / (2 * B_RANK)
    for a, r in zip((gi, gt, gtp), _grads(total, zi, zt, tp)):
        torch.testing.assert_close(a, r, rtol=1e-3, atol=1e-6)


def test_validation_and_exports():
    zi, zt, tp, ti, tt = _inputs()
    assert {"softmax_distillation_loss",
            "DistributedSoftmaxDistillLoss"} <= set(pkg.__all__)
    for bad in (dict(alpha=1.5), dict(alpha=-0.1), dict(impl="triton")):
        with pytest.raises(ValueError):
            softmax_distillation_loss(zi, zt, tp, ti, tt, TP_T,
                                      **{"impl": "torch", **bad})
    for ti_x, tt_x in ((ti[:-1], tt), (ti, tt[:-1]), (ti[:, :8], tt)):
        with pytest.raises(ValueError):
            softmax_distillation_loss(zi, zt, tp, ti_x, tt_x, TP_T,
                                      impl="torch")
    with pytest.raises(ValueError):
        DistributedSoftmaxDistillLoss(8, 2.0, TP_T)
    with pytest.raises(RuntimeError):    # no quiet fall-back from hip
        softmax_distillation_loss(zi, zt, tp, ti, tt, TP_T, impl="hip")
