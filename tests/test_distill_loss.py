"""``sigmoid_distillation_loss`` on the CPU: the torch composite in fp64
against a dense textbook form (loss and gradients), chunk invariance, ``alpha
= 0`` against the positional loss, the module over gloo at W = 2."""

import math

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

from distributed_sigmoid_loss_amd import (
    DistributedSigmoidDistillLoss,
    sigmoid_contrastive_loss,
    sigmoid_distillation_loss,
)
from helpers import run_distributed

B, N, D, DT, B_RANK = 13, 17, 8, 16, 5
TEACHER = (math.log(6.0), -0.25)        # t'_T, bias_T


def _inputs(b=B, n=N, seed=0):
    g = torch.Generator().manual_seed(seed)
    def rows(m, d):
        return F.normalize(torch.randn(m, d, generator=g, dtype=torch.float64),
                           dim=-1)
    tp, bias = torch.tensor([math.log(4.0), -0.5], dtype=torch.float64)
    return (rows(b, D).requires_grad_(), rows(n, D).requires_grad_(),
            tp.clone().requires_grad_(), bias.clone().requires_grad_(),
            rows(b, DT), rows(n, DT))


def _dense(zi, zt, tp, bias, ti, tt, alpha, diag):
    """Textbook form: both grids and the target written out."""
    b, n = zi.shape[0], zt.shape[0]
    z = tp.exp() * zi @ zt.T + bias
    q = alpha * torch.sigmoid(math.exp(TEACHER[0]) * ti @ tt.T + TEACHER[1])
    for i in range(b) if diag is not None else ():
        if 0 <= i + diag < n:
            q[i, i + diag] += 1 - alpha
    return (F.softplus(z) - q * z).sum()


def _assert_same(got, ref, x):
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=0)
    for a, r in zip(torch.autograd.grad(got, x[:4]),
                    torch.autograd.grad(ref, x[:4], retain_graph=True)):
        torch.testing.assert_close(a, r, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("alpha,diag", [(1.0, None), (0.5, 0), (0.3, -5),
                                        (0.0, 3)])
def test_composite_matches_dense_form_and_is_chunk_invariant(alpha, diag):
    x = _inputs()
    ref = _dense(*x, alpha, diag)
    _assert_same(sigmoid_distillation_loss(*x, *TEACHER, alpha, diag), ref, x)
    _assert_same(sigmoid_distillation_loss(*x, *TEACHER, alpha, diag,
                                           col_chunk=5), ref, x)
    with pytest.raises(ValueError, match="alpha"):
        sigmoid_distillation_loss(*x, *TEACHER, 1.5)


@pytest.mark.parametrize("diag", [None, 0, 4])
def test_alpha_zero_is_the_positional_loss(diag):
    x = _inputs()
    _assert_same(sigmoid_distillation_loss(*x, *TEACHER, 0.0, diag),
                 sigmoid_contrastive_loss(*x[:4], diag_offset=diag), x)


def _module_worker(rank, world):
    zi_all, zt_all, _, _, ti_all, tt_all = _inputs(world * B_RANK,
                                                   world * B_RANK, seed=3)
    sl = slice(rank * B_RANK, (rank + 1) * B_RANK)
    zi = zi_all.detach()[sl].clone().requires_grad_()
    zt = zt_all.detach()[sl].clone().requires_grad_()
    mod = DistributedSigmoidDistillLoss(B_RANK, 0.7, *TEACHER).double()
    (loss := mod(zi, zt, ti_all[sl], tt_all[sl])).backward()
    gi, gt = torch.zeros_like(zi_all), torch.zeros_like(zt_all)
    gi[sl], gt[sl] = zi.grad, zt.grad
    out = [loss.detach().clone(), gi, gt, mod.t_prime.grad, mod.bias.grad]
    for t in out:
        dist.all_reduce(t)
    return out if rank == 0 else None


def test_gloo_averaged_grads_match_single_rank():
    world, got = 2, run_distributed(_module_worker, 2)[0]
    zi, zt, _, _, ti, tt = _inputs(world * B_RANK, world * B_RANK, seed=3)
    mod = DistributedSigmoidDistillLoss(world * B_RANK, 0.7, *TEACHER).double()
    assert "teacher_bias" in dict(mod.named_buffers())
    ref = mod(zi, zt, ti, tt)
    ref.backward()
    # DDP averaging: the sum over ranks divided by W
    want = (ref.detach(), zi.grad, zt.grad, mod.t_prime.grad, mod.bias.grad)
    for a, r in zip(got, want):
        torch.testing.assert_close(a / world, r, rtol=1e-10, atol=1e-13)
