"""Softmax (InfoNCE) contrastive loss on CPU: the torch path against the
textbook form, column chunking, the distributed one-grid form over gloo, the
module contract and the training example.

The textbook form materialises the logits: ``CE(z, pos) + CE(zᵀ, pos)``,
summed over the rows and columns whose positive lies inside the block.
"""

from __future__ import annotations

import math
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

from distributed_sigmoid_loss_amd import (
    DistributedSoftmaxLoss,
    softmax_contrastive_loss,
)

from helpers import run_distributed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(b, n, d, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + b * 131 + n * 17 + d)
    zi = F.normalize(torch.randn(b, d, generator=g, dtype=dtype), dim=-1)
    zt = F.normalize(torch.randn(n, d, generator=g, dtype=dtype), dim=-1)
    return (zi.requires_grad_(), zt.requires_grad_(),
            torch.tensor(math.log(5.0), dtype=dtype).requires_grad_())


def _textbook(zi, zt, tp, off):
    """Sum of the row and column cross-entropies that have a target."""
    b, n = zi.shape[0], zt.shape[0]
    z = tp.exp() * zi @ zt.T
    i = torch.arange(b)
    j = i + off
    m = (j >= 0) & (j < n)
    if not bool(m.any()):
        return z.sum() * 0.0
    return (F.cross_entropy(z[i[m]], j[m], reduction="sum")
            + F.cross_entropy(z.T[j[m]], i[m], reduction="sum"))


def _grads(loss, params):
    return torch.autograd.grad(loss, params, allow_unused=True)


SHAPES = [(7, 7, 8), (5, 9, 8)]


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("off", [0, 2, -2, "n"])
def test_fp64_matches_textbook(b, n, d, off):
    off = n if off == "n" else off
    params = _inputs(b, n, d)
    got = softmax_contrastive_loss(*params, diag_offset=off, impl="torch")
    ref = _textbook(*params, off)
    assert got.dtype == torch.float64 and got.dim() == 0
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-12)
    for g, r in zip(_grads(got, params), _grads(ref, params)):
        torch.testing.assert_close(g, r, rtol=1e-9, atol=1e-12)
    if off == n:        # no positive in the block
        assert float(got.detach()) == 0.0
        assert all(float(g.abs().max()) == 0.0 for g in _grads(
            softmax_contrastive_loss(*params, diag_offset=off), params))


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("chunk", [1, 3, "n"])
def test_col_chunk_equals_unchunked(b, n, d, chunk):
    chunk = n if chunk == "n" else chunk
    params = _inputs(b, n, d, seed=1)
    ref = softmax_contrastive_loss(*params, diag_offset=1)
    got = softmax_contrastive_loss(*params, diag_offset=1, col_chunk=chunk)
    torch.testing.assert_close(got, ref, rtol=1e-10, atol=0)
    for g, r in zip(_grads(got, params), _grads(ref, params)):
        torch.testing.assert_close(g, r, rtol=1e-10, atol=1e-14)


def test_rejects_bad_arguments():
    zi, zt, tp = _inputs(4, 4, 8)
    with pytest.raises(ValueError):
        softmax_contrastive_loss(zi, zt[:, :4], tp)
    with pytest.raises(ValueError):
        softmax_contrastive_loss(zi, zt, tp, impl="triton")


# ---------------------------------------------------------------------------
# gloo: W ranks against one process on the global batch.
# ---------------------------------------------------------------------------

B_RANK, DIM = 6, 8


def _global(world):
    g = torch.Generator().manual_seed(11)
    zi = F.normalize(torch.randn(world * B_RANK, DIM, generator=g), dim=-1)
    zt = F.normalize(torch.randn(world * B_RANK, DIM, generator=g), dim=-1)
    return zi, zt


def _module_worker(rank, world, scale_by_rank):
    zi_all, zt_all = _global(world)
    sl = slice(rank * B_RANK, (rank + 1) * B_RANK)
    zi = zi_all[sl].clone().requires_grad_()
    zt = zt_all[sl].clone().requires_grad_()
    mod = DistributedSoftmaxLoss(B_RANK)
    loss = mod(zi, zt)
    (loss * (rank + 1) if scale_by_rank else loss).backward()
    # Every embedding lives on one rank: its gradient summed over ranks.
    gi = torch.zeros_like(zi_all)
    gt = torch.zeros_like(zt_all)
    gi[sl], gt[sl] = zi.grad, zt.grad
    gtp = mod.t_prime.grad.clone()
    for t in (gi, gt, gtp):
        dist.all_reduce(t)
    if rank == 0:
        return float(loss.detach()), gi, gt, gtp


def _single_process(world, weights):
    """Autograd of Σ_q w_q·loss_q with every rank's loss from the textbook
    form of its (b, W·b) block."""
    zi_all, zt_all = _global(world)
    zi = zi_all.clone().requires_grad_()
    zt = zt_all.clone().requires_grad_()
    tp = torch.tensor(math.log(1 / 0.07)).requires_grad_()
    total = 0.0
    for q in range(world):
        z = tp.exp() * zi[q * B_RANK:(q + 1) * B_RANK] @ zt.T
        tgt = torch.arange(B_RANK) + q * B_RANK
        rows = F.cross_entropy(z, tgt, reduction="sum")
        # Column LSEs run over the rows of ALL ranks.
        z_full = tp.exp() * zi @ zt.T
        cols = (torch.logsumexp(z_full, 0)[tgt] - z[torch.arange(B_RANK),
                                                    tgt]).sum()
        total = total + weights[q] * (rows + cols) / (2 * B_RANK)
    total.backward()
    return zi.grad, zt.grad, tp.grad


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_averaged_grads_match_single_rank(world):
    loss0, gi, gt, gtp = run_distributed(_module_worker, world, False)[0]
    zi_all, zt_all = _global(world)
    zi = zi_all.clone().requires_grad_()
    zt = zt_all.clone().requires_grad_()
    mod = DistributedSoftmaxLoss(world * B_RANK)
    mod(zi, zt).backward()
    # DDP averaging: the sum over ranks divided by W.
    torch.testing.assert_close(gi / world, zi.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gt / world, zt.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gtp / world, mod.t_prime.grad, rtol=1e-3,
                               atol=1e-6)
    assert math.isfinite(loss0)


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_unequal_upstream(world):
    _, gi, gt, gtp = run_distributed(_module_worker, world, True)[0]
    ri, rt, rtp = _single_process(world, [q + 1 for q in range(world)])
    torch.testing.assert_close(gi, ri, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gt, rt, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gtp, rtp, rtol=1e-3, atol=1e-6)


def _bad_layout_worker(rank, world):
    zi_all, zt_all = _global(world)
    zi = zi_all[rank * B_RANK:(rank + 1) * B_RANK]
    with pytest.raises(ValueError):
        softmax_contrastive_loss(zi, zt_all, torch.tensor(0.0),
                                 diag_offset=0 if rank else B_RANK,
                                 group=dist.group.WORLD)
    return True


def test_gloo_rejects_wrong_layout():
    assert run_distributed(_bad_layout_worker, 2)[0]


# ---------------------------------------------------------------------------
# Module and example.
# ---------------------------------------------------------------------------

def test_module_state_and_init():
    mod = DistributedSoftmaxLoss(8)
    assert list(mod.state_dict()) == ["t_prime"]
    assert float(mod.t_prime.detach()) == pytest.approx(math.log(1 / 0.07), rel=1e-6)


def test_module_single_rank_is_symmetric_clip_loss():
    zi, zt, _ = _inputs(9, 9, 8, dtype=torch.float32, seed=2)
    mod = DistributedSoftmaxLoss(9)
    z = mod.t_prime.exp() * zi @ zt.T
    tgt = torch.arange(9)
    ref = 0.5 * (F.cross_entropy(z, tgt) + F.cross_entropy(z.T, tgt))
    torch.testing.assert_close(mod(zi, zt), ref, rtol=1e-5, atol=1e-6)


def test_module_clamps_logit_scale():
    zi, zt, _ = _inputs(9, 9, 8, dtype=torch.float32, seed=3)
    mod = DistributedSoftmaxLoss(9)
    with torch.no_grad():
        mod.t_prime.fill_(math.log(100.0) + 1.0)
    loss = mod(zi, zt)
    loss.backward()
    assert float(mod.t_prime.grad) == 0.0
    ref = softmax_contrastive_loss(zi, zt, torch.tensor(math.log(100.0)),
                                   diag_offset=0) / 18
    torch.testing.assert_close(loss, ref, rtol=1e-6, atol=0)
    assert float(zi.grad.abs().max()) > 0.0


def test_example_softmax_cpu():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "train_siglip.py"),
         "--loss", "softmax", "--steps", "2", "--batch-per-gpu", "16",
         "--dim", "16", "--device", "cpu", "--log-every", "1"],
        capture_output=True, text=True, cwd=REPO)
    assert out.returncode == 0, out.stderr
    losses = [float(line.split("loss=")[1].split()[0])
              for line in out.stdout.splitlines() if "loss=" in line]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
