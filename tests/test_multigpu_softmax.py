"""Distributed softmax loss on RCCL at W = 2: every rank's loss and local
gradients must equal the single-GPU run on the global batch, sliced.

GPU-marked and skipped below 2 visible GPUs.  The single-GPU run evaluates
each rank's ``(B, W·B)`` block with the column LSEs of the whole grid, which
is what the one-grid distributed form computes; tolerances are those of
``test_gpu_softmax_loss.py``.
"""

from __future__ import annotations

import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

N_GPUS = torch.cuda.device_count()
needs2 = pytest.mark.skipif(N_GPUS < 2, reason="needs >=2 GPUs")

B, D = 200, 72    # per-rank batch (ragged against the 128-wide tile), emb dim
EMB_TOL = dict(rtol=5e-2, atol=5e-4)
TP_TOL = dict(rtol=2e-2, atol=1e-3)


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _global_batch(world: int):
    g = torch.Generator().manual_seed(5)
    zi = F.normalize(torch.randn(world * B, D, generator=g), dim=-1)
    zt = F.normalize(torch.randn(world * B, D, generator=g), dim=-1)
    return zi.bfloat16(), zt.bfloat16()


def _rank_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    try:
        from distributed_sigmoid_loss_amd import DistributedSoftmaxLoss
        zi_all, zt_all = _global_batch(world)
        zi = zi_all[rank * B:(rank + 1) * B].cuda(rank).requires_grad_()
        zt = zt_all[rank * B:(rank + 1) * B].cuda(rank).requires_grad_()
        mod = DistributedSoftmaxLoss(B, impl="hip").cuda(rank)
        loss = mod(zi, zt)
        loss.backward()
        torch.cuda.synchronize()
        ret[rank] = (loss.detach().cpu(), zi.grad.cpu(), zt.grad.cpu(),
                     mod.t_prime.grad.cpu())
    finally:
        dist.destroy_process_group()


@needs2
def test_rccl_loss_and_grads_equal_single_gpu_slices():
    from distributed_sigmoid_loss_amd import DistributedSoftmaxLoss
    world = 2
    zi_all, zt_all = _global_batch(world)
    zi = zi_all.cuda().requires_grad_()
    zt = zt_all.cuda().requires_grad_()
    # Single GPU on the global batch: total / (2·W·B); a rank's gradients are
    # those of Σ_q loss_q = W × that.
    ref_mod = DistributedSoftmaxLoss(world * B, impl="hip").cuda()
    ref_loss = ref_mod(zi, zt)
    (ref_loss * world).backward()

    manager = mp.Manager()
    ret = manager.dict()
    mp.spawn(_rank_worker, args=(world, free_port(), ret), nprocs=world,
             join=True)

    # Each rank's own loss from the materialised fp32 logits of the grid.
    z = ref_mod.t_prime.detach().exp() * zi.detach().float() @ \
        zt.detach().float().T
    row_ce = torch.logsumexp(z, 1) - z.diagonal()
    col_ce = torch.logsumexp(z, 0) - z.diagonal()
    per_rank = (row_ce + col_ce).view(world, B).sum(1) / (2 * B)

    loss_sum, dtp_sum = 0.0, 0.0
    for rank in range(world):
        loss, dzi, dzt, dtp = ret[rank]
        sl = slice(rank * B, (rank + 1) * B)
        torch.testing.assert_close(loss, per_rank[rank].cpu(), rtol=1e-4,
                                   atol=0)
        torch.testing.assert_close(dzi.float(), zi.grad[sl].float().cpu(),
                                   **EMB_TOL)
        torch.testing.assert_close(dzt.float(), zt.grad[sl].float().cpu(),
                                   **EMB_TOL)
        loss_sum, dtp_sum = loss_sum + loss, dtp_sum + dtp
    torch.testing.assert_close(loss_sum / world, ref_loss.detach().cpu(),
                               rtol=1e-4, atol=0)
    torch.testing.assert_close(dtp_sum, ref_mod.t_prime.grad.cpu(), **TP_TOL)
    assert math.isfinite(float(loss_sum))
