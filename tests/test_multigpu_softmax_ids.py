"""``DistributedSoftmaxLoss`` with sample ids on RCCL at W = 2: the ranks'
gradients, averaged, must equal the single-GPU gradients of the global batch.

GPU-marked and skipped below 2 visible GPUs.  Ids repeat within and across
ranks — the positives of a column sit on both ranks — and one sample per side
is masked; tolerances are the bf16 class of ``test_gpu_softmax_id_loss.py``
(gradients at the module's ``1 / (2 b)`` normalisation).
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
SCALAR_TOL = dict(rtol=2e-2, atol=1e-3)


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
    values = world * B // 3
    img = torch.randint(0, values, (world * B,), generator=g)
    txt = torch.randint(0, values, (world * B,), generator=g)
    img[1], txt[world * B - 2] = -1, -1
    return zi.bfloat16(), zt.bfloat16(), img, txt


def _rank_worker(rank, world, port, duplicates, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    try:
        from distributed_sigmoid_loss_amd import DistributedSoftmaxLoss
        zi_all, zt_all, img, txt = _global_batch(world)
        sl = slice(rank * B, (rank + 1) * B)
        zi = zi_all[sl].cuda(rank).requires_grad_()
        zt = zt_all[sl].cuda(rank).requires_grad_()
        mod = DistributedSoftmaxLoss(B, impl="hip").cuda(rank)
        loss = mod(zi, zt, image_ids=img[sl].cuda(rank),
                   text_ids=txt[sl].cuda(rank), duplicates=duplicates)
        loss.backward()
        torch.cuda.synchronize()
        ret[rank] = (loss.detach().cpu(), zi.grad.cpu(), zt.grad.cpu(),
                     mod.t_prime.grad.cpu())
    finally:
        dist.destroy_process_group()


@needs2
@pytest.mark.parametrize("duplicates", ["positive", "ignore"])
def test_rccl_averaged_grads_equal_single_gpu(duplicates):
    from distributed_sigmoid_loss_amd import DistributedSoftmaxLoss
    world = 2
    zi_all, zt_all, img, txt = _global_batch(world)
    zi = zi_all.cuda().requires_grad_()
    zt = zt_all.cuda().requires_grad_()
    ref_mod = DistributedSoftmaxLoss(world * B, impl="hip").cuda()
    ref_loss = ref_mod(zi, zt, image_ids=img.cuda(), text_ids=txt.cuda(),
                       duplicates=duplicates)
    ref_loss.backward()

    manager = mp.Manager()
    ret = manager.dict()
    mp.spawn(_rank_worker, args=(world, free_port(), duplicates, ret),
             nprocs=world, join=True)

    loss_sum, dtp_sum = 0.0, 0.0
    for rank in range(world):
        loss, dzi, dzt, dtp = ret[rank]
        sl = slice(rank * B, (rank + 1) * B)
        # DDP averaging: a rank's raw gradient over W
        torch.testing.assert_close(dzi.float() / world,
                                   zi.grad[sl].float().cpu(), **EMB_TOL)
        torch.testing.assert_close(dzt.float() / world,
                                   zt.grad[sl].float().cpu(), **EMB_TOL)
        loss_sum, dtp_sum = loss_sum + loss, dtp_sum + dtp
    torch.testing.assert_close(loss_sum / world, ref_loss.detach().cpu(),
                               rtol=1e-4, atol=0)
    torch.testing.assert_close(dtp_sum / world, ref_mod.t_prime.grad.cpu(),
                               **SCALAR_TOL)
    assert math.isfinite(float(loss_sum))
