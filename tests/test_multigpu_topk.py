"""Distributed top-k retrieval on RCCL: every rank's ``i2t`` / ``t2i`` lists
must equal its slice of the single-GPU ``retrieval_topk`` on the global batch,
with and without the positive.

GPU-marked and skipped below 2 visible GPUs.  Inputs are integer-valued, so
the scores are exact in fp32 and the comparison is ``torch.equal``."""

from __future__ import annotations

import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

N_GPUS = torch.cuda.device_count()
needs2 = pytest.mark.skipif(N_GPUS < 2, reason="needs >=2 GPUs")

B, D, K = 200, 72, 8   # per-rank batch (ragged against the 128-wide tile)


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _global_batch(world: int):
    g = torch.Generator().manual_seed(5)
    zi = torch.randint(-3, 4, (world * B, D), generator=g).bfloat16()
    zt = torch.randint(-3, 4, (world * B, D), generator=g).bfloat16()
    return zi, zt


def _rank_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    try:
        from distributed_sigmoid_loss_amd import distributed_retrieval_topk
        zi_all, zt_all = _global_batch(world)
        out = []
        for exclude in (False, True):
            i2t, t2i = distributed_retrieval_topk(
                zi_all[rank * B:(rank + 1) * B].cuda(rank),
                zt_all[rank * B:(rank + 1) * B].cuda(rank), K,
                exclude_positive=exclude, impl="hip")
            torch.cuda.synchronize()
            out.append(tuple(t.cpu() for t in (*i2t, *t2i)))
        ret[rank] = out
    finally:
        dist.destroy_process_group()


@needs2
def test_rccl_topk_equals_single_gpu_slices():
    from distributed_sigmoid_loss_amd import retrieval_topk
    world = 2
    zi_all, zt_all = _global_batch(world)
    manager = mp.Manager()
    ret = manager.dict()
    mp.spawn(_rank_worker, args=(world, free_port(), ret), nprocs=world,
             join=True)
    for e, exclude in enumerate((False, True)):
        ref = retrieval_topk(zi_all.cuda(), zt_all.cuda(), K,
                             0 if exclude else None, impl="hip")
        ref = [t.cpu() for t in (*ref[0], *ref[1])]
        for rank in range(world):
            sl = slice(rank * B, (rank + 1) * B)
            for got, want in zip(ret[rank][e], ref):
                assert torch.equal(got, want[sl])
