"""Distributed retrieval ranks on RCCL: every rank's ``i2t`` / ``t2i`` must
equal its slice of the single-GPU ``retrieval_ranks`` on the global batch.

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

B, D = 200, 72    # per-rank batch (ragged against the 128-wide tile), emb dim


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
        from distributed_sigmoid_loss_amd import distributed_retrieval_ranks
        zi_all, zt_all = _global_batch(world)
        got = distributed_retrieval_ranks(
            zi_all[rank * B:(rank + 1) * B].cuda(rank),
            zt_all[rank * B:(rank + 1) * B].cuda(rank), impl="hip")
        torch.cuda.synchronize()
        ret[rank] = (got.i2t.cpu(), got.t2i.cpu())
    finally:
        dist.destroy_process_group()


@needs2
def test_rccl_ranks_equal_single_gpu_slices():
    from distributed_sigmoid_loss_amd import retrieval_ranks
    world = 2
    zi_all, zt_all = _global_batch(world)
    ref = retrieval_ranks(zi_all.cuda(), zt_all.cuda(), 0, impl="hip")
    ref_i2t, ref_t2i = ref.i2t.cpu(), ref.t2i.cpu()
    manager = mp.Manager()
    ret = manager.dict()
    mp.spawn(_rank_worker, args=(world, free_port(), ret), nprocs=world,
             join=True)
    for rank in range(world):
        i2t, t2i = ret[rank]
        assert torch.equal(i2t, ref_i2t[rank * B:(rank + 1) * B])
        assert torch.equal(t2i, ref_t2i[rank * B:(rank + 1) * B])
