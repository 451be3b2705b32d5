"""Distributed top-k under sample-ID labels on RCCL: every rank's ``i2t`` /
``t2i`` lists must equal its slice of the single-GPU ``retrieval_topk_ids`` on
the global batch.

GPU-marked and skipped below 2 visible GPUs.  Inputs are integer-valued, so
the scores are exact in fp32 and the comparison is ``torch.equal``."""

from __future__ import annotations

import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from helpers import free_port

needs2 = pytest.mark.skipif(torch.cuda.device_count() < 2,
                            reason="needs >=2 GPUs")

B, D, K = 200, 72, 8   # per-rank batch (ragged against the 128-wide tile)
MODES = ("positive", "ignore")


def _global_batch(world: int):
    """5 shuffled texts and 3 images per id: positives cross the ranks."""
    g = torch.Generator().manual_seed(5)
    zi = torch.randint(-3, 4, (world * B, D), generator=g).bfloat16()
    zt = torch.randint(-3, 4, (world * B, D), generator=g).bfloat16()
    ii = torch.arange(world * B) // 3
    ti = (torch.arange(world * B) // 5)[torch.randperm(world * B, generator=g)]
    ii[1], ti[2] = -1, -1
    return zi, zt, ii, ti


def _rank_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    try:
        from distributed_sigmoid_loss_amd import distributed_retrieval_topk_ids
        sl = slice(rank * B, (rank + 1) * B)
        zi, zt, ii, ti = (t[sl].cuda(rank) for t in _global_batch(world))
        out = []
        for mode in MODES:
            i2t, t2i = distributed_retrieval_topk_ids(zi, zt, K, ii, ti, mode,
                                                      impl="hip")
            torch.cuda.synchronize()
            out.append(tuple(t.cpu() for t in (*i2t, *t2i)))
        ret[rank] = out
    finally:
        dist.destroy_process_group()


@needs2
def test_rccl_topk_ids_equals_single_gpu_slices():
    from distributed_sigmoid_loss_amd import retrieval_topk_ids
    world = 2
    zi, zt, ii, ti = (t.cuda() for t in _global_batch(world))
    manager = mp.Manager()
    ret = manager.dict()
    mp.spawn(_rank_worker, args=(world, free_port(), ret), nprocs=world,
             join=True)
    for m, mode in enumerate(MODES):
        ref = retrieval_topk_ids(zi, zt, K, ii, ti, mode, 0, impl="hip")
        ref = [t.cpu() for t in (*ref[0], *ref[1])]
        for rank in range(world):
            sl = slice(rank * B, (rank + 1) * B)
            for got, want in zip(ret[rank][m], ref):
                assert torch.equal(got, want[sl])
