#!/usr/bin/env python3
"""End-to-end distributed SigLIP contrastive training example.

Trains a two-tower model with the fused MI355X loss kernels over RCCL/xGMI.
Synthetic data (no network access in this environment); swap `synthetic_batch`
for a real image/text dataloader in production.

Single GPU:
    python examples/train_siglip.py --steps 50

8 GPUs (one process per GPU over RCCL):
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
        --master-addr 127.0.0.1 examples/train_siglip.py --steps 50

CPU smoke (gloo):
    python examples/train_siglip.py --device cpu --batch-per-gpu 8 --dim 64

``--loss softmax`` trains against the softmax (CLIP / InfoNCE) baseline loss
instead of the sigmoid one.

``--eval-every N`` prints the retrieval metrics of the current batch every N
steps (image→text and text→image recall@1/5 and the median rank, over the
global batch): the loss alone barely moves with retrieval quality at the
SigLIP initialisation.

``--hard-negatives K`` (with ``--eval-every``) adds one line per eval: the
mean margin between the positive score and the mean of the K hardest negative
scores, image→text and text→image, over the global batch.

``--captions-per-image C`` trains on multi-caption batches: the batch holds
``batch-per-gpu / C`` images, each repeated ``C`` times against ``C`` distinct
texts, and the sample ids (global sample index // C) tell the loss that all
``C`` pairs of an image are positives.  Needs ``--loss sigmoid --strategy
all_gather --quant bf16``.
"""

from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist

from distributed_sigmoid_loss_amd import (
    DistributedSigmoidLoss,
    DistributedSoftmaxLoss,
    distributed_retrieval_ranks,
    distributed_retrieval_topk,
    positive_scores,
    recall_at_k,
)
from distributed_sigmoid_loss_amd.models import TwoTowerModel
from distributed_sigmoid_loss_amd.parallel import average_gradients
from distributed_sigmoid_loss_amd.utils import init_from_env, set_seed
from distributed_sigmoid_loss_amd.utils.profiling import PhaseTimer


def synthetic_batch(b, dim, device, dtype, seed):
    # Device-side generation — a host dataloader would overlap H2D copies
    # with compute via a prefetching pipeline; synthetic data skips that.
    # Seeded per (step, rank) so each rank's shard is distinct — with a
    # shared generator every rank would draw identical batches and the
    # cross-rank negatives would duplicate the positives.
    g = torch.Generator(device=device).manual_seed(seed)
    img = torch.randn(b, dim, device=device, dtype=dtype, generator=g)
    txt = torch.randn(b, dim, device=device, dtype=dtype, generator=g)
    return img, txt


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--batch-per-gpu", type=int, default=4096)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--strategy", choices=["ring", "all_gather"],
                   default="ring")
    p.add_argument("--quant", choices=["bf16", "fp8", "mixed"], default="bf16")
    p.add_argument("--loss", choices=["sigmoid", "softmax"],
                   default="sigmoid",
                   help="softmax: the CLIP / InfoNCE baseline (bf16 only; "
                        "--strategy and --quant do not apply)")
    p.add_argument("--device", default=None)
    p.add_argument("--log-every", type=int, default=10)
    p.add_argument("--eval-every", type=int, default=0,
                   help="print retrieval recall of the current batch every N "
                        "steps (0 = off)")
    p.add_argument("--hard-negatives", type=int, default=0,
                   help="with --eval-every: also print the mean margin of "
                        "the positive over the K hardest negatives (0 = off)")
    p.add_argument("--captions-per-image", type=int, default=1,
                   help="C texts per image: b/C images repeated C times, "
                        "positives from sample ids (needs --loss sigmoid "
                        "--strategy all_gather --quant bf16 and "
                        "batch-per-gpu %% C == 0)")
    args = p.parse_args()
    cpi = args.captions_per_image
    if cpi < 1:
        p.error("--captions-per-image must be at least 1")
    if cpi > 1:
        if (args.loss != "sigmoid" or args.strategy != "all_gather"
                or args.quant != "bf16"):
            p.error("--captions-per-image needs --loss sigmoid --strategy "
                    "all_gather --quant bf16")
        if args.batch_per_gpu % cpi != 0:
            p.error("--batch-per-gpu must be a multiple of "
                    "--captions-per-image")

    rank, local_rank, world = init_from_env()
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    dtype = torch.bfloat16 if device == "cuda" else torch.float32
    set_seed(1234)  # identical tower init on every rank

    model = TwoTowerModel(args.dim, args.dim).to(device=device, dtype=dtype)
    if args.loss == "softmax":
        loss_mod = DistributedSoftmaxLoss(args.batch_per_gpu).to(device)
    else:
        loss_mod = DistributedSigmoidLoss(
            args.batch_per_gpu, strategy=args.strategy,
            quant=args.quant if device == "cuda" else "bf16").to(device)
    # Loss params (t_prime, bias) must reach the optimizer too
    # (reference README.md:20).
    opt = torch.optim.AdamW(
        list(model.parameters()) + list(loss_mod.parameters()), lr=args.lr)

    timer = PhaseTimer(enabled=True, use_cuda=(device == "cuda"))
    t0 = time.perf_counter()
    for step in range(args.steps):
        img, txt = synthetic_batch(args.batch_per_gpu, args.dim, device,
                                   dtype, step * world + rank)
        ids = None
        if cpi > 1:
            # b/C images, each against C distinct texts; an id is the global
            # sample index // C, so the C pairs of an image share it.
            img = img[:args.batch_per_gpu // cpi].repeat_interleave(cpi, 0)
            ids = (rank * args.batch_per_gpu + torch.arange(
                args.batch_per_gpu, device=device)) // cpi
        opt.zero_grad(set_to_none=True)
        with timer.phase("encode"):
            zi, zt = model(img, txt)
        with timer.phase("loss"):
            loss = (loss_mod(zi, zt) if ids is None else
                    loss_mod(zi, zt, image_ids=ids, text_ids=ids))
        with timer.phase("backward"):
            loss.backward()
        with timer.phase("grad_avg"):
            if world > 1:
                average_gradients(model)
                average_gradients(loss_mod)
        with timer.phase("opt"):
            opt.step()
        timer.step_end()

        if rank == 0 and (step + 1) % args.log_every == 0:
            phases = "  ".join(f"{k}={v:.2f}ms"
                               for k, v in timer.summary().items())
            print(f"step {step + 1:4d}  loss={float(loss.detach()):.4f}  "
                  f"t={float(loss_mod.t_prime.detach().exp()):.3f}  "
                  + (f"bias={float(loss_mod.bias.detach()):.3f}  "
                     if hasattr(loss_mod, "bias") else "")
                  + phases, flush=True)
            timer.rows.clear()

        if args.eval_every > 0 and (step + 1) % args.eval_every == 0:
            # Collective: every rank takes part, rank 0 reports its shard's
            # ranks against the global batch.
            ranks = distributed_retrieval_ranks(zi.detach(), zt.detach())
            if rank == 0:
                r_i2t, r_t2i = recall_at_k(ranks.i2t, (1, 5)), \
                    recall_at_k(ranks.t2i, (1, 5))
                print(f"eval {step + 1:4d}  "
                      f"i2t R@1={r_i2t['R@1']:.4f} R@5={r_i2t['R@5']:.4f} "
                      f"median={int(ranks.i2t.median())}  "
                      f"t2i R@1={r_t2i['R@1']:.4f} R@5={r_t2i['R@5']:.4f} "
                      f"median={int(ranks.t2i.median())}", flush=True)
            if args.hard_negatives > 0:
                # Collective as well.  Every rank's margins cover its shard
                # against the global batch; their mean is averaged over ranks.
                neg_i2t, neg_t2i = distributed_retrieval_topk(
                    zi.detach(), zt.detach(), args.hard_negatives,
                    exclude_positive=True)
                pos = positive_scores(zi.detach(), zt.detach(), 0).float()
                margins = torch.stack([
                    (pos - neg.scores.float().mean(1)).mean()
                    for neg in (neg_i2t, neg_t2i)])
                if world > 1:
                    dist.all_reduce(margins)
                    margins /= world
                if rank == 0:
                    print(f"hardneg {step + 1:4d}  k={args.hard_negatives}  "
                          f"i2t margin={float(margins[0]):.4f}  "
                          f"t2i margin={float(margins[1]):.4f}", flush=True)

    if device == "cuda":
        torch.cuda.synchronize()
    if rank == 0:
        total = time.perf_counter() - t0
        pairs = args.batch_per_gpu * world * args.steps
        print(f"done: {args.steps} steps, {pairs / total:,.0f} pairs/s "
              f"aggregate over {world} rank(s)")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
