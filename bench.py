#!/usr/bin/env python3
"""Flagship benchmark: distributed SigLIP contrastive training step.

Measures the BASELINE.json north-star metric — image-text pairs/sec,
forward+backward(+grad-average+optimizer), global batch B=32768, emb dim 768,
bf16, strong scaling over 1/2/4/8 MI355X GPUs (per-rank batch = B/N; the
pair-grid work B² is fixed as N grows).

One step = encode both towers → L2-normalize → DistributedSigmoidLoss
(fused CDNA4 HIP kernels; ring or all-gather comm over RCCL/xGMI) → backward
(tower grads via torch DDP's bucketed all-reduce overlapped with backward at
N>1; loss params averaged manually) → SGD step.  Data is synthetic random
features; weights are random-init (no datasets/checkpoints offline).

Launch (driver contract):
    python bench.py --gpus N --steps K --warmup W
    # N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
    #        --master-addr 127.0.0.1 bench.py --gpus N ...
Rank 0 prints exactly one JSON line with the aggregate metric.

A plain run does only what that line needs: set up, warm up, time the K
steps, print.  ``--dump-outputs DIR`` additionally writes what the last timed
step computed as ``DIR/<name>.npy`` (same arguments → same seeded inputs, so
two builds can be compared output for output).  ``--full`` is where any
measurement beyond the headline figure belongs; none exists at present.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

from distributed_sigmoid_loss_amd import DistributedSigmoidLoss
from distributed_sigmoid_loss_amd.models import TwoTowerModel
from distributed_sigmoid_loss_amd.parallel import average_gradients
from distributed_sigmoid_loss_amd.utils import init_from_env, set_seed
from distributed_sigmoid_loss_amd.utils.profiling import PhaseTimer, HopStats


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1,
                   help="world size (informational; actual size from env)")
    p.add_argument("--steps", type=int, default=20,
                   help="number of timed steps (>= 1)")
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--global-batch", type=int, default=32768)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--strategy", choices=["ring", "all_gather"],
                   default="ring")
    p.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    p.add_argument("--quant", choices=["bf16", "fp8", "mixed"],
                   default="bf16",
                   help="bf16 | fp8 (MX-scaled e4m3 logits + fp8 grad GEMMs)"
                        " | mixed (bf16 logits, fp8 grad GEMMs)")
    p.add_argument("--impl", choices=["auto", "hip", "torch"], default="auto",
                   help="'torch' = stock-PyTorch floor (materialized logits)")
    p.add_argument("--device", choices=["cuda", "cpu"], default=None)
    p.add_argument("--col-chunk", type=int, default=None,
                   help="column slab size for chunked negatives")
    p.add_argument("--csv", default=None,
                   help="write per-step phase timings (ms) to this CSV")
    p.add_argument("--graph", action="store_true",
                   help="capture the steady-state step in a hipGraph and "
                        "replay it (single-GPU; falls back to eager if "
                        "capture fails)")
    p.add_argument("--ddp", dest="ddp", action="store_true", default=True,
                   help="wrap the towers in torch DDP (bucketed RCCL "
                        "all-reduce overlapped with backward) — the "
                        "default at N>1")
    p.add_argument("--no-ddp", dest="ddp", action="store_false",
                   help="manual post-backward grad averaging instead "
                        "(the reference harness's scheme)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last step's "
                        "outputs (loss, embeddings, gradients, updated "
                        "parameters) as DIR/<name>.npy, float32, at most "
                        "64 MB in all (large arrays: a fixed seeded row "
                        "sample)")
    p.add_argument("--full", action="store_true",
                   help="also run every measurement beyond the headline "
                        "figure (none at present: a plain run already "
                        "does only what the result line needs)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")
    return args


# --dump-outputs budget: 64 MB in all, shared evenly by the six arrays that
# can be large (two embeddings, two tower weights, their two gradients); the
# scalar loss parameters are a few bytes.
_DUMP_MAX_ELEMS = (60 * 2 ** 20) // (6 * 4)


def _dump_array(t: torch.Tensor) -> np.ndarray:
    """float32 host copy; arrays over the per-array budget keep a fixed,
    seeded, sorted sample of their rows."""
    t = t.detach()
    if t.dim() >= 2 and t.numel() > _DUMP_MAX_ELEMS:
        row = t[0].numel()
        k = max(1, _DUMP_MAX_ELEMS // row)
        idx = np.sort(np.random.RandomState(0).choice(
            t.shape[0], size=k, replace=False))
        t = t[torch.as_tensor(idx, device=t.device)]
    return t.float().cpu().numpy()


def dump_outputs(path, last, model, loss_mod):
    """Write what the last timed step handed its caller: the loss, both
    embedding batches, every gradient and every updated parameter."""
    os.makedirs(path, exist_ok=True)
    arrays = {"loss": last["loss"], "image_emb": last["image_emb"],
              "text_emb": last["text_emb"]}
    named = [("model." + (n[7:] if n.startswith("module.") else n), p)
             for n, p in model.named_parameters()]
    named += [("loss." + n, p) for n, p in loss_mod.named_parameters()]
    for n, p in named:
        arrays["param." + n] = p
        if p.grad is not None:
            arrays["grad." + n] = p.grad
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"), _dump_array(t))


def main():
    args = parse_args()
    rank, local_rank, world = init_from_env()
    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    if device == "cpu" and args.dtype == "bf16":
        args.dtype = "fp32"  # CPU plumbing config runs fp32
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32

    if args.global_batch % world:
        raise SystemExit(f"global batch {args.global_batch} not divisible by "
                         f"world size {world}")
    b = args.global_batch // world
    set_seed(1234 + rank)

    model = TwoTowerModel(args.dim, args.dim).to(device=device, dtype=dtype)
    loss_mod = DistributedSigmoidLoss(b, strategy=args.strategy,
                                      col_chunk=args.col_chunk,
                                      quant=args.quant,
                                      impl=args.impl).to(device)
    if args.ddp and world > 1:
        model = torch.nn.parallel.DistributedDataParallel(
            model, device_ids=[local_rank] if device == "cuda" else None)
        # loss params still averaged manually (2 scalars)
    params = list(model.parameters()) + list(loss_mod.parameters())
    opt = torch.optim.SGD(params, lr=1e-4)
    timer = PhaseTimer(enabled=args.csv is not None,
                       use_cuda=(device == "cuda"))
    if args.csv and device == "cuda":
        HopStats.set_enabled(True)   # per-hop ring comm/compute breakdown

    img_feats = torch.randn(b, args.dim, device=device, dtype=dtype)
    txt_feats = torch.randn(b, args.dim, device=device, dtype=dtype)

    use_graph = (args.graph and device == "cuda" and world == 1
                 and args.csv is None)
    last = {}   # the latest step's outputs, kept only for --dump-outputs

    def step():
        # Graph mode needs stable grad buffers across replays.
        opt.zero_grad(set_to_none=not use_graph)
        with timer.phase("encode"):
            zi, zt = model(img_feats, txt_feats)
        with timer.phase("loss_fwd"):
            loss = loss_mod(zi, zt)
        if args.dump_outputs:
            # References only (no copy, no sync); under --graph these are
            # the capture's static tensors, refreshed by every replay.
            last.update(loss=loss, image_emb=zi, text_emb=zt)
        with timer.phase("backward"):
            loss.backward()
        with timer.phase("grad_avg"):
            if world > 1:
                if not args.ddp:
                    average_gradients(model)
                average_gradients(loss_mod)
        with timer.phase("optimizer"):
            opt.step()
        timer.step_end()
        return loss

    def sync():
        if device == "cuda":
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    run_step = step
    if use_graph:
        try:
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                step()
            run_step = graph.replay
        except Exception as e:  # pragma: no cover - capture support varies
            print(f"# graph capture failed, falling back to eager: {e}",
                  file=sys.stderr)
            run_step = step
        run_step()   # one replay as extra warmup
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run_step()
    sync()
    elapsed = time.perf_counter() - t0

    # Max over ranks so stragglers count.
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        if dist.get_backend() != "gloo":
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.csv and rank == 0:
        timer.write_csv(args.csv)
        hops = HopStats.summary()
        if hops:
            print("# hop_stats_ms " + json.dumps(
                {k: round(v, 4) for k, v in hops.items()}), file=sys.stderr)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last, model, loss_mod)

    ms_per_step = elapsed / args.steps * 1000.0
    pairs_per_sec = args.global_batch / (elapsed / args.steps)

    if rank == 0:
        print(json.dumps({
            "metric": "image-text pairs/sec fwd+bwd",
            "value": pairs_per_sec,
            "unit": "pairs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": args.dtype if args.quant == "bf16" else args.quant,
            "data": "synthetic",
            "config": {
                "model": "two-tower-linear-siglip",
                "global_batch": args.global_batch,
                "emb_dim": args.dim,
                "seq_len": None,
                "parallelism": f"dp{world}-{args.strategy}",
                "impl": args.impl,
                "graph": bool(use_graph),
                "ddp_towers": bool(args.ddp and world > 1),
            },
        }), flush=True)

    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
