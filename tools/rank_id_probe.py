"""Time the sample-ID rank kernels against the positional rank-count kernel
on the same embeddings and against the dense torch composite, in one process.

    python tools/rank_id_probe.py [--batch 32768] [--dim 768] [--iters 30]
                                  [--captions 5]

At one (B, B, d) bf16 shape, with ``--captions`` consecutive texts per image
id (*grouped*: the positives lie in the tiles along the diagonal) and with the
same ids after a permutation of the texts (*shuffled*: positives in most
tiles), each figure the median (min–max) of ``--iters`` warm calls timed one
by one between device events, the variants alternating within a round:

- ``positional``: ``ops.pair_rank_counts``, both sides, ``diag_offset = 0``
                  — the yardstick;
- ``counts_*``:   ``ops.pair_rank_counts_ids``, both sides, thresholds at the
                  best positives;
- ``best_*``:     ``ops.pair_best_positive_ids``, both sides (the accumulators
                  are not reset between calls: max is idempotent);
- ``ranks_*``:    ``retrieval_ranks_ids(impl="hip")``, end to end;
- ``composite_*``: the torch code a user writes without the kernels — bf16
                  ``zimg[r0:r1] @ ztxt.T`` in 4096-row chunks, the id classes
                  by broadcasting, a masked max, then the same again for the
                  masked compare-and-sum.

Prints one JSON line.
"""

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_sigmoid_loss_amd import (  # noqa: E402
    ops, positive_scores, retrieval_ranks_ids)


def timed(fns, iters, warmup=5):
    """{name: [ms, …]} for the callables of ``fns``, run round-robin."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))
    return times


def composite(zi, zt, img_ids, txt_ids, chunk=4096):
    """Dense ``"positive"``-mode ranks: two passes over row chunks."""
    b, n = zi.shape[0], zt.shape[0]
    dev = zi.device
    ok_c = txt_ids >= 0

    def chunks():
        for r0 in range(0, b, chunk):
            r1 = min(b, r0 + chunk)
            s = (zi[r0:r1] @ zt.T).float()
            live = (img_ids[r0:r1] >= 0)[:, None] & ok_c[None, :]
            eq = img_ids[r0:r1, None] == txt_ids[None, :]
            yield r0, r1, s, eq & live, ~eq & live

    rb = torch.empty(b, device=dev)
    cb = torch.full((n,), -math.inf, device=dev)
    for r0, r1, s, pos, _ in chunks():
        sp = s.masked_fill(~pos, -math.inf)
        rb[r0:r1] = sp.amax(1)
        cb = torch.maximum(cb, sp.amax(0))
    rc = torch.empty(b, device=dev, dtype=torch.int32)
    cc = torch.zeros(n, device=dev, dtype=torch.int32)
    for r0, r1, s, _, neg in chunks():
        rc[r0:r1] = ((s > rb[r0:r1, None]) & neg).sum(1, dtype=torch.int32)
        cc += ((s > cb[None, :]) & neg).sum(0, dtype=torch.int32)
    return rc, cc


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32768)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--captions", type=int, default=5)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_id_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")

    b, d = args.batch, args.dim
    g = torch.Generator(device="cuda").manual_seed(0)
    zi = torch.nn.functional.normalize(
        torch.randn(b, d, device="cuda", generator=g), dim=-1).bfloat16()
    zt = torch.nn.functional.normalize(
        torch.randn(b, d, device="cuda", generator=g), dim=-1).bfloat16()
    ids = torch.arange(b, device="cuda") // args.captions
    layouts = {"grouped": ids,
               "shuffled": ids[torch.randperm(b, device="cuda", generator=g)]}
    thr = positive_scores(zi, zt, 0)
    rc = torch.zeros(b, device="cuda", dtype=torch.int32)
    cc = torch.zeros(b, device="cuda", dtype=torch.int32)

    fns = {"positional": lambda: ops.pair_rank_counts(
        zi, zt, thr, thr, 0, row_cnt=rc, col_cnt=cc)}
    for name, txt_ids in layouts.items():
        rb, cb = ops.pair_best_positive_ids(zi, zt, ids, txt_ids)
        fns[f"best_{name}"] = (
            lambda t=txt_ids, r=rb, c=cb: ops.pair_best_positive_ids(
                zi, zt, ids, t, row_best=r, col_best=c))
        fns[f"counts_{name}"] = (
            lambda t=txt_ids, r=rb, c=cb: ops.pair_rank_counts_ids(
                zi, zt, r, c, ids, t, row_cnt=rc, col_cnt=cc))
        fns[f"ranks_{name}"] = (
            lambda t=txt_ids: retrieval_ranks_ids(zi, zt, ids, t, impl="hip"))
        fns[f"composite_{name}"] = (
            lambda t=txt_ids: composite(zi, zt, ids, t))

    out = {"probe": "rank_ids", "batch": b, "dim": d, "iters": args.iters,
           "captions": args.captions,
           "device": torch.cuda.get_device_name(0)}
    times = timed(fns, args.iters)
    for name, ts in times.items():
        out[f"{name}_ms"] = round(statistics.median(ts), 4)
        out[f"{name}_min_ms"] = round(min(ts), 4)
        out[f"{name}_max_ms"] = round(max(ts), 4)
    pos_ms = out["positional_ms"]
    for name in layouts:
        out[f"counts_{name}_over_positional"] = round(
            out[f"counts_{name}_ms"] / pos_ms, 3)
        out[f"best_{name}_over_positional"] = round(
            out[f"best_{name}_ms"] / pos_ms, 3)
        out[f"composite_over_ranks_{name}"] = round(
            out[f"composite_{name}_ms"] / out[f"ranks_{name}_ms"], 3)
        # tiles of the grid that hold a positive
        tile = torch.nn.functional.max_pool2d(
            (ids[:, None] == layouts[name][None, :])[None, None].half(),
            128, ceil_mode=True) if b <= 8192 else None
        if tile is not None:
            out[f"tiles_with_positive_{name}"] = round(
                float(tile.mean()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
