"""Time the sample-ID top-k kernel against the positional top-k kernel on the
same embeddings and against the dense torch composite, in one process.

    python tools/topk_id_probe.py [--batch 32768] [--dim 768] [--iters 30]
                                  [--captions 5]

At one (B, B, d) bf16 shape, L2-normalised, with ``--captions`` consecutive
texts per image id (*grouped*: equal ids lie in the tiles along the diagonal,
every other tile takes the kernel's range shortcut) and with the same ids
after a permutation of the texts (*shuffled*: every tile compares ids), in
``"positive"`` mode, for k = 1 and k = 16, each figure the median (min–max) of
``--iters`` warm calls timed one by one between device events, the variants
alternating within a round:

- ``positional_k*``: ``ops.pair_topk(diag_offset=0)`` — the yardstick;
- ``ids_*_k*``:      ``ops.pair_topk_ids``;
- ``composite_*_k*``: the torch code a user writes without the kernel — bf16
                     ``zimg[r0:r1] @ ztxt.T`` in 4096-row chunks, the id
                     classes by broadcasting, ``masked_fill``, ``torch.topk``.

An extension built with ``-DTOPK_IDS_SHORTCUT=0`` times the kernel without
its tile-uniform shortcut; the yardstick in the same rounds makes two runs
comparable.  Prints one JSON line.
"""

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_sigmoid_loss_amd import ops  # noqa: E402


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


def composite(zi, zt, img_ids, txt_ids, k, chunk=4096):
    """Dense ``"positive"``-mode top-k of the negatives over row chunks."""
    b = zi.shape[0]
    ok_c = txt_ids >= 0
    scores = torch.empty((b, k), device=zi.device)
    cols = torch.empty((b, k), device=zi.device, dtype=torch.long)
    for r0 in range(0, b, chunk):
        r1 = min(b, r0 + chunk)
        s = (zi[r0:r1] @ zt.T).float()
        neg = ((img_ids[r0:r1, None] != txt_ids[None, :])
               & (img_ids[r0:r1] >= 0)[:, None] & ok_c[None, :])
        scores[r0:r1], cols[r0:r1] = torch.topk(
            s.masked_fill_(~neg, -math.inf), k, dim=1)
    return scores, cols


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32768)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--captions", type=int, default=5)
    p.add_argument("--only", default=None,
                   help="time one variant alone (for a kernel-trace run)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_id_probe needs a GPU")
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

    fns = {}
    for k in (1, 16):
        fns[f"positional_k{k}"] = lambda k=k: ops.pair_topk(zi, zt, k, 0)
        for name, txt_ids in layouts.items():
            fns[f"ids_{name}_k{k}"] = (
                lambda k=k, t=txt_ids: ops.pair_topk_ids(zi, zt, k, ids, t))
            fns[f"composite_{name}_k{k}"] = (
                lambda k=k, t=txt_ids: composite(zi, zt, ids, t, k))
    if args.only is not None:
        fns = {args.only: fns[args.only]}

    out = {"probe": "topk_ids", "batch": b, "dim": d, "iters": args.iters,
           "captions": args.captions,
           "device": torch.cuda.get_device_name(0)}
    for name, ts in timed(fns, args.iters).items():
        out[f"{name}_ms"] = round(statistics.median(ts), 4)
        out[f"{name}_min_ms"] = round(min(ts), 4)
        out[f"{name}_max_ms"] = round(max(ts), 4)
    if args.only is None:
        for k in (1, 16):
            for name in layouts:
                ids_ms = out[f"ids_{name}_k{k}_ms"]
                out[f"ids_{name}_k{k}_over_positional"] = round(
                    ids_ms / out[f"positional_k{k}_ms"], 3)
                out[f"composite_over_ids_{name}_k{k}"] = round(
                    out[f"composite_{name}_k{k}_ms"] / ids_ms, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
