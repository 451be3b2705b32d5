"""Time the sample-ID sigmoid kernel against the 256×256 persistent fwd+g
kernel at the same shape and against the stock composite it replaces, in one
process.

    python tools/idlabel_probe.py [--batch 32768 8192] [--dim 768] [--iters 30]

At each (B, B, d) bf16 shape, L2-normalised inputs, ``t = 10``, ``bias =
−10``; ids uniform over ``B // 3`` values (each id appears 3 times on average)
with 1 % of each side set to ``−1``.  Every timing is the median (with min and
max) of ``--iters`` warm calls timed one by one between device events:

- ``loss``:    ``ops.sigmoid_ids(want_g=False)`` — the loss-only kernel;
- ``g``:       ``ops.sigmoid_ids`` writing the g slab;
- ``fwd_g``:   ``ops.siglip_fwd_g`` — the positional loss's 256×256 persistent
               fwd+g kernel, the reference point (not a target);
- ``fused``:   ``sigmoid_contrastive_loss_ids(impl="hip")`` forward + backward;
- ``stock``:   what a user writes without the kernel — a materialised bf16
               ``t·zi @ zt.T + bias``, labels from ``ids[:, None] ==
               ids[None, :]``, a masked ``F.logsigmoid``, ``backward()``.

``fused`` and ``stock`` are timed alternately, call by call, so that drift of
the clocks hits both alike.  Peak memory of each is the growth of
``torch.cuda.max_memory_allocated`` over one call.  ``--only loss|g`` times
one kernel alone (for a kernel-trace run).  Prints one JSON line per shape.
"""

import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_sigmoid_loss_amd import ops, sigmoid_contrastive_loss_ids  # noqa: E402


def _timed(fn):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def _stats(times):
    return (round(statistics.median(times), 4), round(min(times), 4),
            round(max(times), 4))


def median_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return _stats([_timed(fn) for _ in range(iters)])


def alternate_ms(fn_a, fn_b, iters, warmup=3):
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(iters):
        ta.append(_timed(fn_a))
        tb.append(_timed(fn_b))
    return _stats(ta), _stats(tb)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def probe(b, d, iters, only):
    gen = torch.Generator(device="cuda").manual_seed(0)
    zi = F.normalize(torch.randn(b, d, device="cuda", generator=gen),
                     dim=-1).bfloat16()
    zt = F.normalize(torch.randn(b, d, device="cuda", generator=gen),
                     dim=-1).bfloat16()
    tp = torch.tensor(math.log(10.0), device="cuda")
    bias = torch.tensor(-10.0, device="cuda")
    ids = []
    for _ in range(2):
        v = torch.randint(0, max(1, b // 3), (b,), device="cuda",
                          generator=gen)
        v[torch.rand(b, device="cuda", generator=gen) < 0.01] = -1
        ids.append(v)
    img_ids, txt_ids = ids
    out = {"probe": "idlabel", "batch": b, "dim": d, "iters": iters,
           "device": torch.cuda.get_device_name(0)}
    flop = 2.0 * b * b * d

    def put(name, stats):
        out.update({f"{name}_ms": stats[0], f"{name}_min_ms": stats[1],
                    f"{name}_max_ms": stats[2]})

    if only in ("all", "loss"):
        put("loss", median_ms(lambda: ops.sigmoid_ids(
            zi, zt, tp, bias, img_ids, txt_ids, want_g=False), iters))
        out["loss_tflops"] = round(flop / out["loss_ms"] * 1e-9, 1)
    if only in ("all", "g"):
        g_buf = torch.empty((b, b), device="cuda", dtype=torch.bfloat16)
        put("g", median_ms(lambda: ops.sigmoid_ids(
            zi, zt, tp, bias, img_ids, txt_ids, g=g_buf), iters))
        out["g_tflops"] = round(flop / out["g_ms"] * 1e-9, 1)
        if only == "all":
            put("fwd_g", median_ms(lambda: ops.siglip_fwd_g(
                zi, zt, tp, bias, 0, g_slab=g_buf), iters))
            out["g_over_fwd_g"] = round(out["g_ms"] / out["fwd_g_ms"], 3)
        del g_buf
    if only != "all":
        return out

    zi_g = zi.clone().requires_grad_()
    zt_g = zt.clone().requires_grad_()
    tp_g = tp.clone().requires_grad_()
    bias_g = bias.clone().requires_grad_()

    def clear():
        zi_g.grad = zt_g.grad = tp_g.grad = bias_g.grad = None

    def fused():
        clear()
        sigmoid_contrastive_loss_ids(zi_g, zt_g, tp_g, bias_g, img_ids,
                                     txt_ids, impl="hip").backward()

    def stock():
        clear()
        z = (tp_g.exp().to(torch.bfloat16) * zi_g @ zt_g.T
             + bias_g.to(torch.bfloat16))
        eq = img_ids[:, None] == txt_ids[None, :]
        on = (img_ids >= 0)[:, None] & (txt_ids >= 0)[None, :]
        (-(F.logsigmoid(torch.where(eq, z, -z)) * on).sum()).backward()

    f_stats, s_stats = alternate_ms(fused, stock, iters)
    put("fused", f_stats)
    put("stock", s_stats)
    out["stock_over_fused"] = round(out["stock_ms"] / out["fused_ms"], 3)
    out["fused_peak_mib"] = peak_mib(fused)
    out["stock_peak_mib"] = peak_mib(stock)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, nargs="+", default=[32768, 8192])
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--only", choices=["all", "loss", "g"], default="all")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("idlabel_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    for b in args.batch:
        print(json.dumps(probe(b, args.dim, args.iters, args.only)),
              flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
