"""Time the fused softmax-loss kernels against one MFMA pass with a scalar
epilogue and against the stock composite they replace, in one process.

    python tools/softmax_probe.py [--batch 32768 8192] [--dim 768] [--iters 30]

At each (B, B, d) bf16 shape, L2-normalised inputs, ``t = 10``; every timing
is the median (with min and max) of ``--iters`` warm calls timed one by one
between device events:

- ``lse``:     ``ops.pair_lse`` — both sides;
- ``g``:       ``ops.softmax_g`` — both sides, unit weights, ``diag_offset = 0``;
- ``fused``:   ``softmax_contrastive_loss(impl="hip")`` forward + backward;
- ``fwd``:     ``ops.siglip_fwd`` — the cost of one MFMA pass over the pair
               grid with a scalar epilogue, the one-pass yardstick;
- ``stock``:   what a user writes without the kernels — a materialised bf16
               ``t·zi @ zt.T``, two ``F.cross_entropy`` calls, ``backward()``.

``fused`` and ``stock`` are timed alternately, call by call, so that drift of
the clocks hits both alike.  Peak memory of each is the growth of
``torch.cuda.max_memory_allocated`` over one call.  ``--only lse|g`` times
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

from distributed_sigmoid_loss_amd import ops, softmax_contrastive_loss  # noqa: E402


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
    out = {"probe": "softmax", "batch": b, "dim": d, "iters": iters,
           "device": torch.cuda.get_device_name(0)}
    flop = 2.0 * b * b * d

    def put(name, stats):
        out.update({f"{name}_ms": stats[0], f"{name}_min_ms": stats[1],
                    f"{name}_max_ms": stats[2]})

    row_lse, col_lse = ops.pair_lse(zi, zt, tp)
    ones = torch.ones(b, device="cuda")
    g_buf = torch.empty((b, b), device="cuda", dtype=torch.bfloat16)
    if only in ("all", "lse"):
        put("lse", median_ms(lambda: ops.pair_lse(zi, zt, tp), iters))
        out["lse_tflops"] = round(flop / out["lse_ms"] * 1e-9, 1)
    if only in ("all", "g"):
        put("g", median_ms(lambda: ops.softmax_g(
            zi, zt, tp, row_lse, ones, col_lse, ones, 0, g=g_buf), iters))
        out["g_tflops"] = round(flop / out["g_ms"] * 1e-9, 1)
    del g_buf
    if only != "all":
        return out

    bias = torch.tensor(0.0, device="cuda")
    put("fwd", median_ms(lambda: ops.siglip_fwd(zi, zt, tp, bias, 0), iters))
    out["lse_over_fwd"] = round(out["lse_ms"] / out["fwd_ms"], 3)
    out["g_over_fwd"] = round(out["g_ms"] / out["fwd_ms"], 3)

    zi_g = zi.clone().requires_grad_()
    zt_g = zt.clone().requires_grad_()
    tp_g = tp.clone().requires_grad_()
    tgt = torch.arange(b, device="cuda")

    def clear():
        zi_g.grad = zt_g.grad = tp_g.grad = None

    def fused():
        clear()
        softmax_contrastive_loss(zi_g, zt_g, tp_g, impl="hip").backward()

    def stock():
        clear()
        z = tp_g.exp().to(torch.bfloat16) * zi_g @ zt_g.T
        (F.cross_entropy(z, tgt, reduction="sum")
         + F.cross_entropy(z.T, tgt, reduction="sum")).backward()

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
    p.add_argument("--only", choices=["all", "lse", "g"], default="all")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    for b in args.batch:
        print(json.dumps(probe(b, args.dim, args.iters, args.only)),
              flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
