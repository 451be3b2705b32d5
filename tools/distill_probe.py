"""Time the sigmoid distillation kernel against the sample-ID sigmoid kernel on
the same student pair (one K loop: the floor of a kernel that runs two) and
against the chunked torch composite it replaces, in one process.

    python tools/distill_probe.py [--batch 32768 8192] [--dim 768]
                                  [--teacher-dim 768] [--alpha 0.5]
                                  [--iters 30] [--stock-iters 5]
                                  [--only all|loss|g]
                                  [--teacher-quant bf16|mxfp8]

``--teacher-quant mxfp8`` times the MXFP8-teacher kernel against the
bf16-teacher kernel instead (``probe_mx``).  At each (B, B, d / d_T) bf16 shape: L2-normalised student and teacher rows,
``t = t_T = 10``, ``bias = bias_T = −10``, ``diag_offset = 0``.  Every timing
is the median (with min and max) of warm calls timed one by one between device
events; the two sides of a pair are timed alternately, call by call, so that
drift of the clocks hits both alike:

- ``loss`` against ``ids_loss``: ``ops.sigmoid_distill(want_g=False)`` against
  ``ops.sigmoid_ids(want_g=False)`` with ``arange`` ids;
- ``g`` against ``ids_g``: both writing the bf16 g slab, into the same buffer;
- ``fused`` against ``stock``: ``sigmoid_distillation_loss(impl="hip")``
  forward + backward against ``impl="torch", col_chunk=4096`` — fp32 logits
  and targets, ``b × 4096`` at a time, kept for autograd — ``--stock-iters``
  calls of each, and the peak memory of each (growth of
  ``torch.cuda.max_memory_allocated`` over one call).

The TFLOP/s figures count both grids: ``2·B²·(d + d_T)`` over the kernel's
time.  ``--only loss|g`` times one kernel alone (for a kernel-trace run).
Prints one JSON line per shape.
"""

import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from idlabel_probe import alternate_ms, median_ms, peak_mib  # noqa: E402
from distributed_sigmoid_loss_amd import ops, sigmoid_distillation_loss  # noqa: E402


def probe(b, d, d_t, alpha, iters, stock_iters, only):
    gen = torch.Generator(device="cuda").manual_seed(0)

    def rows(dim):
        return F.normalize(torch.randn(b, dim, device="cuda", generator=gen),
                           dim=-1).bfloat16()

    zi, zt, ti, tt = rows(d), rows(d), rows(d_t), rows(d_t)
    tp = torch.tensor(math.log(10.0), device="cuda")
    bias = torch.tensor(-10.0, device="cuda")
    teacher = (ti, tt, tp.clone(), bias.clone())
    ids = torch.arange(b, device="cuda")
    out = {"probe": "distill", "batch": b, "dim": d, "teacher_dim": d_t,
           "alpha": alpha, "iters": iters,
           "device": torch.cuda.get_device_name(0)}
    flop = 2.0 * b * b * (d + d_t)

    def put(name, stats):
        out.update({f"{name}_ms": stats[0], f"{name}_min_ms": stats[1],
                    f"{name}_max_ms": stats[2]})

    def loss():
        ops.sigmoid_distill(zi, zt, tp, bias, *teacher, alpha, 0,
                            want_g=False)

    g_buf = torch.empty((b, b), device="cuda", dtype=torch.bfloat16)

    def g():
        ops.sigmoid_distill(zi, zt, tp, bias, *teacher, alpha, 0, g=g_buf)

    if only != "all":
        put(only, median_ms(loss if only == "loss" else g, iters))
        return out
    for name, fn, want_g in (("loss", loss, False), ("g", g, True)):
        ours, floor = alternate_ms(fn, lambda: ops.sigmoid_ids(
            zi, zt, tp, bias, ids, ids, g=g_buf if want_g else None,
            want_g=want_g), iters)
        put(name, ours)
        put(f"ids_{name}", floor)
        out[f"{name}_tflops"] = round(flop / out[f"{name}_ms"] * 1e-9, 1)
        out[f"{name}_over_ids_{name}"] = round(
            out[f"{name}_ms"] / out[f"ids_{name}_ms"], 3)
    del g_buf

    leaves = [x.clone().requires_grad_() for x in (zi, zt, tp, bias)]

    def step(**kw):
        def run():
            for x in leaves:
                x.grad = None
            sigmoid_distillation_loss(*leaves, *teacher, alpha, 0,
                                      **kw).backward()
        return run

    fused, stock = step(impl="hip"), step(impl="torch", col_chunk=4096)
    f_stats, s_stats = alternate_ms(fused, stock, stock_iters, warmup=2)
    put("fused", f_stats)
    put("stock", s_stats)
    out["stock_over_fused"] = round(out["stock_ms"] / out["fused_ms"], 3)
    out["fused_peak_mib"] = peak_mib(fused)
    out["stock_peak_mib"] = peak_mib(stock)
    return out


def probe_mx(b, d, d_t, alpha, iters, stock_iters):
    """``--teacher-quant mxfp8``: the MX-teacher kernel against the
    bf16-teacher kernel on the same teacher, alternated call by call; the cost
    of ``ops.quantize_mx`` on one ``(B, d_T)`` shard; the forward + backward
    with a stored ``(q, e8)`` teacher against the bf16 one."""
    gen = torch.Generator(device="cuda").manual_seed(0)

    def rows(dim):
        return F.normalize(torch.randn(b, dim, device="cuda", generator=gen),
                           dim=-1).bfloat16()

    zi, zt, ti, tt = rows(d), rows(d), rows(d_t), rows(d_t)
    tp = torch.tensor(math.log(10.0), device="cuda")
    bias = torch.tensor(-10.0, device="cuda")
    pairs = ops.quantize_mx(ti), ops.quantize_mx(tt)
    tail = (tp.clone(), bias.clone(), alpha, 0)
    out = {"probe": "distill_mx_teacher", "batch": b, "dim": d,
           "teacher_dim": d_t, "alpha": alpha, "iters": iters,
           "device": torch.cuda.get_device_name(0)}

    def put(name, stats):
        out.update({f"{name}_ms": stats[0], f"{name}_min_ms": stats[1],
                    f"{name}_max_ms": stats[2]})

    put("quantize_mx", median_ms(lambda: ops.quantize_mx(ti), iters))
    g_buf = torch.empty((b, b), device="cuda", dtype=torch.bfloat16)
    for name, kw in (("loss", dict(want_g=False)), ("g", dict(g=g_buf))):
        mx, bf = alternate_ms(
            lambda: ops.sigmoid_distill_mx(zi, zt, tp, bias, *pairs[0],
                                           *pairs[1], *tail, **kw),
            lambda: ops.sigmoid_distill(zi, zt, tp, bias, ti, tt, *tail,
                                        **kw), iters)
        put(f"mx_{name}", mx)
        put(f"bf16_{name}", bf)
        out[f"mx_over_bf16_{name}"] = round(
            out[f"mx_{name}_ms"] / out[f"bf16_{name}_ms"], 3)
    del g_buf

    leaves = [x.clone().requires_grad_() for x in (zi, zt, tp, bias)]

    def step(ti, tt, quant):
        def run():
            for x in leaves:
                x.grad = None
            sigmoid_distillation_loss(*leaves, ti, tt, *tail, impl="hip",
                                      teacher_quant=quant).backward()
        return run

    mx, bf = alternate_ms(step(*pairs, "mxfp8"), step(ti, tt, "bf16"),
                          stock_iters, warmup=2)
    put("mx_fused", mx)
    put("bf16_fused", bf)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, nargs="+", default=[32768, 8192])
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--teacher-dim", type=int, default=768)
    p.add_argument("--alpha", type=float, default=0.5)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--stock-iters", type=int, default=5)
    p.add_argument("--only", choices=["all", "loss", "g"], default="all")
    p.add_argument("--teacher-quant", choices=["bf16", "mxfp8"],
                   default="bf16")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    for b in args.batch:
        if args.teacher_quant == "mxfp8":
            res = probe_mx(b, args.dim, args.teacher_dim, args.alpha,
                           args.iters, args.stock_iters)
        else:
            res = probe(b, args.dim, args.teacher_dim, args.alpha,
                        args.iters, args.stock_iters, args.only)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
