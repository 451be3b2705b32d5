"""Time the sample-ID softmax kernels against their positional siblings, one
MFMA pass with a scalar epilogue and the stock composite they replace, in one
process.

    python tools/softmax_id_probe.py [--batch 32768 8192] [--dim 768]
                                     [--iters 30]

At each (B, B, d) bf16 shape, L2-normalised inputs, ``t = 10``, ids uniform
over ``B // 3`` values with 1 % of each side set to −1; every timing is the
median (with min and max) of ``--iters`` warm calls timed one by one between
device events:

- ``lse_ids``: ``ops.pair_lse_ids`` — both sides, ``duplicates="positive"``;
- ``lse``:     ``ops.pair_lse`` — the positional sibling, untouched code and
               the yardstick, in the same run;
- ``g_ids``:   ``ops.softmax_g_ids`` — both sides, the weights of a unit
               upstream gradient;
- ``g``:       ``ops.softmax_g`` — its sibling, unit weights;
- ``fwd``:     ``ops.siglip_fwd`` — the cost of one MFMA pass over the pair
               grid with a scalar epilogue;
- ``fused``:   ``softmax_contrastive_loss_ids(impl="hip")`` forward +
               backward;
- ``stock``:   what a user writes without the kernels — a materialised bf16
               ``t·zi @ zt.T``, the id-equality and mask matrices, two masked
               ``logsumexp``, the mean over the positives, ``backward()``.

``lse_ids`` / ``lse``, ``g_ids`` / ``g`` and ``fused`` / ``stock`` are each
timed alternately, call by call, so that drift of the clocks hits both alike.
Peak memory is the growth of ``torch.cuda.max_memory_allocated`` over one
call.  ``--only lse_ids|g_ids`` times one kernel alone (for a kernel-trace
run).  Prints one JSON line per shape.
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

from distributed_sigmoid_loss_amd import (  # noqa: E402
    ops,
    softmax_contrastive_loss_ids,
)


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
    ids = []
    for _ in range(2):
        v = torch.randint(0, max(b // 3, 1), (b,), device="cuda",
                          generator=gen)
        v[torch.rand(b, device="cuda", generator=gen) < 0.01] = -1
        ids.append(v)
    iid, tid = ids
    out = {"probe": "softmax_ids", "batch": b, "dim": d, "iters": iters,
           "device": torch.cuda.get_device_name(0)}
    flop = 2.0 * b * b * d

    def put(name, stats):
        out.update({f"{name}_ms": stats[0], f"{name}_min_ms": stats[1],
                    f"{name}_max_ms": stats[2]})

    o = ops.pair_lse_ids(zi, zt, tp, iid, tid)
    one = torch.ones((), device="cuda")

    def weights(cnt):
        w = torch.where(cnt > 0, one, torch.zeros_like(one)).contiguous()
        return w, (w / cnt.clamp(min=1).float()).contiguous()

    row_w, row_pw = weights(o.row_cnt)
    col_w, col_pw = weights(o.col_cnt)
    g_buf = torch.empty((b, b), device="cuda", dtype=torch.bfloat16)

    def lse_ids():
        ops.pair_lse_ids(zi, zt, tp, iid, tid)

    def g_ids():
        ops.softmax_g_ids(zi, zt, tp, iid, tid, "positive", None, o.row_lse,
                          row_w, row_pw, o.col_lse, col_w, col_pw, g=g_buf)

    if only == "lse_ids":
        put("lse_ids", median_ms(lse_ids, iters))
        return out
    if only == "g_ids":
        put("g_ids", median_ms(g_ids, iters))
        return out

    row_lse, col_lse = ops.pair_lse(zi, zt, tp)
    ones = torch.ones(b, device="cuda")
    a, s = alternate_ms(lse_ids, lambda: ops.pair_lse(zi, zt, tp), iters)
    put("lse_ids", a)
    put("lse", s)
    a, s = alternate_ms(g_ids, lambda: ops.softmax_g(
        zi, zt, tp, row_lse, ones, col_lse, ones, 0, g=g_buf), iters)
    put("g_ids", a)
    put("g", s)
    del g_buf
    for name in ("lse_ids", "g_ids"):
        out[f"{name}_tflops"] = round(flop / out[f"{name}_ms"] * 1e-9, 1)
    bias = torch.tensor(0.0, device="cuda")
    put("fwd", median_ms(lambda: ops.siglip_fwd(zi, zt, tp, bias, 0), iters))
    out["lse_ids_over_lse"] = round(out["lse_ids_ms"] / out["lse_ms"], 3)
    out["g_ids_over_g"] = round(out["g_ids_ms"] / out["g_ms"], 3)
    out["lse_ids_over_fwd"] = round(out["lse_ids_ms"] / out["fwd_ms"], 3)
    out["g_ids_over_fwd"] = round(out["g_ids_ms"] / out["fwd_ms"], 3)

    zi_g = zi.clone().requires_grad_()
    zt_g = zt.clone().requires_grad_()
    tp_g = tp.clone().requires_grad_()

    def clear():
        zi_g.grad = zt_g.grad = tp_g.grad = None

    def fused():
        clear()
        softmax_contrastive_loss_ids(zi_g, zt_g, tp_g, iid, tid,
                                     impl="hip").backward()

    def stock():
        clear()
        z = tp_g.exp().to(torch.bfloat16) * zi_g @ zt_g.T
        masked = (iid < 0)[:, None] | (tid < 0)[None, :]
        pos = (iid[:, None] == tid[None, :]) & ~masked
        # the lowest finite value, not −inf: a fully masked row must not
        # send NaN through logsumexp's backward
        zm = z.masked_fill(masked, torch.finfo(z.dtype).min)
        zp = torch.where(pos, z, torch.zeros_like(z))
        total = 0.0
        for dim in (1, 0):
            cnt = pos.sum(dim)
            term = torch.logsumexp(zm, dim) - zp.sum(dim) / cnt.clamp(min=1)
            total = total + torch.where(cnt > 0, term,
                                        torch.zeros_like(term)).sum()
        total.backward()

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
    p.add_argument("--only", choices=["all", "lse_ids", "g_ids"],
                   default="all")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_id_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    for b in args.batch:
        print(json.dumps(probe(b, args.dim, args.iters, args.only)),
              flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
