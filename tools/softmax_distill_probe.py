"""Time the two softmax distillation kernels against the one-grid softmax
passes on the same student pair (one K loop: the floor of a kernel that runs
two) and the loss against the chunked torch composite it replaces, in one
process.

    python tools/softmax_distill_probe.py [--batch 32768 8192] [--dim 768]
                                          [--teacher-dim 768] [--alpha 0.5]
                                          [--iters 30] [--stock-iters 5]
                                          [--only all|stats|g]
                                          [--teacher-quant bf16|mxfp8]

``--teacher-quant mxfp8`` times the MXFP8-teacher ops against the
bf16-teacher ops instead (``probe_mx``).  At each (B, B, d / d_T) bf16 shape: L2-normalised student and teacher rows,
``t = t_T = 10``, ``diag_offset = 0``.  Every timing is the median (with min
and max) of warm calls timed one by one between device events; the two sides
of a pair are timed alternately, call by call, so that drift of the clocks
hits both alike:

- ``stats`` against ``lse``: ``ops.pair_distill_stats`` against
  ``ops.pair_lse``;
- ``g`` against ``softmax_g``: ``ops.softmax_distill_g`` against
  ``ops.softmax_g``, both writing the bf16 g slab into the same buffer, from
  the statistics of the pass above and unit upstream weights;
- ``fused`` against ``stock``: ``softmax_distillation_loss(impl="hip")``
  forward + backward against ``impl="torch", col_chunk=4096``,
  ``--stock-iters`` calls of each, and the peak memory of each (growth of
  ``torch.cuda.max_memory_allocated`` over one call); ``fused_banded`` is the
  fused path under the composite's own ``col_chunk=4096``.

The TFLOP/s figures count both grids: ``2·B²·(d + d_T)`` over the kernel's
time.  ``--only stats|g`` times one kernel alone (for a kernel-trace run).
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
from distributed_sigmoid_loss_amd import ops, softmax_distillation_loss  # noqa: E402


def probe(b, d, d_t, alpha, iters, stock_iters, only):
    gen = torch.Generator(device="cuda").manual_seed(0)

    def rows(dim):
        return F.normalize(torch.randn(b, dim, device="cuda", generator=gen),
                           dim=-1).bfloat16()

    zi, zt, ti, tt = rows(d), rows(d), rows(d_t), rows(d_t)
    tp = torch.tensor(math.log(10.0), device="cuda")
    pairs = (zi, zt, tp, ti, tt, tp.clone())
    out = {"probe": "softmax_distill", "batch": b, "dim": d,
           "teacher_dim": d_t, "alpha": alpha, "iters": iters,
           "device": torch.cuda.get_device_name(0)}
    flop = 2.0 * b * b * (d + d_t)

    def put(name, stats):
        out.update({f"{name}_ms": stats[0], f"{name}_min_ms": stats[1],
                    f"{name}_max_ms": stats[2]})

    st = ops.pair_distill_stats(*pairs)
    tw = torch.full((b,), alpha, device="cuda")
    hw = torch.full((b,), 1.0 - alpha, device="cuda")
    row = (st.row_lse_s, st.row_lse_t, tw + hw, tw, hw)
    col = (st.col_lse_s, st.col_lse_t, tw + hw, tw, hw)
    g_buf = torch.empty((b, b), device="cuda", dtype=torch.bfloat16)

    def stats():
        ops.pair_distill_stats(*pairs)

    def g():
        ops.softmax_distill_g(*pairs, row, col, 0, g=g_buf)

    if only != "all":
        put(only, median_ms(stats if only == "stats" else g, iters))
        return out
    floors = (("stats", stats, "lse", lambda: ops.pair_lse(zi, zt, tp)),
              ("g", g, "softmax_g", lambda: ops.softmax_g(
                  zi, zt, tp, row[0], row[2], col[0], col[2], 0, g=g_buf)))
    for name, fn, floor_name, floor_fn in floors:
        ours, floor = alternate_ms(fn, floor_fn, iters)
        put(name, ours)
        put(floor_name, floor)
        out[f"{name}_tflops"] = round(flop / out[f"{name}_ms"] * 1e-9, 1)
        out[f"{name}_over_{floor_name}"] = round(
            out[f"{name}_ms"] / out[f"{floor_name}_ms"], 3)
    del g_buf

    leaves = [x.clone().requires_grad_() for x in (zi, zt, tp)]

    def step(**kw):
        def run():
            for x in leaves:
                x.grad = None
            softmax_distillation_loss(*leaves, ti, tt, tp, alpha, 0,
                                      **kw).backward()
        return run

    fused, stock = step(impl="hip"), step(impl="torch", col_chunk=4096)
    f_stats, s_stats = alternate_ms(fused, stock, stock_iters, warmup=2)
    put("fused", f_stats)
    put("stock", s_stats)
    out["stock_over_fused"] = round(out["stock_ms"] / out["fused_ms"], 3)
    out["fused_peak_mib"] = peak_mib(fused)
    out["stock_peak_mib"] = peak_mib(stock)
    # The fused path under the composite's own column chunk: g in bands.
    banded = step(impl="hip", col_chunk=4096)
    put("fused_banded", median_ms(banded, stock_iters))
    out["fused_banded_peak_mib"] = peak_mib(banded)
    return out


def probe_mx(b, d, d_t, alpha, iters):
    """``--teacher-quant mxfp8``: the two MX-teacher ops against the
    bf16-teacher ops on the same teacher, alternated call by call."""
    gen = torch.Generator(device="cuda").manual_seed(0)

    def rows(dim):
        return F.normalize(torch.randn(b, dim, device="cuda", generator=gen),
                           dim=-1).bfloat16()

    zi, zt, ti, tt = rows(d), rows(d), rows(d_t), rows(d_t)
    tp = torch.tensor(math.log(10.0), device="cuda")
    mx = (*ops.quantize_mx(ti), *ops.quantize_mx(tt))
    out = {"probe": "softmax_distill_mx_teacher", "batch": b, "dim": d,
           "teacher_dim": d_t, "alpha": alpha, "iters": iters,
           "device": torch.cuda.get_device_name(0)}
    st = ops.pair_distill_stats(zi, zt, tp, ti, tt, tp)
    tw = torch.full((b,), alpha, device="cuda")
    hw = torch.full((b,), 1.0 - alpha, device="cuda")
    row = (st.row_lse_s, st.row_lse_t, tw + hw, tw, hw)
    col = (st.col_lse_s, st.col_lse_t, tw + hw, tw, hw)
    g_buf = torch.empty((b, b), device="cuda", dtype=torch.bfloat16)
    pairs = (
        ("stats", lambda: ops.pair_distill_stats_mx(zi, zt, tp, *mx, tp),
         lambda: ops.pair_distill_stats(zi, zt, tp, ti, tt, tp)),
        ("g", lambda: ops.softmax_distill_g_mx(zi, zt, tp, *mx, tp, row, col,
                                               0, g=g_buf),
         lambda: ops.softmax_distill_g(zi, zt, tp, ti, tt, tp, row, col, 0,
                                       g=g_buf)))
    for name, mx_fn, bf_fn in pairs:
        for key, stats in zip((f"mx_{name}", f"bf16_{name}"),
                              alternate_ms(mx_fn, bf_fn, iters)):
            out.update({f"{key}_ms": stats[0], f"{key}_min_ms": stats[1],
                        f"{key}_max_ms": stats[2]})
        out[f"mx_over_bf16_{name}"] = round(
            out[f"mx_{name}_ms"] / out[f"bf16_{name}_ms"], 3)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, nargs="+", default=[32768, 8192])
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--teacher-dim", type=int, default=768)
    p.add_argument("--alpha", type=float, default=0.5)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--stock-iters", type=int, default=5)
    p.add_argument("--only", choices=["all", "stats", "g"], default="all")
    p.add_argument("--teacher-quant", choices=["bf16", "mxfp8"],
                   default="bf16")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_distill_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    for b in args.batch:
        if args.teacher_quant == "mxfp8":
            res = probe_mx(b, args.dim, args.teacher_dim, args.alpha,
                           args.iters)
        else:
            res = probe(b, args.dim, args.teacher_dim, args.alpha,
                        args.iters, args.stock_iters, args.only)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
