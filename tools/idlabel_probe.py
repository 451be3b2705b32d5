"""Time the sample-ID sigmoid kernel against the 256×256 persistent fwd+g
kernel at the same shape and against the stock composite it replaces, in one
process.

    python tools/idlabel_probe.py [--batch 32768 8192] [--dim 768] [--iters 30]
                                  [--quant bf16|mixed|fp8|mxfp8]
                                  [--only all|loss|g|g8|loss8|pair8]

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

``--quant mixed`` is a row set of its own for the ``mixed`` policy, each pair
timed alternately in this process, with the shipped fp8 GEMM table loaded
(``ops.load_tuned_gemms()``, as the module does for ``mixed``):

- ``g8`` against ``g``: ``ops.sigmoid_ids_e4m3`` writing the e4m3 slab pair
  against the bf16 g-writing kernel;
- ``mixed`` against ``bf16``: fused forward + backward with ``quant="mixed"``
  against ``quant="bf16"``, and the peak memory of each.

``--quant fp8`` is the row set of the ``fp8`` policy, again in alternating
pairs with the GEMM table loaded; the e4m3 pair is quantised once outside the
timed calls and its scales are added to ``t'``:

- ``loss8`` against ``loss``: ``ops.sigmoid_ids_fp8(want_g=False)`` against
  the bf16 loss-only kernel;
- ``pair8`` against ``g8``: ``ops.sigmoid_ids_fp8`` writing the slab pair
  against ``ops.sigmoid_ids_e4m3``, into the same buffers;
- ``fp8`` against ``mixed``: fused forward + backward, and the peak memory.

``--quant mxfp8`` is the row set of the ``mxfp8`` policy, next to the ``fp8``
one in alternating pairs, GEMM table loaded, both quantisations made once
outside the timed kernel calls:

- ``quant_mx`` against ``quant_fp8``: ``ops.quantize_mx`` on both operands
  against ``ops.quantize_fp8_pair``;
- ``loss_mx`` against ``loss8``: ``ops.sigmoid_ids_mx(want_g=False)`` against
  ``ops.sigmoid_ids_fp8(want_g=False)``;
- ``pair_mx`` against ``pair8``: both writing the slab pair, into the same
  buffers;
- ``mxfp8`` against ``fp8``: fused forward + backward, and the peak memory.

``fused`` and ``stock`` are timed alternately, call by call, so that drift of
the clocks hits both alike.  Peak memory of each is the growth of
``torch.cuda.max_memory_allocated`` over one call.  ``--only
loss|g|g8|loss8|pair8`` times one kernel alone (for a kernel-trace run).
Prints one JSON line per shape.
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


def probe(b, d, iters, only, quant="bf16"):
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

    if quant == "mxfp8":
        return probe_mx(out, zi, zt, tp, bias, img_ids, txt_ids, iters)
    if quant == "fp8" or only in ("loss8", "pair8"):
        return probe_fp8(out, zi, zt, tp, bias, img_ids, txt_ids, iters, only)
    if quant == "mixed" or only == "g8":
        return probe_mixed(out, zi, zt, tp, bias, img_ids, txt_ids, iters,
                           only)
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


def probe_mixed(out, zi, zt, tp, bias, img_ids, txt_ids, iters, only):
    b = zi.shape[0]
    out["quant"] = "mixed"
    out["tuned_gemms"] = ops.load_tuned_gemms()

    def put(name, stats):
        out.update({f"{name}_ms": stats[0], f"{name}_min_ms": stats[1],
                    f"{name}_max_ms": stats[2]})

    g8 = torch.empty((b, b), device="cuda", dtype=torch.float8_e4m3fn)
    gt8 = torch.empty((b, b), device="cuda", dtype=torch.float8_e4m3fn)

    def run_g8():
        ops.sigmoid_ids_e4m3(zi, zt, tp, bias, img_ids, txt_ids, g=g8, gt=gt8)

    if only == "g8":
        put("g8", median_ms(run_g8, iters))
        return out
    g_buf = torch.empty((b, b), device="cuda", dtype=torch.bfloat16)
    g8_stats, g_stats = alternate_ms(run_g8, lambda: ops.sigmoid_ids(
        zi, zt, tp, bias, img_ids, txt_ids, g=g_buf), iters)
    put("g8", g8_stats)
    put("g", g_stats)
    out["g8_over_g"] = round(out["g8_ms"] / out["g_ms"], 3)
    del g8, gt8, g_buf

    leaves = [x.clone().requires_grad_() for x in (zi, zt, tp, bias)]

    def step(quant):
        def run():
            for x in leaves:
                x.grad = None
            sigmoid_contrastive_loss_ids(*leaves, img_ids, txt_ids,
                                         impl="hip", quant=quant).backward()
        return run

    m_stats, b_stats = alternate_ms(step("mixed"), step("bf16"), iters)
    put("mixed", m_stats)
    put("bf16", b_stats)
    out["bf16_over_mixed"] = round(out["bf16_ms"] / out["mixed_ms"], 3)
    out["mixed_peak_mib"] = peak_mib(step("mixed"))
    out["bf16_peak_mib"] = peak_mib(step("bf16"))
    return out


def probe_fp8(out, zi, zt, tp, bias, img_ids, txt_ids, iters, only):
    b = zi.shape[0]
    out["quant"] = "fp8"
    out["tuned_gemms"] = ops.load_tuned_gemms()
    flop = 2.0 * b * b * zi.shape[1]

    def put(name, stats):
        out.update({f"{name}_ms": stats[0], f"{name}_min_ms": stats[1],
                    f"{name}_max_ms": stats[2]})

    qc = ops.quantize_fp8_pair(zi, zt)
    tp8 = tp + qc.si.log() + qc.st.log()
    ids = (bias, img_ids, txt_ids)
    g8 = torch.empty((b, b), device="cuda", dtype=torch.float8_e4m3fn)
    gt8 = torch.empty((b, b), device="cuda", dtype=torch.float8_e4m3fn)

    def loss8():
        ops.sigmoid_ids_fp8(qc.zi_q, qc.zt_q, tp8, *ids, want_g=False)

    def pair8():
        ops.sigmoid_ids_fp8(qc.zi_q, qc.zt_q, tp8, *ids, g=g8, gt=gt8)

    if only in ("loss8", "pair8"):
        put(only, median_ms(loss8 if only == "loss8" else pair8, iters))
        return out
    l8, l16 = alternate_ms(loss8, lambda: ops.sigmoid_ids(
        zi, zt, tp, *ids, want_g=False), iters)
    put("loss8", l8)
    put("loss", l16)
    out["loss8_over_loss"] = round(out["loss8_ms"] / out["loss_ms"], 3)
    out["loss8_tflops"] = round(flop / out["loss8_ms"] * 1e-9, 1)
    p8, p16 = alternate_ms(pair8, lambda: ops.sigmoid_ids_e4m3(
        zi, zt, tp, *ids, g=g8, gt=gt8), iters)
    put("pair8", p8)
    put("g8", p16)
    out["pair8_over_g8"] = round(out["pair8_ms"] / out["g8_ms"], 3)
    del g8, gt8

    leaves = [x.clone().requires_grad_() for x in (zi, zt, tp, bias)]

    def step(quant):
        def run():
            for x in leaves:
                x.grad = None
            sigmoid_contrastive_loss_ids(*leaves, img_ids, txt_ids,
                                         impl="hip", quant=quant).backward()
        return run

    f_stats, m_stats = alternate_ms(step("fp8"), step("mixed"), iters)
    put("fp8", f_stats)
    put("mixed", m_stats)
    out["mixed_over_fp8"] = round(out["mixed_ms"] / out["fp8_ms"], 3)
    out["fp8_peak_mib"] = peak_mib(step("fp8"))
    out["mixed_peak_mib"] = peak_mib(step("mixed"))
    return out


def probe_mx(out, zi, zt, tp, bias, img_ids, txt_ids, iters):
    b = zi.shape[0]
    out["quant"] = "mxfp8"
    out["tuned_gemms"] = ops.load_tuned_gemms()
    flop = 2.0 * b * b * zi.shape[1]

    def pair(a, b_, stats_a, stats_b):
        for name, st in ((a, stats_a), (b_, stats_b)):
            out.update({f"{name}_ms": st[0], f"{name}_min_ms": st[1],
                        f"{name}_max_ms": st[2]})
        out[f"{a}_over_{b_}"] = round(out[f"{a}_ms"] / out[f"{b_}_ms"], 3)

    pair("quant_mx", "quant_fp8", *alternate_ms(
        lambda: (ops.quantize_mx(zi), ops.quantize_mx(zt)),
        lambda: ops.quantize_fp8_pair(zi, zt), iters))
    qc = ops.quantize_fp8_pair(zi, zt)
    tp8 = tp + qc.si.log() + qc.st.log()
    mx = (*ops.quantize_mx(zi), *ops.quantize_mx(zt))
    ids = (bias, img_ids, txt_ids)
    g8 = torch.empty((b, b), device="cuda", dtype=torch.float8_e4m3fn)
    gt8 = torch.empty((b, b), device="cuda", dtype=torch.float8_e4m3fn)
    pair("loss_mx", "loss8", *alternate_ms(
        lambda: ops.sigmoid_ids_mx(*mx, tp, *ids, want_g=False),
        lambda: ops.sigmoid_ids_fp8(qc.zi_q, qc.zt_q, tp8, *ids, want_g=False),
        iters))
    out["loss_mx_tflops"] = round(flop / out["loss_mx_ms"] * 1e-9, 1)
    pair("pair_mx", "pair8", *alternate_ms(
        lambda: ops.sigmoid_ids_mx(*mx, tp, *ids, g=g8, gt=gt8),
        lambda: ops.sigmoid_ids_fp8(qc.zi_q, qc.zt_q, tp8, *ids, g=g8, gt=gt8),
        iters))
    del g8, gt8

    leaves = [x.clone().requires_grad_() for x in (zi, zt, tp, bias)]

    def step(quant):
        def run():
            for x in leaves:
                x.grad = None
            sigmoid_contrastive_loss_ids(*leaves, img_ids, txt_ids,
                                         impl="hip", quant=quant).backward()
        return run

    pair("mxfp8", "fp8", *alternate_ms(step("mxfp8"), step("fp8"), iters))
    out["mxfp8_peak_mib"] = peak_mib(step("mxfp8"))
    out["fp8_peak_mib"] = peak_mib(step("fp8"))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, nargs="+", default=[32768, 8192])
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--only",
                   choices=["all", "loss", "g", "g8", "loss8", "pair8"],
                   default="all")
    p.add_argument("--quant", choices=["bf16", "mixed", "fp8", "mxfp8"],
                   default="bf16")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("idlabel_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    for b in args.batch:
        print(json.dumps(probe(b, args.dim, args.iters, args.only,
                               args.quant)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
