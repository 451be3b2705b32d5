"""Time the fused top-k kernel against one pass of the same tile structure
and against the stock composite it replaces, in one process.

    python tools/topk_probe.py [--batches 32768,8192] [--dim 768] [--iters 30]

At every (B, B, d) bf16 shape and for k = 1 and k = 16, positive excluded,
each figure the median of ``--iters`` warm calls timed one by one between
device events:

- ``topk``:      ``ops.pair_topk`` (partials kernel + merge kernel);
- ``rank``:      (a) ``ops.pair_rank_counts``, both sides — the cost of one
                 pass of this 128×128 register-staged tile structure;
- ``composite``: (b) the torch code a user writes without the kernel — bf16
                 ``zimg[r0:r1] @ ztxt.T`` in 4096-row chunks followed by
                 ``torch.topk(k)`` (no positive mask: in its favour);
- peak memory over one fused call and over one call of (b).

``--only topk`` times the kernel alone (for a kernel-trace run).  Prints one
JSON line per shape.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_sigmoid_loss_amd import ops, positive_scores  # noqa: E402


def median_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times), min(times), max(times)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def composite(zi, zt, k, chunk=4096):
    b = zi.shape[0]
    sc = torch.empty(b, k, device=zi.device, dtype=zi.dtype)
    ix = torch.empty(b, k, device=zi.device, dtype=torch.long)
    for r0 in range(0, b, chunk):
        r1 = min(b, r0 + chunk)
        sc[r0:r1], ix[r0:r1] = (zi[r0:r1] @ zt.T).topk(k, dim=1)
    return sc, ix


def probe(b, d, iters, only):
    g = torch.Generator(device="cuda").manual_seed(0)
    zi = torch.nn.functional.normalize(
        torch.randn(b, d, device="cuda", generator=g), dim=-1).bfloat16()
    zt = torch.nn.functional.normalize(
        torch.randn(b, d, device="cuda", generator=g), dim=-1).bfloat16()
    flop = 2.0 * b * b * d
    out = {"probe": "topk", "batch": b, "dim": d, "iters": iters,
           "device": torch.cuda.get_device_name(0)}
    for k in (1, 16):
        ms, lo, hi = median_ms(lambda: ops.pair_topk(zi, zt, k, 0), iters)
        out.update({f"topk{k}_ms": round(ms, 4),
                    f"topk{k}_min_ms": round(lo, 4),
                    f"topk{k}_max_ms": round(hi, 4),
                    f"topk{k}_tflops": round(flop / ms * 1e-9, 1)})
    if only == "topk":
        return out
    thr = positive_scores(zi, zt, 0)
    rc = torch.zeros(b, device="cuda", dtype=torch.int32)
    cc = torch.zeros(b, device="cuda", dtype=torch.int32)
    ms_r, lo, hi = median_ms(
        lambda: ops.pair_rank_counts(zi, zt, thr, thr, 0, row_cnt=rc,
                                     col_cnt=cc), iters)
    out.update(rank_ms=round(ms_r, 4), rank_min_ms=round(lo, 4),
               rank_max_ms=round(hi, 4))
    for k in (1, 16):
        ms_c, lo, hi = median_ms(lambda: composite(zi, zt, k), iters)
        out.update({f"composite{k}_ms": round(ms_c, 4),
                    f"composite{k}_min_ms": round(lo, 4),
                    f"composite{k}_max_ms": round(hi, 4),
                    f"topk{k}_over_rank": round(out[f"topk{k}_ms"] / ms_r, 3),
                    f"composite{k}_over_topk{k}":
                        round(ms_c / out[f"topk{k}_ms"], 3)})
    out.update(
        topk16_peak_mib=round(peak_mib(lambda: ops.pair_topk(zi, zt, 16, 0)), 1),
        composite16_peak_mib=round(peak_mib(lambda: composite(zi, zt, 16)), 1))
    # How often the composite's bf16-rounded scores give the same best match.
    k_c = ops.pair_topk(zi, zt, 1, None)[1].long()
    out.update(composite_top1_equal=round(
        float((k_c == composite(zi, zt, 1)[1]).double().mean()), 4))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="32768,8192")
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--only", choices=["all", "topk"], default="all")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")
    for b in (int(x) for x in args.batches.split(",")):
        print(json.dumps(probe(b, args.dim, args.iters, args.only)),
              flush=True)


if __name__ == "__main__":
    main()
